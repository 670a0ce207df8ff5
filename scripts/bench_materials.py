"""Material baking A/B: (a) the fused kernel (csrc/bake.hip) against the layered path that was the only way to the same arrays before
it -- sdf_network(x) + nets.materials + sigmoid under no_grad -- (b) in chunks of 8192 points, the reference's recipe, and (c) in one
piece where memory allows.  GPU events, median of 5 per variant, the variants run in alternating order on one device; V = 100 000 and
2 500 000 random points in the unit ball.  Prints ms, points/s, achieved TFLOP/s against the fp32-MFMA peak (157.3 TFLOP/s) and the
peak memory the variant allocates on top of the points and the outputs.

    python scripts/bench_materials.py [--points 100000 2500000] [--reps 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402

PEAK = 157.3e12
# algorithmic MACs per point: SDF 39->256, 256->256 x2, 256->217, 256->256 x4, 256->257; three predictors 259->256->256->256->(1, 1, 3)
MACS = (39 * 256 + 2 * 256 * 256 + 256 * 217 + 4 * 256 * 256 + 256 * 257) + 3 * (259 * 256 + 2 * 256 * 256) + 256 * 5
FLOP = 2 * MACS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='+', default=[100000, 2500000])
    ap.add_argument('--reps', type=int, default=5)
    flags = ap.parse_args()
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.materials import bake_materials

    dev = torch.device('cuda:0')
    net = NeROShapeRenderer({}, training=False)
    net.load_param_dict(randomize_for_parity(init_stage1_params(6033), seed=1))
    net = net.to(dev)
    eng = net.engine()
    eng.pack()
    nets = Stage1Nets(eng, net._named())

    def fused(x):
        o = bake_materials(net, x)
        return o['metallic'], o['roughness'], o['albedo']

    def layered_piece(x):
        YX = eng.sdf_forward(addr(x), 3, x.shape[0], keep=False, want_feat=True)['YX']
        s = torch.sigmoid(nets.materials(YX[:, 1:257].contiguous(), x))
        return s[:, 0:1], s[:, 1:2], s[:, 2:5]

    def layered_chunks(x):
        parts = [layered_piece(x[i:i + 8192]) for i in range(0, x.shape[0], 8192)]
        return tuple(torch.cat([p[j] for p in parts], 0) for j in range(3))

    variants = [('fused kernel', fused), ('layered, chunks of 8192', layered_chunks), ('layered, one piece', layered_piece)]
    print(f"{FLOP / 1e6:.3f} MFLOP per point (three predictors; the layered path also evaluates the transmission predictor)")
    for V in flags.points:
        g = np.random.Generator(np.random.PCG64(V))
        d = g.standard_normal((V, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        x = torch.from_numpy((d * g.random((V, 1)) ** (1 / 3)).astype(np.float32)).to(dev)
        times = {n: [] for n, _ in variants}
        mem = {}
        alive = dict(variants)
        with torch.no_grad():
            for rep in range(flags.reps + 1):                       # rep 0: warm-up (allocator, code objects) and the memory figure
                order = list(alive.items())
                if rep % 2:
                    order.reverse()
                for name, fn in order:
                    try:
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        out = fn(x)
                        e1.record()
                        torch.cuda.synchronize()
                        if rep == 0:
                            mem[name] = torch.cuda.max_memory_allocated() - base - sum(o.numel() * 4 for o in out)
                        else:
                            times[name].append(e0.elapsed_time(e1))
                        del out
                    except torch.cuda.OutOfMemoryError:
                        print(f"V={V}: {name}: out of memory, dropped")
                        alive.pop(name)
                eng._cap_classes.clear()
                torch.cuda.empty_cache() if rep == 0 else None
        for name, _ in variants:
            if name not in alive:
                continue
            ms = statistics.median(times[name])
            print(f"V={V:8d}  {name:26s} median {ms:9.3f} ms  (min {min(times[name]):9.3f}, max {max(times[name]):9.3f})  "
                  f"{V / ms * 1e3 / 1e6:8.2f} Mpoints/s  {V * FLOP / ms * 1e3 / 1e12:6.1f} TFLOP/s = {V * FLOP / ms * 1e3 / PEAK:5.3f} of peak  "
                  f"workspace {mem[name] / V:8.0f} B/point")


if __name__ == '__main__':
    main()
