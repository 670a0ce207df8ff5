"""Environment bake A/B: the fused kernel (csrc/light_bake.hip) against the layered composition that reaches the same radiance on the
same rows -- nu_ide of the direction (| nu_ide of the sphere point) into the outer_light input rows, relu_stack_fwd (three NT GEMMs
with their ReLU sign masks), skinny_fwd, torch exp(min(., exp_max)) -- under no_grad.  Two workloads: the 256 x 512 map at five
roughness levels (655 360 rows, what extract_environment bakes by default) and one 512 x 1024 level (524 288 rows).  GPU events around
each variant, one warm-up round, median of --reps, the two variants in alternating order on one device.  Prints ms, Mrows/s, achieved
TFLOP/s against the fp32-MFMA peak (157.3 TFLOP/s) and the device memory each variant allocates on top of the rows and the result.

    python scripts/bench_environment.py [--reps 9] [--sphere]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sphere', action='store_true', help="shader_config.sphere_direction: 144 input columns instead of 72")
    flags = ap.parse_args()
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.environment import bake_light, latlong_dirs
    from nu_nerf_amd import torch_glue as G
    from nu_nerf_amd.shading_glue import sphere_point

    dev = torch.device('cuda:0')
    net = NeROShapeRenderer({'shader_config': {'sphere_direction': flags.sphere}}, training=False)
    net.load_param_dict(randomize_for_parity(init_stage1_params(6033, sphere_direction=flags.sphere), seed=1))
    net = net.to(dev)
    eng = net.engine()
    eng.pack()
    k_in = 144 if flags.sphere else 72
    flop = 2 * (k_in * 256 + 2 * 256 * 256 + 256 * 3)               # algorithmic, per row
    head = eng.outer_light[3]

    def fused(d, k):
        return bake_light(net, d, k)['light']

    def layered(d, k):
        n = d.shape[0]
        rows = eng.zeros(n, eng.ld_ol)
        rows[:, :72] = G.ide(d, k[:, None])
        if flags.sphere:
            rows[:, 72:144] = G.ide(sphere_point(torch.zeros_like(d), d), k[:, None])
        Hs = eng.relu_stack_fwd(eng.outer_light, rows, eng.ld_ol, n)
        raw = eng.empty(n, 4)
        eng.skinny_fwd(addr(Hs[2]), 256, n, 256, addr(*head.Wp), 256, addr(head.b), 3, addr(raw), 4)
        return torch.exp(torch.clamp(raw[:, :3], max=eng.exp_max))

    variants = [('fused kernel', fused), ('layered composition', layered)]
    print(f"{flop / 1e6:.3f} MFLOP per row (outer_light, {k_in} input columns)")
    for name, h, w, levels in (('256 x 512 x 5 levels', 256, 512, (0.0, 0.25, 0.5, 0.75, 1.0)), ('512 x 1024 x 1 level', 512, 1024, (0.0,))):
        dirs = latlong_dirs(h, w)
        d = torch.from_numpy(np.tile(dirs, (len(levels), 1))).to(dev)
        k = torch.from_numpy(np.repeat(np.asarray(levels, np.float32), h * w)).to(dev)
        n = d.shape[0]
        times = {v: [] for v, _ in variants}
        mem, res = {}, {}
        with torch.no_grad():
            for rep in range(flags.reps + 1):                       # rep 0: warm-up (allocator, code objects), memory and the result
                order = list(variants)
                if rep % 2:
                    order.reverse()
                for v, fn in order:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn(d, k)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep == 0:
                        mem[v] = torch.cuda.max_memory_allocated() - base - out.numel() * 4
                        res[v] = out.clone()
                    else:
                        times[v].append(e0.elapsed_time(e1))
                    del out
                eng._cap_classes.clear()
        diff = float(((res['fused kernel'] - res['layered composition']).abs() / res['layered composition']).max())
        print(f"{name}: {n} rows; fused vs layered result: max relative difference {diff:.2e}")
        ms = {v: statistics.median(times[v]) for v, _ in variants}
        for v, _ in variants:
            print(f"  {v:20s} median {ms[v]:8.3f} ms  (min {min(times[v]):8.3f}, max {max(times[v]):8.3f})  {n / ms[v] * 1e3 / 1e6:7.2f} Mrows/s  "
                  f"{n * flop / ms[v] * 1e3 / 1e12:6.1f} TFLOP/s = {n * flop / ms[v] * 1e3 / PEAK:5.3f} of peak  workspace {mem[v] / n:7.0f} B/row")
        print(f"  layered / fused = {ms['layered composition'] / ms['fused kernel']:.2f}")


if __name__ == '__main__':
    main()
