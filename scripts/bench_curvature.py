"""Curvature bake A/B: (a) the fused jet kernel (csrc/sdf_jet.hip: value, gradient, Hessian and curvatures in one launch) against (b) ten
times the per-point time of nu_sdf_fused_fwd at the same point count -- the arithmetic floor: the jet carries ten rows per point through
the same layers -- and (c) the only composition that gave a Hessian before the kernel: three Hessian-vector passes through the layered
SdfFn path (forward with kept activations, normal, second-order backward with the cotangent e_i on the normal; one pass per row of H).
GPU events, median of 5 per variant, the variants run in alternating order on one device; random points at radius 0.2 .. 0.95.
Prints ms per call, the achieved TFLOP/s against the fp32-MFMA peak (157.3 TFLOP/s), the two ratios and the memory a variant allocates on
top of the points and its outputs.

    python scripts/bench_curvature.py [--points 131072 1048576] [--reps 5]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402

PEAK = 157.3e12
# algorithmic MACs per row of the SDF network with the sdf head only: 39->256, 256->256 x2, 256->217, 256->256 x4, 256->1; the jet carries
# ten rows per point
MACS = 39 * 256 + 2 * 256 * 256 + 256 * 217 + 4 * 256 * 256 + 256
FLOP_JET = 2 * MACS * 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='+', default=[131072, 1048576])
    ap.add_argument('--reps', type=int, default=5)
    flags = ap.parse_args()
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.curvature import bake_curvature

    dev = torch.device('cuda:0')
    net = NeROShapeRenderer({}, training=False)
    net.load_param_dict(randomize_for_parity(init_stage1_params(6033), seed=1))
    net = net.to(dev)
    eng = net.engine()
    eng.pack()
    nets = Stage1Nets(eng, net._named())

    def jet(x):
        with torch.no_grad():
            o = bake_curvature(net, x, hessian=True)
        return tuple(o.values())

    def fused_value(x):
        sdf = torch.empty(x.shape[0], device=dev)
        eng.lib.nu_sdf_fused_fwd(ctypes.byref(eng._sdf_net), addr(x), 3, x.shape[0], addr(sdf), eng.stream())
        return (sdf,)

    def three_hvp(x):
        rows = []
        for i in range(3):
            xi = x.detach().requires_grad_(True)
            _, n = nets.sdf(xi)
            rows.append(torch.autograd.grad(n[:, i].sum(), xi)[0])
        for p in net.parameters():                                  # the passes also accumulate parameter gradients nobody wants
            p.grad = None
        return (torch.stack(rows, 1),)

    variants = [('jet kernel', jet), ('nu_sdf_fused_fwd (value only)', fused_value), ('3 HVP passes, layered', three_hvp)]
    for V in flags.points:
        g = np.random.Generator(np.random.PCG64(V))
        d = g.standard_normal((V, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        x = torch.from_numpy((d * g.uniform(0.2, 0.95, (V, 1))).astype(np.float32)).to(dev)
        times = {n: [] for n, _ in variants}
        mem = {}
        alive = dict(variants)
        for rep in range(flags.reps + 1):                           # rep 0: warm-up (allocator, code objects) and the memory figure
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
        med = {n: statistics.median(times[n]) for n in alive}
        for name, _ in variants:
            if name in alive:
                print(f"V={V:8d}  {name:30s} median {med[name]:9.3f} ms  (min {min(times[name]):9.3f}, max {max(times[name]):9.3f})  "
                      f"{V / med[name] * 1e3 / 1e6:8.2f} Mpoints/s  workspace {mem[name] / V:8.0f} B/point")
        j = med.get('jet kernel')
        if j:
            print(f"V={V:8d}  jet kernel: {FLOP_JET / 1e6:.3f} MFLOP per point (ten rows), {V * FLOP_JET / j * 1e3 / 1e12:6.1f} TFLOP/s = "
                  f"{V * FLOP_JET / j * 1e3 / PEAK:5.3f} of the fp32-MFMA peak (call time, one launch)")
        if j and 'nu_sdf_fused_fwd (value only)' in med:
            print(f"V={V:8d}  jet / (10 x value-only) = {j / (10.0 * med['nu_sdf_fused_fwd (value only)']):.3f}")
        if j and '3 HVP passes, layered' in med:
            print(f"V={V:8d}  jet / 3 HVP passes     = {j / med['3 HVP passes, layered']:.3f}  ({med['3 HVP passes, layered'] / j:.2f} x faster)")


if __name__ == '__main__':
    main()
