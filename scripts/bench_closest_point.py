"""Report aid: closest-point queries per second of LBVH.closest_points (nu_lbvh_closest) on icospheres of 20 480, 327 680 and
1 310 720 faces (subdiv 5, 7, 8) with 2^20 queries of three kinds -- near the surface (the vertices of an r = 0.45 icosphere of
subdiv 8, cycled to 2^20, against r = 0.5: the postprocess case), area-weighted samples of the mesh itself, uniform in [-1, 1]^3, also split into
its points inside and outside the r = 0.5 sphere -- and the speed-up over the O(N*F) sweep (nu_brute_closest) at 20 480 faces x 65 536 near-surface queries.  Device events around
`--reps` calls after `--warmup` calls; one JSON line."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from nu_nerf_amd.lbvh import LBVH, icosphere
from nu_nerf_amd.mesh import sample_surface


def timed_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subdivs', type=int, nargs='+', default=[5, 7, 8])
    ap.add_argument('--queries', type=int, default=1 << 20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n = args.queries
    near_v, _ = icosphere(8, 0.45)
    near = torch.from_numpy(near_v[np.arange(n) % len(near_v)]).to(dev)
    uniform = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
    out = {'queries': n, 'meshes': []}
    for sub in args.subdivs:
        V, F = icosphere(sub, 0.5)
        Vt, Ft = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
        bvh = LBVH(Vt, Ft)
        row = {'faces': int(len(F))}
        inner = uniform.norm(dim=1) < 0.5
        sets = (('near', near), ('surface', sample_surface(Vt, Ft, n, seed=1)), ('uniform', uniform),
                ('uniform_inside', uniform[inner].contiguous()), ('uniform_outside', uniform[~inner].contiguous()))
        for name, P in sets:
            ms = timed_ms(lambda: bvh.closest_points(P), args.warmup, args.reps)
            row[name] = {'queries': len(P), 'ms': round(ms, 4), 'Gq_per_s': round(len(P) / ms / 1e6, 4)}
        out['meshes'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    V, F = icosphere(5, 0.5)
    bvh = LBVH(torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev))
    P = near[:65536].contiguous()
    lb = timed_ms(lambda: bvh.closest_points(P), args.warmup, args.reps)
    br = timed_ms(lambda: bvh.closest_points_brute(P), 1, 3)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bvh.closest_points(P), bvh.closest_points_brute(P)))
    out['brute'] = {'faces': int(len(F)), 'queries': 65536, 'lbvh_ms': round(lb, 4), 'brute_ms': round(br, 4),
                    'speedup': round(br / lb, 1), 'bit_identical': same}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
