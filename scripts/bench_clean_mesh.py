"""Report aid: component labelling, statistics and compaction (nu_nerf_amd.components, csrc/components.hip) on a marching-cubes mesh
of an analytic r = 0.5 sphere plus seeded blobs at `--res`^3 (1024: about 2.5 M faces).  Per connectivity: ms of the half-edge sort
both share, of the labelling (links, rounds, renumbering) with its rounds, of the statistics and of the compaction that keeps the
largest component -- device events, `--warmup` calls first, the median of `--reps`.  Also the seconds the numpy union-find of
tests/components_oracle.py takes for the same labelling on the host (--no-oracle skips it) and whether the labels agree.  One JSON
line per connectivity on stderr, all of them on stdout at the end."""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from nu_nerf_amd import components as C
from nu_nerf_amd.mesh import marching_cubes


def blob_mesh(res, dev, n_blobs=32, seed=0):
    """Sphere of radius 0.5 and n_blobs small balls (radius 0.01 .. 0.03) between it and the unit sphere, as one marching-cubes mesh."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_blobs, 3))
    centres = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.6, 0.9, (n_blobs, 1))
    radii = rng.uniform(0.01, 0.03, n_blobs)
    x = torch.linspace(-1.0, 1.0, res, device=dev)
    u = torch.empty(res, res, res, device=dev)
    xs = x.double().cpu().numpy()
    for i in range(res):                                   # slab by slab: a 1024^3 float64 meshgrid would not fit
        X, Y, Z = torch.meshgrid(x[i:i + 1].double(), x.double(), x.double(), indexing='ij')
        s = torch.sqrt(X * X + Y * Y + Z * Z) - 0.5
        for c, r in zip(centres, radii):
            if abs(xs[i] - c[0]) < r + 4.0 / res:
                s = torch.minimum(s, torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r)
        u[i] = s.float()[0]
    V, F = marching_cubes(u, 0.0)
    V = V * (2.0 / (res - 1)) - 1.0
    return V.contiguous(), F.flip(1).contiguous()


def timed(fn, warmup, reps):
    """(median ms of `reps` calls after `warmup`, the last result)."""
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-oracle', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    V, F = blob_mesh(args.res, dev)
    Vh, Fh = V.cpu().numpy(), F.cpu().numpy()
    rows = []
    for connectivity in C.CONNECTIVITIES:
        sort_ms, edges = timed(lambda: C._sorted_edges(F), args.warmup, args.reps)
        label_ms, (fl, _, ncomp, rounds) = timed(lambda: C._components(V, F, connectivity, C.MAX_ROUNDS, edges), args.warmup, args.reps)
        stats_ms, table = timed(lambda: C._stats(V, F, fl, ncomp, edges), args.warmup, args.reps)
        mask = C.select_components(C._host_table(table))
        keep = torch.from_numpy(mask.astype(np.int32)).to(dev)
        compact_ms, (Vk, Fk) = timed(lambda: C._compact(V, F, fl, keep), args.warmup, args.reps)
        total_ms, _ = timed(lambda: C.remove_floaters(V, F, connectivity=connectivity), args.warmup, args.reps)
        row = {'res': args.res, 'connectivity': connectivity, 'vertices': int(len(V)), 'faces': int(len(F)), 'components': ncomp,
               'rounds': rounds, 'edge_sort_ms': sort_ms, 'label_ms': label_ms, 'stats_ms': stats_ms, 'compact_ms': compact_ms,
               'remove_floaters_ms': total_ms, 'faces_kept': int(len(Fk))}
        if not args.no_oracle:
            import components_oracle as O
            t0 = time.perf_counter()
            ofl, _, oC = O.connected_components(Vh, Fh, connectivity)
            row['oracle_label_s'] = round(time.perf_counter() - t0, 2)
            row['labels_equal'] = bool(oC == ncomp and np.array_equal(ofl, fl.cpu().numpy()))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
