"""Report aid: remesh.remesh_isotropic (csrc/remesh.hip) on marching-cubes meshes of the analytic r = 0.5 sphere at 256^3, 512^3
and 1024^3 with the default arguments (target length and surface distance 0.5 % of the bounding-box diagonal, 3 iterations):
ms per call (device events around `--reps` calls after `--warmup`), faces in and out, split edges and collapse / flip rounds per
iteration, and the Hausdorff distance to the input (mesh.mesh_distance).  One JSON line per resolution on stderr, all of them on
stdout at the end."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from nu_nerf_amd.mesh import marching_cubes, mesh_distance, remesh_isotropic


def sphere_mesh(res, dev):
    x = torch.linspace(-1.0, 1.0, res, device=dev)
    u = torch.empty(res, res, res, device=dev)
    for i in range(res):                                   # slab by slab: a 1024^3 float64 meshgrid would not fit
        X, Y, Z = torch.meshgrid(x[i:i + 1].double(), x.double(), x.double(), indexing='ij')
        u[i] = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.5).float()[0]
    V, F = marching_cubes(u, 0.0)
    V = V * (2.0 / (res - 1)) - 1.0
    return V.contiguous(), F.flip(1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512, 1024])
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = []
    for res in args.res:
        V, F = sphere_mesh(res, dev)
        stats = {}
        for _ in range(args.warmup):
            remesh_isotropic(V, F)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            Vr, Fr = remesh_isotropic(V, F, stats=stats)
        e1.record()
        torch.cuda.synchronize()
        d = mesh_distance((Vr, Fr), (V, F), n_samples=1_000_000)
        row = {'res': res, 'faces_in': int(len(F)), 'faces_out': int(len(Fr)), 'ms': round(e0.elapsed_time(e1) / args.reps, 2),
               'splits': stats['splits'], 'collapse_rounds': stats['collapse_rounds'], 'flip_rounds': stats['flip_rounds'],
               'target_len': stats['target_len'], 'hausdorff': d['hausdorff'], 'max_surf_dist': stats['max_surf_dist']}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
