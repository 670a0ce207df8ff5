"""Block-sparse against dense mesh extraction on the stage-1 geometric initialisation (a sphere of radius 0.5), DESIGN.md 37.

  python scripts/bench_extract_mesh_sparse.py --resolution 512 1024 [--block 8] [--repeats 3]
  python scripts/bench_extract_mesh_sparse.py --resolution 2048 --sparse-only

Per resolution: one untimed warm-up of each variant, then `--repeats` rounds in which the dense path (mesh.sdf_grid +
marching_cubes) and the sparse path (mesh_sparse) alternate; device events around every phase, the median of each reported.  The
sparse phases: probe (region geometry + one SDF row per block), evaluate (the rule, the slot table, the SDF on the active blocks,
the outside fill), marching cubes.  Fails (AssertionError) unless both meshes have the same number of vertices and triangles and
the sparse one has no open edges.  --sparse-only (2048^3, whose dense grid does not fit) adds the peak device memory.  One JSON line per
resolution."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(n):
    import torch
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def dense_run(mesh, eng, res):
    import torch
    st = {}
    e = _events(3)
    e[0].record()
    u = mesh.sdf_grid(eng, mesh.BOX_MIN, mesh.BOX_MAX, res, stats=st)
    e[1].record()
    V, F = mesh.marching_cubes(u, 0.0)
    e[2].record()
    torch.cuda.synchronize()
    return dict(grid_ms=e[0].elapsed_time(e[1]), mc_ms=e[1].elapsed_time(e[2]), total_ms=e[0].elapsed_time(e[2]), rows=st['points'],
                Nv=int(V.shape[0]), Nf=int(F.shape[0]))


def sparse_run(mesh, eng, res, block, lipschitz):
    import torch
    from nu_nerf_amd import mesh_sparse
    e = _events(4)
    e[0].record()
    band = mesh_sparse.ProbeBand((eng,), mesh.BOX_MIN, mesh.BOX_MAX, res, block, None)
    e[1].record()
    grid = band.grid(lipschitz)
    e[2].record()
    V, F, n_open = mesh_sparse.marching_cubes_sparse(grid, 0.0)
    e[3].record()
    torch.cuda.synchronize()
    return dict(probe_ms=e[0].elapsed_time(e[1]), evaluate_ms=e[1].elapsed_time(e[2]), mc_ms=e[2].elapsed_time(e[3]),
                total_ms=e[0].elapsed_time(e[3]), probes=band.probes, blocks=grid.nslots, rows=band.rows_evaluated, open_edges=n_open,
                Nv=int(V.shape[0]), Nf=int(F.shape[0]))


def _median(runs):
    return {k: (round(statistics.median(r[k] for r in runs), 3) if k.endswith('_ms') else runs[-1][k]) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument('--resolution', type=int, nargs='+', default=[512])
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--lipschitz', type=float, default=2.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--sparse-only', action='store_true')
    a = ap.parse_args()
    import torch
    from nu_nerf_amd import mesh
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params
    dev = torch.device('cuda:0')
    net = NeROShapeRenderer({'is_nerf': True}, training=False)
    net.load_param_dict(init_stage1_params(6033))
    eng = net.to(dev).engine()
    dense_run(mesh, eng, 64)                                               # allocator classes, code objects
    sparse_run(mesh, eng, 64, a.block, a.lipschitz)
    for res in a.resolution:
        if not a.sparse_only:
            dense_run(mesh, eng, res)
        sparse_run(mesh, eng, res, a.block, a.lipschitz)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        dense, sparse = [], []
        for _ in range(a.repeats):
            if not a.sparse_only:
                dense.append(dense_run(mesh, eng, res))
            sparse.append(sparse_run(mesh, eng, res, a.block, a.lipschitz))
        assert all(r['open_edges'] == 0 for r in sparse), sparse
        assert all((d['Nv'], d['Nf']) == (r['Nv'], r['Nf']) for d, r in zip(dense, sparse)), (dense, sparse)
        out = dict(resolution=res, block=a.block, lipschitz=a.lipschitz, repeats=a.repeats, sparse=_median(sparse))
        if dense:
            out['dense'] = _median(dense)
            out['rows_ratio'] = round(out['sparse']['rows'] / out['dense']['rows'], 4)
            out['speedup'] = round(out['dense']['total_ms'] / out['sparse']['total_ms'], 2)
            out['same_counts'] = (out['dense']['Nv'], out['dense']['Nf']) == (out['sparse']['Nv'], out['sparse']['Nf'])
        else:
            out['peak_memory_gb'] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
