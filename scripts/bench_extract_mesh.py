"""Mesh extraction time at one resolution: the device SDF grid (mesh.sdf_grid) and marching cubes (mesh.marching_cubes), each timed
with events around one warm run.  Network: the stage-1 geometric initialisation (a sphere of radius 0.5, the shape a trained
stage-1 SDF starts from).  Prints one JSON line.

  python scripts/bench_extract_mesh.py --resolution 512
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_PEAK_TFLOPS = 157.3
# SDF MLP FLOPs per point with the sdf column only: lin0 39x256, lin1-2 256x256, lin3 256x217, lin4-7 256x256, lin8 256x1
FLOP_PER_POINT = 2 * (39 * 256 + 2 * 256 * 256 + 256 * 217 + 4 * 256 * 256 + 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--slab-points', type=int, default=None)
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--no-warm-run', action='store_true', help="skip the untimed extraction at the full resolution (profiler runs)")
    a = ap.parse_args()
    import torch
    from nu_nerf_amd import mesh
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params
    dev = torch.device('cuda:0')
    net = NeROShapeRenderer({'is_nerf': True}, training=False)
    net.load_param_dict(init_stage1_params(6033))
    net = net.to(dev)
    eng = net.engine()
    res = a.resolution
    box = mesh.BOX_MIN, mesh.BOX_MAX
    mesh.marching_cubes(mesh.sdf_grid(eng, *box, 64), 0.0)                  # warm-up: allocator classes, code objects
    if not a.no_warm_run:
        u = mesh.sdf_grid(eng, *box, res, slab_points=a.slab_points)
        mesh.marching_cubes(u, 0.0)
        del u
    grid_ms, mc_ms = [], []
    for _ in range(a.repeats):
        st = {}
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t0 = time.perf_counter()
        e0.record()
        u = mesh.sdf_grid(eng, *box, res, slab_points=a.slab_points, stats=st)
        e1.record()
        V, F = mesh.marching_cubes(u, 0.0)
        e2.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        grid_ms.append(e0.elapsed_time(e1))
        mc_ms.append(e1.elapsed_time(e2))
        del u
    g, m = min(grid_ms), min(mc_ms)
    tflops = st['points'] * FLOP_PER_POINT / (g * 1e-3) / 1e12
    print(json.dumps({'resolution': res, 'grid_ms': round(g, 3), 'mc_ms': round(m, 3), 'wall_ms': round(wall, 3),
                      'mc_share': round(m / (g + m), 4), 'Nv': int(V.shape[0]), 'Nf': int(F.shape[0]),
                      'inside_points': st['points'], 'slabs': st['slabs'], 'flop_per_point': FLOP_PER_POINT,
                      'grid_tflops': round(tflops, 2), 'grid_frac_of_fp32_mfma_peak': round(tflops / FP32_MFMA_PEAK_TFLOPS, 4)}))


if __name__ == "__main__":
    main()
