"""python -m nu_nerf_amd.bake_transfer --mesh PLY [--samples 1024] [--radius R] [--seed 0] [--eps E] [--trans] [--out DIR]

Per-vertex visibility transfer of a mesh (transfer.py; one fused kernel): `--samples` cosine-weighted hemisphere rays per
vertex (a multiple of 16) about its angle-weighted normal are traced against the mesh itself, and DIR/ao.npy [V,1] (ambient occlusion:
the unoccluded share), DIR/bent_normal.npy [V,3] (the mean unoccluded direction, unit) and DIR/transfer.npy [V,9] (the order-2
spherical-harmonic transfer vector) are written: float32, in the vertex order of the PLY, beside the material arrays.
`python -m nu_nerf_amd.relight --splitsum ... --transfer DIR` renders shadowed frames with them; ao.npy is the occlusion channel of a
glTF / DCC material.

--out defaults to data/materials/{stem of PLY}.  --radius: occluders farther away than this do not count (default: unbounded).
--eps: rays start eps along the normal (default relight's origin offset).  --trans turns the mesh +90 degrees about x, as relight
--trans does (the bent normals and the transfer vectors are in the turned frame).  Prints one JSON line.
"""
import argparse
import json
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.bake_transfer", description=__doc__.split("\n\n")[1])
    ap.add_argument('--mesh', type=str, required=True, help="triangle mesh (PLY)")
    ap.add_argument('--samples', type=int, default=1024, help="hemisphere rays per vertex, a multiple of 16")
    ap.add_argument('--radius', type=float, default=None, help="occluders farther than this do not count (default: unbounded)")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eps', type=float, default=None, help="ray origin offset along the normal (default relight.ORIGIN_EPS)")
    ap.add_argument('--trans', action='store_true', default=False, help="turn the mesh +90 degrees about x (as relight --trans)")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/materials/{stem of the mesh})")
    flags = ap.parse_args(argv)
    if flags.samples < 16 or flags.samples % 16:
        ap.error("--samples must be a multiple of 16 and >= 16")
    if flags.radius is not None and not (0.0 < flags.radius < float('inf')):
        ap.error("--radius must be > 0 and finite")
    if flags.eps is not None and not (float('-inf') < flags.eps < float('inf')):
        ap.error("--eps must be finite")
    return flags


def output_dir(flags):
    return flags.out or os.path.join('data', 'materials', os.path.splitext(os.path.basename(flags.mesh))[0])


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    from . import mesh as M
    from .relight import TRANS
    from .transfer import bake_transfer, save_transfer_dir

    V, F = M.read_ply(flags.mesh)
    if flags.trans:
        V = (np.asarray(V, np.float64) @ TRANS.T).astype(np.float32)
    V, F = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.int32)
    rows = bake_transfer(V, F, flags.samples, flags.seed, flags.eps, flags.radius)
    out = output_dir(flags)
    paths = save_transfer_dir(out, rows)
    ao = rows[:, 9].cpu().numpy()
    print(json.dumps({'mesh': flags.mesh, 'out': out, 'V': int(len(V)), 'F': int(len(F)), 'samples': flags.samples,
                      'radius': flags.radius, 'ao_min': float(ao.min()), 'ao_mean': float(ao.mean()), 'ao_max': float(ao.max()),
                      'paths': paths}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
