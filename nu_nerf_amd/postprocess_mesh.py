"""python -m nu_nerf_amd.postprocess_mesh --inner PLY --outer PLY [--min-dist 0.055] [--out PLY]

postprocess_stage2_mesh.py with its paths as arguments: every face of the inner (stage-2) mesh whose three vertices all lie within
min_dist of the outer (stage-1) mesh is dropped -- the faces the stage-2 field's torch.where seam puts on the outer shell
(mesh.remove_faces_near; closest points on the GPU LBVH).  Writes <inner stem>_cleaned.ply next to the input unless --out is given.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.postprocess_mesh", description=__doc__.split("\n\n")[1])
    ap.add_argument('--inner', type=str, required=True, help="stage-2 inner mesh (PLY)")
    ap.add_argument('--outer', type=str, required=True, help="stage-1 outer mesh (PLY)")
    ap.add_argument('--min-dist', type=float, default=0.055, help="keep faces whose vertices all lie farther than this (default 0.055)")
    ap.add_argument('--out', type=str, default=None, help="output PLY (default <inner stem>_cleaned.ply next to the input)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from .mesh import read_ply, write_ply, remove_faces_near
    Vi, Fi = read_ply(args.inner)
    Vo, Fo = read_ply(args.outer)
    V, F = remove_faces_near(Vi, Fi, Vo, Fo, min_dist=args.min_dist)
    out = args.out or os.path.splitext(args.inner)[0] + "_cleaned.ply"
    write_ply(out, V, F)
    print(f"inner mesh: {len(Vi)} vertices, {len(Fi)} faces -> {len(V)} vertices, {len(F)} faces; wrote {out}")
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
