"""python -m nu_nerf_amd.mesh_distance A.ply B.ply [--samples N] [--seed S]

How close two triangle meshes are: N area-weighted surface samples of each, the distance of every sample to the other mesh
(closest points on the GPU LBVH), and one JSON line with a_to_b_mean, b_to_a_mean, chamfer (their mean), a_to_b_max, b_to_a_max
and hausdorff (the larger maximum) -- mesh.mesh_distance.
"""
import argparse
import json
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.mesh_distance", description=__doc__.split("\n\n")[1])
    ap.add_argument('a', type=str, help="mesh A (PLY)")
    ap.add_argument('b', type=str, help="mesh B (PLY)")
    ap.add_argument('--samples', type=int, default=1_000_000, help="surface samples per mesh (default 1 000 000)")
    ap.add_argument('--seed', type=int, default=0, help="sampling seed (default 0)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from .mesh import read_ply, mesh_distance
    res = mesh_distance(read_ply(args.a), read_ply(args.b), n_samples=args.samples, seed=args.seed)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
