"""python -m nu_nerf_amd.prefilter_environment --hdr FILE [--out DIR] [--height H] [--width W] [--roughness R ...] [--lobe ggx|vmf]
[--diffuse cosine|vmf] [--sh]

A foreign lat-long HDR environment prefiltered into the roughness pyramid of the split-sum appearance model: level l is
the map seen through the lobe of roughness R_l, the diffuse map the cosine-weighted mean (environment.prefilter; one launch of the
nu_env_prefilter kernel, levels narrower than the source grid are its bilinear tap).

It writes DIR (default data/environment/{stem of FILE}-prefiltered) in the layout extract_environment uses: env.npy [H,W,3] float32 and
env.hdr, the map at the FIRST roughness; env_pyramid.npy [L,H,W,3] and roughness.npy [L]; env_diffuse.npy [H,W,3]; env.png, an sRGB
preview of env.npy -- and prints one JSON line.  `python -m nu_nerf_amd.relight --splitsum --pyramid DIR ...` renders under it.
--hdr takes a Radiance .hdr or a .npy float [H,W,3]; --height / --width default to the source's.  --sh also writes env_sh.npy [9,3], the
order-2 spherical-harmonic coefficients of the SOURCE map (environment.project_sh), which relight --transfer --occlusion sh reads.
"""
import argparse
import json
import os
import sys

FILES = (('env', 'env.npy'), ('hdr', 'env.hdr'), ('pyramid', 'env_pyramid.npy'), ('roughness', 'roughness.npy'),
         ('diffuse', 'env_diffuse.npy'), ('png', 'env.png'))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.prefilter_environment", description=__doc__.split("\n\n")[1])
    ap.add_argument('--hdr', type=str, required=True, help="environment map: Radiance .hdr or .npy float [H,W,3]")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/environment/{stem}-prefiltered)")
    ap.add_argument('--height', type=int, default=None)
    ap.add_argument('--width', type=int, default=None)
    ap.add_argument('--roughness', type=float, nargs='+', default=[0.0, 0.25, 0.5, 0.75, 1.0], help="roughness levels of the pyramid")
    ap.add_argument('--lobe', choices=('ggx', 'vmf'), default='ggx', help="the specular lobe of the levels")
    ap.add_argument('--diffuse', choices=('cosine', 'vmf'), default='cosine', help="the lobe of the diffuse map")
    ap.add_argument('--sh', action='store_true', default=False, help="also write env_sh.npy, the SH coefficients [9,3] of the source map")
    flags = ap.parse_args(argv)
    if (flags.height is not None and flags.height < 1) or (flags.width is not None and flags.width < 1):
        ap.error("--height and --width must be >= 1")
    if any(r < 0.0 for r in flags.roughness) or sorted(set(flags.roughness)) != flags.roughness or len(flags.roughness) > 16:
        ap.error("--roughness takes at most 16 ascending values >= 0")
    return flags


def output_dir(flags):
    stem = os.path.splitext(os.path.basename(flags.hdr))[0]
    return flags.out or os.path.join('data', 'environment', f'{stem}-prefiltered')


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    from .environment import prefilter, project_sh, write_hdr
    from .relight import read_hdr, to_srgb8, write_png

    src = read_hdr(flags.hdr)
    levels = np.asarray(flags.roughness, np.float32)
    pyramid, diffuse, info = prefilter(src, levels, flags.height, flags.width, flags.lobe, flags.diffuse)
    out = output_dir(flags)
    os.makedirs(out, exist_ok=True)
    paths = {k: os.path.join(out, f) for k, f in FILES}
    env = np.ascontiguousarray(pyramid[0])
    np.save(paths['env'], env)
    write_hdr(paths['hdr'], env)
    np.save(paths['pyramid'], pyramid)
    np.save(paths['roughness'], levels)
    np.save(paths['diffuse'], diffuse)
    if flags.sh:
        paths['sh'] = os.path.join(out, 'env_sh.npy')
        np.save(paths['sh'], project_sh(src))
    h, w = env.shape[:2]
    write_png(paths['png'], to_srgb8(torch.cat([torch.from_numpy(env), torch.ones(h, w, 1)], -1)))
    print(json.dumps({'shape': list(pyramid.shape), 'roughness': [float(r) for r in levels], 'source': list(src.shape[:2]),
                      'lobe': flags.lobe, 'diffuse': flags.diffuse, 'tapped': info['tapped'], 'pairs': info['pairs'],
                      'min': float(env.min()), 'max': float(env.max()), 'mean': float(env.mean()), 'paths': paths}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
