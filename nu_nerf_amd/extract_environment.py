"""python -m nu_nerf_amd.extract_environment --cfg CFG [--ckpt PATH] [--stage2] [--which outer|inner] [--height H] [--width W]
[--roughness R ...] [--point X Y Z] [--probe] [--sh] [--out DIR]

The illumination a trained model learned, exported as a lat-long environment map: the renderer named by the config loads
data/model/{name}/model.pth (train_glue.save_checkpoint format, as extract_materials does) and the light predictors are evaluated at
the texel-centre directions of the map by one fused kernel (environment.bake_light), once per roughness level in the same launch.

It writes DIR (default data/environment/{name}-{step}): env.npy [H,W,3] float32 and env.hdr (Radiance RGBE), the map at the FIRST
roughness given (default 0, the mirror query); env_pyramid.npy [L,H,W,3] and roughness.npy [L], every level; env.png, an sRGB preview
of env.npy -- and prints one JSON line (shape, min / max / mean radiance, the paths).  The map is in relight's convention, so
`python -m nu_nerf_amd.relight --hdr DIR/env.hdr ...` re-renders the baked mesh under the illumination it was trained under.
--point: where the environment is seen from (default the origin; with `sphere_direction` the outer light depends on it).  --probe:
the blended light at --point (indirect light, occlusion and direct light) instead of the direct light alone.  --stage2: a stage-2
config; --which outer (default) evaluates the stage-1 networks the model carries, --which inner the inner shading network's.
--sh also writes env_sh.npy [9,3], the order-2 spherical-harmonic coefficients of env.npy (environment.project_sh), which
relight --transfer --occlusion sh reads.
"""
import argparse
import json
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.extract_environment", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth)")
    ap.add_argument('--stage2', action='store_true', help="the config is a stage-2 config")
    ap.add_argument('--which', choices=('outer', 'inner'), default=None, help="stage 2: whose light predictors (default outer)")
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--roughness', type=float, nargs='+', default=[0.0, 0.25, 0.5, 0.75, 1.0], help="roughness levels of the pyramid")
    ap.add_argument('--point', type=float, nargs=3, default=None, metavar=('X', 'Y', 'Z'), help="where the map is seen from (default the origin)")
    ap.add_argument('--probe', action='store_true', help="the blended light at --point instead of the direct light")
    ap.add_argument('--sh', action='store_true', default=False, help="also write env_sh.npy, the SH coefficients [9,3] of env.npy")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/environment/{name}-{step})")
    flags = ap.parse_args(argv)
    if flags.which == 'inner' and not flags.stage2:
        ap.error("--which inner needs --stage2")
    if flags.height < 1 or flags.width < 1:
        ap.error("--height and --width must be >= 1")
    if any(r < 0.0 for r in flags.roughness):
        ap.error("--roughness values must be >= 0")
    return flags


def output_dir(flags, name, step):
    return flags.out or os.path.join('data', 'environment', f'{name}-{step}')


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    import yaml
    from .environment import environment_map, project_sh, write_hdr
    from .extract_mesh import _renderer
    from .relight import to_srgb8, write_png
    from .train_glue import load_checkpoint

    with open(flags.cfg) as fh:
        cfg = yaml.safe_load(fh)
    network = _renderer(cfg)
    is_s2 = hasattr(network, 'stage1_network')
    if is_s2 != flags.stage2:
        raise SystemExit(f"config network {cfg['network']!r} is{'' if is_s2 else ' not'} a stage-2 model: "
                         f"{'pass' if is_s2 else 'drop'} --stage2")
    ckpt = flags.ckpt or f'data/model/{cfg["name"]}/model.pth'
    _, step = load_checkpoint(ckpt, network, map_location='cpu')
    if flags.stage2:
        s1_ckpt = network.cfg.get('stage1_ckpt_dir')
        if s1_ckpt and os.path.exists(s1_ckpt):                # as extract_materials --stage2: stage 1 from its own checkpoint
            load_checkpoint(s1_ckpt, network.stage1_network, map_location='cpu')
    network = network.eval().to(torch.device('cuda', torch.cuda.current_device()))
    print(f'successfully load {cfg["name"]} step {step}!')
    out = output_dir(flags, cfg['name'], step)
    os.makedirs(out, exist_ok=True)
    levels = np.asarray(flags.roughness, np.float32)
    pyramid = environment_map(network, flags.height, flags.width, levels, flags.point, flags.which, flags.probe)
    env = np.ascontiguousarray(pyramid[0])
    paths = {k: os.path.join(out, f) for k, f in (('env', 'env.npy'), ('hdr', 'env.hdr'), ('pyramid', 'env_pyramid.npy'),
                                                  ('roughness', 'roughness.npy'), ('png', 'env.png'))}
    np.save(paths['env'], env)
    write_hdr(paths['hdr'], env)
    np.save(paths['pyramid'], pyramid)
    np.save(paths['roughness'], levels)
    if flags.sh:
        paths['sh'] = os.path.join(out, 'env_sh.npy')
        np.save(paths['sh'], project_sh(env))
    rgba = torch.cat([torch.from_numpy(env), torch.ones(flags.height, flags.width, 1)], -1)
    write_png(paths['png'], to_srgb8(rgba))
    print(json.dumps({'shape': list(pyramid.shape), 'roughness': [float(r) for r in levels], 'min': float(env.min()),
                      'max': float(env.max()), 'mean': float(env.mean()), 'paths': paths}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
