"""python -m nu_nerf_amd.render_surface --cfg CFG [--ckpt PATH|none] [--stage2 [--which inner|outer]] [--poses relight|FILE.npz] [--hw 800] [--aovs ...] [--out DIR]

Pictures of the surface the SDF has learned, seen from cameras, without a mesh (sdf_trace.py: one fused sphere-tracing kernel per
frame, then the curvature jet and the material bake at the hit points): the renderer named by the config loads
data/model/{name}/model.pth (as extract_curvature does; --ckpt none renders the freshly initialised model as step 0) and, for frame k
and every requested AOV, DIR/{k}_{aov}.png is written, plus DIR/{k}_depth.npy (float32 [h,w], t along the unit ray, 0 where missed).

--poses relight (default): the camera orbit of the relight command (relight.relighting_poses with --num, --azimuth, --elevation,
--cam_dist; relight.intrinsics at --hw).  --poses FILE.npz: 'poses' [n,3,4] world -> camera and optionally 'K' [3,3].  --out defaults to
data/surface/{name}-{step}.  --stage2: a stage-2 config; --which inner (default) traces the inner SDF, outer the stage-1 SDF it
carries.  PNG encoding (RGBA, alpha = the mask): depth scaled to the frame's hit range, normal and position as 0.5 + 0.5 v, materials
as they are, curvatures as 0.5 + k / 20 clipped.  The learned appearance (sdf_trace.SHADING_AOVS, one fused shading kernel on the hit
pixels, surface_shade.py): `--aovs rgb` writes DIR/{k}_rgb.png as RGBA with the hit mask as alpha; the other shading images are RGB or grey
PNGs, 0 where missed.  Only the traced surface is shaded: no background model is evaluated, no human light, and a stage-2 shell is not seen
through.  The learned NeRF++ background (sdf_trace.BACKGROUND_AOVS, one fused kernel on every pixel's ray, background.py): `--aovs frame`
writes DIR/{k}_frame.png (RGB, no alpha: the shaded surface over the background it was trained with) and DIR/{k}_background.png;
`transmittance` is a grey PNG.  --white-background / --no-white-background: what lies behind the background on missed pixels (default: the
config's is_nerf, the reference's color + (1 - acc)).  Prints one JSON line: the output directory, the frame count and the rays hit per frame.
"""
import argparse
import json
import os
import sys

DEFAULT_AOVS = ('depth', 'normal', 'mask')


def parse_args(argv=None):
    from .sdf_trace import ALL_AOVS, BACKGROUND_AOVS
    AOVS = ALL_AOVS + BACKGROUND_AOVS
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.render_surface", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth; 'none': the initialised model)")
    ap.add_argument('--stage2', action='store_true', help="the config is a stage-2 config")
    ap.add_argument('--which', choices=('inner', 'outer'), default=None, help="stage 2: the inner SDF (default) or the stage-1 SDF")
    ap.add_argument('--poses', type=str, default='relight', help="'relight' (the relight command's orbit) or an .npz with 'poses' [n,3,4]")
    ap.add_argument('--hw', type=int, default=800, help="image height = width")
    ap.add_argument('--aovs', type=str, nargs='+', default=list(DEFAULT_AOVS), choices=AOVS, metavar='AOV',
                    help="images to write: " + ' '.join(AOVS))
    ap.add_argument('--num', type=int, default=8, help="frames of the relight orbit")
    ap.add_argument('--azimuth', type=float, default=0.0)
    ap.add_argument('--elevation', type=float, default=45.0)
    ap.add_argument('--cam_dist', type=float, default=3.0)
    ap.add_argument('--max_iter', type=int, default=200)
    ap.add_argument('--threshold', type=float, default=1e-5)
    ap.add_argument('--bound_radius', type=float, default=1.0)
    ap.add_argument('--white-background', dest='white_background', action='store_true', default=None,
                    help="frame: white behind the learned background on missed pixels (default: the config's is_nerf)")
    ap.add_argument('--no-white-background', dest='white_background', action='store_false')
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/surface/{name}-{step})")
    flags = ap.parse_args(argv)
    if flags.which is not None and not flags.stage2:
        ap.error("--which needs --stage2")
    if flags.hw < 1 or flags.num < 1 or flags.max_iter < 1:
        ap.error("--hw, --num and --max_iter must be >= 1")
    if not flags.threshold > 0 or flags.bound_radius < 0:
        ap.error("--threshold must be > 0 and --bound_radius >= 0")
    if flags.poses != 'relight' and not flags.poses.endswith('.npz'):
        ap.error("--poses: 'relight' or a .npz file")
    flags.aovs = tuple(dict.fromkeys(flags.aovs))
    return flags


def which_of(flags):
    if not flags.stage2:
        return 'outer'
    return flags.which or 'inner'


def output_dir(flags, name, step):
    return flags.out or os.path.join('data', 'surface', f'{name}-{step}')


def frame_paths(out, k, aovs):
    """{aov: path} of frame k (+ 'depth.npy' when depth is asked for; 'frame' also writes the background it is composed over)."""
    paths = {a: os.path.join(out, f'{k}_{a}.png') for a in aovs}
    if 'frame' in aovs:
        paths['background'] = os.path.join(out, f'{k}_background.png')
    if 'depth' in aovs:
        paths['depth.npy'] = os.path.join(out, f'{k}_depth.npy')
    return paths


def cameras(flags):
    """(K [3,3], poses [n,3,4]) float64 of the command's cameras."""
    import numpy as np
    from . import relight
    K = relight.intrinsics(flags.hw, flags.hw)
    if flags.poses == 'relight':
        return K, relight.relighting_poses(flags.num, flags.azimuth, flags.elevation, flags.cam_dist)
    with np.load(flags.poses) as z:
        poses = np.asarray(z['poses'], np.float64)
        if 'K' in z.files:
            K = np.asarray(z['K'], np.float64).reshape(3, 3)
    if poses.ndim != 3 or poses.shape[1:] != (3, 4):
        raise SystemExit(f"{flags.poses}: 'poses' must be [n,3,4], got {poses.shape}")
    return K, poses


def to_rgba(aov, img, mask):
    """uint8 [h,w,4] numpy of one AOV (float numpy image, uint8 mask)."""
    import numpy as np
    img = np.asarray(img, np.float32)
    hit = mask > 0
    if aov == 'mask':
        v = np.asarray(mask, np.float32) / 255.0
    elif aov == 'depth':
        lo, hi = (float(img[hit].min()), float(img[hit].max())) if hit.any() else (0.0, 1.0)
        v = (img - lo) / max(hi - lo, 1e-12)
    elif aov in ('normal', 'position'):
        v = 0.5 + 0.5 * img
    elif aov in ('mean_curvature', 'gaussian_curvature'):
        v = 0.5 + img / 20.0
    else:
        v = img
    v = np.clip(np.nan_to_num(v), 0.0, 1.0)
    if v.ndim == 2:
        v = np.repeat(v[:, :, None], 3, 2)
    rgb = (v * 255.0 + 0.5).astype(np.uint8)
    alpha = np.full(mask.shape, 255, np.uint8) if aov == 'mask' else np.where(hit, 255, 0).astype(np.uint8)
    return np.concatenate([np.where(hit[:, :, None] | (aov == 'mask'), rgb, 0).astype(np.uint8), alpha[:, :, None]], 2)


def to_plain(img):
    """uint8 numpy [h,w,3] or [h,w] of a shading AOV already in [0, 1] (0 where missed): what the RGB / grey PNGs hold."""
    import numpy as np
    return (np.clip(np.nan_to_num(np.asarray(img, np.float32)), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    import yaml
    from .extract_mesh import _renderer
    from .relight import write_png
    from .mask_render import _pillow
    from .sdf_trace import BACKGROUND_AOVS, SHADING_AOVS, render_surface
    from .train_glue import load_checkpoint

    with open(flags.cfg) as fh:
        cfg = yaml.safe_load(fh)
    network = _renderer(cfg)
    is_s2 = hasattr(network, 'stage1_network')
    if is_s2 != flags.stage2:
        raise SystemExit(f"config network {cfg['network']!r} is{'' if is_s2 else ' not'} a stage-2 model: "
                         f"{'pass' if is_s2 else 'drop'} --stage2")
    step = 0
    if flags.ckpt != 'none':
        _, step = load_checkpoint(flags.ckpt or f'data/model/{cfg["name"]}/model.pth', network, map_location='cpu')
        if flags.stage2:
            s1_ckpt = network.cfg.get('stage1_ckpt_dir')
            if s1_ckpt and os.path.exists(s1_ckpt):                # as extract_mesh --stage2: stage 1 from its own checkpoint
                load_checkpoint(s1_ckpt, network.stage1_network, map_location='cpu')
    network = network.eval().to(torch.device('cuda', torch.cuda.current_device()))
    out = output_dir(flags, cfg['name'], step)
    os.makedirs(out, exist_ok=True)
    K, poses = cameras(flags)
    want = tuple(dict.fromkeys(flags.aovs + ('mask',) + (('background',) if 'frame' in flags.aovs else ())))
    hits = []
    for k, pose in enumerate(poses):
        imgs = render_surface(network, K, pose, flags.hw, flags.hw, which=which_of(flags), aovs=want, max_iter=flags.max_iter,
                              threshold=flags.threshold, bound_radius=flags.bound_radius, white_background=flags.white_background)
        imgs = {a: v.cpu().numpy() for a, v in imgs.items()}
        paths = frame_paths(out, k, flags.aovs)
        for a in (p for p in paths if p != 'depth.npy'):
            if a in BACKGROUND_AOVS or (a in SHADING_AOVS and a != 'rgb'):
                _pillow().fromarray(to_plain(imgs[a])).save(paths[a])
            else:
                write_png(paths[a], to_rgba(a, imgs[a], imgs['mask']))
        if 'depth' in flags.aovs:
            np.save(paths['depth.npy'], np.ascontiguousarray(imgs['depth'], np.float32))
        hits.append(int((imgs['mask'] > 0).sum()))
    print(json.dumps({'name': cfg['name'], 'step': int(step), 'out': out, 'frames': len(poses), 'hw': flags.hw, 'aovs': list(flags.aovs),
                      'hit': hits}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
