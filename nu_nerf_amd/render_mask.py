"""python -m nu_nerf_amd.render_mask --cfg CFG --mesh_path PLY
   python -m nu_nerf_amd.render_mask --cameras NPZ --mesh_path PLY --out DIR

render_mask.py on the GPU: every training image's object mask against the stage-1 mesh, 255 where the pixel's ray hits it.
--cfg dispatches on `is_nerf` like the reference: NeRF-synthetic data -> mask_render.render_masks (render_mask_synthetic.py),
real captures -> mask_render.render_masks_real (render_mask_real.py, any-hit LBVH trace per pixel); the train split comes from
the user's NU-NeRF checkout (dataset/database_formask.py, dataset/database.py) and the masks go to
<dataset_dir>/<object>/mask/<stem>.jpg.  --cameras needs no checkout: an NPZ with Ks [n,3,3] (or [3,3]), poses [n,3,4]
(world -> camera; camera -> world when it also holds is_nerf=True), names [n], h, w; the masks go to DIR/<stem>.jpg.
JPEG at quality 95, three equal channels, through Pillow.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.render_mask", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, default=None, help="stage-2 training config (YAML)")
    ap.add_argument('--mesh_path', type=str, required=True, help="stage-1 mesh (PLY)")
    ap.add_argument('--cameras', type=str, default=None, help="NPZ with Ks, poses, names, h, w (instead of --cfg)")
    ap.add_argument('--out', type=str, default=None, help="output directory of the --cameras mode")
    ap.add_argument('--chunk', type=int, default=16, help="images per launch (default 16)")
    flags = ap.parse_args(argv)
    if (flags.cfg is None) == (flags.cameras is None):
        ap.error("give exactly one of --cfg and --cameras")
    if flags.cameras is not None and flags.out is None:
        ap.error("--cameras needs --out")
    return flags


def _cameras_from_cfg(cfg):
    import numpy as np
    from .mask_render import load_database_split, object_dir
    is_nerf = bool(cfg['is_nerf'])
    database, ids = load_database_split(cfg, 'database' if is_nerf else 'database_formask')
    h, w = database.get_image(ids[0]).shape[:2]
    Ks = np.stack([database.get_K(i) for i in ids], 0).astype(np.float32)
    poses = np.stack([database.get_pose(i) for i in ids], 0).astype(np.float32)
    names = [database.image_names[int(i) if is_nerf else i] for i in ids]
    return Ks, poses, names, int(h), int(w), is_nerf, os.path.join(object_dir(cfg), 'mask')


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    from . import mesh
    from .lbvh import LBVH
    from .mask_render import render_masks, render_masks_real, write_mask_jpegs, _pillow

    _pillow()                                                  # fail before any work when Pillow is missing
    if flags.cfg is not None:
        import yaml
        with open(flags.cfg) as fh:
            cfg = yaml.safe_load(fh)
        Ks, poses, names, h, w, is_nerf, out_dir = _cameras_from_cfg(cfg)
    else:
        z = np.load(flags.cameras, allow_pickle=False)
        Ks, poses, names = z['Ks'], z['poses'], [str(s) for s in z['names']]
        h, w, is_nerf, out_dir = int(z['h']), int(z['w']), bool(z['is_nerf']) if 'is_nerf' in z else False, flags.out
    dev = torch.device('cuda', torch.cuda.current_device())
    V, F = mesh.read_ply(flags.mesh_path)
    V, F = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    bvh = LBVH(V, F)
    n, chunk = len(names), max(1, int(flags.chunk))
    paths = []
    for i in range(0, n, chunk):
        sl = slice(i, min(i + chunk, n))
        if is_nerf:
            m = render_masks(V, F, Ks, poses[sl], h, w, bvh=bvh)
        else:
            m = render_masks_real(V, F, Ks if np.ndim(Ks) == 2 else Ks[sl], poses[sl], h, w, bvh=bvh)
        paths += write_mask_jpegs(m, out_dir, names[sl])
    print(f'wrote {len(paths)} masks to {out_dir}')
    return paths


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
