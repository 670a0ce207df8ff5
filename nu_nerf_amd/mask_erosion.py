"""python -m nu_nerf_amd.mask_erosion --cfg CFG [--erosion 15]
   python -m nu_nerf_amd.mask_erosion --mask-dir DIR --out-dir DIR [--erosion 15]

mask_erosion.py on the GPU: every file of <dataset_dir>/<object>/mask (channel 0, what get_mask reads) is eroded with an
erosion x erosion box and composed with its inverted self (mask_render.erode_masks, nu_mask_erode) and written under the same file
name to <dataset_dir>/<object>/mask_erosion.  --mask-dir / --out-dir name the two directories directly.  Images are read and
written through Pillow (JPEG at quality 95, three equal channels).
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.mask_erosion", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, default=None, help="stage-2 training config (YAML)")
    ap.add_argument('--erosion', type=int, default=15, help="box size in pixels (default 15)")
    ap.add_argument('--mask-dir', type=str, default=None, help="input masks (instead of --cfg)")
    ap.add_argument('--out-dir', type=str, default=None, help="output directory (with --mask-dir)")
    ap.add_argument('--chunk', type=int, default=16, help="images per launch (default 16)")
    flags = ap.parse_args(argv)
    if (flags.cfg is None) == (flags.mask_dir is None):
        ap.error("give exactly one of --cfg and --mask-dir")
    if flags.mask_dir is not None and flags.out_dir is None:
        ap.error("--mask-dir needs --out-dir")
    if flags.erosion < 1:
        ap.error("--erosion must be >= 1")
    return flags


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    from .mask_render import erode_masks, object_dir, read_mask_image, write_mask_image, _pillow

    _pillow()
    if flags.cfg is not None:
        import yaml
        with open(flags.cfg) as fh:
            cfg = yaml.safe_load(fh)
        src, dst = os.path.join(object_dir(cfg), 'mask'), os.path.join(object_dir(cfg), 'mask_erosion')
    else:
        src, dst = flags.mask_dir, flags.out_dir
    os.makedirs(dst, exist_ok=True)
    names = sorted(f for f in os.listdir(src) if os.path.isfile(os.path.join(src, f)))
    dev = torch.device('cuda', torch.cuda.current_device())
    chunk = max(1, int(flags.chunk))
    group, paths = [], []

    def flush():
        m = torch.from_numpy(np.stack([a for _, a in group], 0)).to(dev)
        out = erode_masks(m, flags.erosion).cpu().numpy()
        for (name, _), o in zip(group, out):
            paths.append(write_mask_image(os.path.join(dst, name), o))
        group.clear()

    for name in names:                   # consecutive images of one size go to the GPU together
        a = read_mask_image(os.path.join(src, name))
        if group and (a.shape != group[0][1].shape or len(group) == chunk):
            flush()
        group.append((name, a))
    if group:
        flush()
    print(f'wrote {len(paths)} eroded masks to {dst}')
    return paths


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
