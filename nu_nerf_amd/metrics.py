"""python -m nu_nerf_amd.metrics PR GT [--win-size 11]

PSNR and SSIM of rendered images against ground truth, on the GPU (csrc/metrics.hip): PR and GT are two image files, or two
directories whose files are matched by stem.  Prints one JSON line: images (name, psnr, ssim per pair), psnr and ssim (their
means), win_size and count.  Identical images have psnr Infinity, as numpy gives.

As a module it is network/metrics.py of the reference without skimage and cv2:

  to_uint8, psnr, ssim               device tensors in, device tensors out, nothing read back
  compute_psnr                       the reference's function (one number on the host)
  ShapeRenderMetrics, Stage2RenderMetrics, name2metrics, name2key_metrics
                                     what train/trainer*.py and train/train_valid.py look up
  panel                              the validation picture the metric classes save, without the text labels

SSIM is skimage.metrics.structural_similarity(gt, pr, win_size=11, channel_axis=2, data_range=255) on the uint8 images; its window
sums are exact integers on the device and its result is the same bits on every run.  'mat_render' is not in
name2metrics: MaterialRenderMetrics belongs to the material-estimation stage of NeRO, which NU-NeRF does not have.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

from . import _lib as L


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def to_uint8(x):
    """color_map_backward on the device: uint8 of clamp(x * 255, 0, 255), truncated; the shape of x."""
    L.require_cuda(x)
    x = x.detach().to(torch.float32).contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.load().nu_img_quantize(L.ptr(x), x.numel(), L.ptr(out), L.stream())
    return out


def _pair(gt, pr, what):
    """Both images as contiguous [n, h, w, c] uint8 on the device."""
    L.require_cuda(gt, pr)
    if gt.dtype != torch.uint8 or pr.dtype != torch.uint8 or gt.shape != pr.shape or gt.dim() not in (3, 4):
        raise ValueError(f"{what}: two uint8 tensors of one shape [h,w,c] or [n,h,w,c] are needed, got {gt.dtype} {tuple(gt.shape)} "
                         f"and {pr.dtype} {tuple(pr.shape)}")
    if gt.shape[-1] not in (1, 3):
        raise ValueError(f"{what}: images have 1 or 3 channels, got {gt.shape[-1]}")
    if gt.dim() == 3:
        gt, pr = gt[None], pr[None]
    return gt.contiguous(), pr.contiguous()


def sqdiff(gt_u8, pr_u8):
    """int64 [n]: the sum of squared differences of each image pair, exactly."""
    gt, pr = _pair(gt_u8, pr_u8, "sqdiff")
    n = gt.shape[0]
    ssd = torch.empty(n, dtype=torch.int64, device=gt.device)
    L.load().nu_img_sqdiff(L.ptr(gt), L.ptr(pr), n, gt[0].numel() if n else 0, L.ptr(ssd), L.stream())
    return ssd


def psnr(gt_u8, pr_u8):
    """float64 [n] on the device: 10 log10(255^2 count / ssd) from the exact ssd; +inf where the images are equal."""
    ssd = sqdiff(gt_u8, pr_u8)
    count = gt_u8[0].numel() if gt_u8.dim() == 4 else gt_u8.numel()
    return 10.0 * torch.log10((255.0 * 255.0 * count) / ssd.to(torch.float64))


def ssim(gt_u8, pr_u8, win_size=11, full=False):
    """float64 [n] on the device: the mean structural similarity of each pair over a uniform win_size x win_size window.
    full=True also returns the map [n, h - win_size + 1, w - win_size + 1, c] over the windows inside the image (what skimage's
    full=True map is after the crop its mean uses)."""
    gt, pr = _pair(gt_u8, pr_u8, "ssim")
    n, h, w, c = (int(s) for s in gt.shape)
    win = int(win_size)
    if win % 2 == 0 or win < 3 or win > 15:
        raise ValueError(f"ssim: win_size must be odd and in [3, 15], got {win_size}")
    if h < win or w < win:
        raise ValueError(f"ssim: win_size {win} exceeds the image ({h} x {w})")
    lib = L.load()
    mssim = torch.empty(n, dtype=torch.float64, device=gt.device)
    smap = torch.empty(n, h - win + 1, w - win + 1, c, dtype=torch.float64, device=gt.device) if full else None
    nbytes = lib.nu_img_ssim_workspace_bytes(n, h, w, c)
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=gt.device)
    lib.nu_img_ssim(L.ptr(gt), L.ptr(pr), n, h, w, c, win, L.ptr(mssim), L.ptr(smap), L.ptr(work), nbytes, L.stream())
    return (mssim, smap) if full else mssim


def _to_device_u8(img):
    t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8:
        raise ValueError(f"uint8 images are needed, got {t.dtype}")
    return t if t.is_cuda else t.to(_device())


def compute_psnr(img_gt, img_pr):
    """The reference's compute_psnr(img_gt, img_pr) for uint8 images (arrays or tensors, any shape): one number on the host.  The
    reference averages in float32; this is the exact value."""
    gt, pr = _to_device_u8(img_gt).reshape(1, 1, -1, 1), _to_device_u8(img_pr).reshape(1, 1, -1, 1)
    return np.float64(psnr(gt, pr).item())


_SHAPE_KEYS = ['diffuse_albedo', 'diffuse_light', 'diffuse_color', 'refraction_light',
               'specular_albedo', 'specular_light', 'specular_color', 'specular_ref',
               'transmission_weight', 'roughness', 'occ_prob', 'indirect_light']
_STAGE2_KEYS = ['specular_light', 'specular_color', 'specular_ref']


def panel(data_pr, stage2=False):
    """uint8 [H, W, 3] on the device: the picture the reference's metric classes save.  Row 1 is gt_rgb | ray_rgb | normal; below
    it the maps of draw_materials (those of the 12 keys that data_pr has, four per row) or, for stage 2, of draw_materials_s2
    (three, one row); one-channel maps are repeated to three.  Rows narrower than the widest are padded with zeros on the right
    (concat_images_list, utils/draw_utils.py:172-192).  The text labels cv2.putText draws on the material maps are not reproduced.
    With shader_config.human_light the outputs carry `human_light`: it is appended to row 1 (network/metrics.py:118-119)."""
    pr = to_uint8(data_pr['ray_rgb'])
    h, w = int(pr.shape[0]), int(pr.shape[1])

    def image(k):
        img = to_uint8(data_pr[k]).reshape(h, w, -1)
        return img.expand(h, w, 3) if img.shape[-1] == 1 else img

    keys = [k for k in (_STAGE2_KEYS if stage2 else _SHAPE_KEYS) if k in data_pr]
    rows = [['gt_rgb', 'ray_rgb', 'normal'] + (['human_light'] if 'human_light' in data_pr else [])]
    rows += [keys[i:i + 4] for i in range(0, len(keys), 4)]
    out = torch.zeros(h * len(rows), w * max(len(r) for r in rows), 3, dtype=torch.uint8, device=pr.device)
    for ri, row in enumerate(rows):
        for ci, k in enumerate(row):
            out[ri * h:(ri + 1) * h, ci * w:(ci + 1) * w] = pr if k == 'ray_rgb' else image(k)
    return out


_warned_no_pillow = False


def save_panel(img, path):
    """Write the panel as a JPEG of quality 95 through Pillow; without Pillow: one warning, no file.  Returns the path or None."""
    global _warned_no_pillow
    try:
        from PIL import Image
    except ImportError:
        if not _warned_no_pillow:
            warnings.warn("Pillow is not installed: the validation pictures under data/train_vis are not written")
            _warned_no_pillow = True
        return None
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(img.cpu().numpy()).save(path, quality=95)
    return path


class ShapeRenderMetrics:
    """metric(data_pr, data_gt, step, data_index=i, model_name=name) -> {'psnr': ndarray [1], 'ssim': ndarray [1]} of
    data_pr['ray_rgb'] against data_pr['gt_rgb'] ([h, w, 3] floats in [0, 1]), and data/train_vis/<name>/<step>-index-<i>.jpg.
    Both metrics are queued before the one host read that fetches the two numbers."""
    stage2 = False

    def __init__(self, cfg=None):
        pass

    def __call__(self, data_pr, data_gt, step, **kwargs):
        gt, pr = to_uint8(data_pr['gt_rgb']), to_uint8(data_pr['ray_rgb'])
        both = torch.cat([psnr(gt, pr), ssim(gt, pr, win_size=11)]).cpu().numpy()
        save_panel(panel(data_pr, self.stage2),
                   os.path.join('data', 'train_vis', str(kwargs['model_name']), f"{step}-index-{kwargs['data_index']}.jpg"))
        return {'psnr': both[0:1], 'ssim': both[1:2]}


class Stage2RenderMetrics(ShapeRenderMetrics):
    stage2 = True


name2metrics = {
    'shape_render': ShapeRenderMetrics,
    'stage2': Stage2RenderMetrics,
}


def _mean_psnr(results):
    return np.mean(results['psnr'])


name2key_metrics = {
    'psnr': _mean_psnr,
}


def read_image(path):
    """uint8 [h, w, 1] for a greyscale file, [h, w, 3] for anything else (converted to RGB)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("reading image files needs Pillow (pip install pillow); cv2 is not used") from e
    with Image.open(path) as im:
        a = np.asarray(im if im.mode == 'L' else im.convert('RGB'))
    return np.array(a.reshape(a.shape[0], a.shape[1], -1))          # a writable copy: Pillow's buffer is read-only


def match_files(pr, gt):
    """[(name, pr_path, gt_path)]: the two files, or the files of the two directories that share a stem, sorted by stem."""
    if os.path.isdir(pr) != os.path.isdir(gt):
        raise ValueError("PR and GT must be two files or two directories")
    if not os.path.isdir(pr):
        return [(os.path.splitext(os.path.basename(pr))[0], pr, gt)]

    def stems(d):
        return {os.path.splitext(f)[0]: os.path.join(d, f) for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}
    a, b = stems(pr), stems(gt)
    return [(s, a[s], b[s]) for s in sorted(set(a) & set(b))]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.metrics", description=__doc__.split("\n\n")[1])
    ap.add_argument('pr', type=str, help="rendered image, or a directory of them")
    ap.add_argument('gt', type=str, help="ground-truth image, or a directory matched by file stem")
    ap.add_argument('--win-size', type=int, default=11, help="SSIM window (odd, 3..15; default 11)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    pairs = match_files(args.pr, args.gt)
    if not pairs:
        raise SystemExit(f"no file stem is in both {args.pr} and {args.gt}")
    dev = _device()
    images, queued = [], []
    for name, p, g in pairs:                # every pair is queued before the first number is read
        a, b = torch.from_numpy(read_image(p)).to(dev), torch.from_numpy(read_image(g)).to(dev)
        if a.shape != b.shape:
            raise SystemExit(f"{name}: {p} is {tuple(a.shape)}, {g} is {tuple(b.shape)}")
        queued.append(torch.cat([psnr(b, a), ssim(b, a, win_size=args.win_size)]))
    for (name, _, _), v in zip(pairs, torch.stack(queued).cpu().tolist()):
        images.append({'name': name, 'psnr': v[0], 'ssim': v[1]})
    res = {'images': images, 'psnr': float(np.mean([i['psnr'] for i in images])), 'ssim': float(np.mean([i['ssim'] for i in images])),
           'win_size': args.win_size, 'count': len(images)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
