"""numpy statements of the validation metrics (network/metrics.py of the reference), independent of nu_nerf_amd.

  to_uint8            color_map_backward: x * 255 in float32, clip to [0, 255], cast to uint8
  ssd_exact           the sum of squared differences as a Python int
  psnr_exact          10 log10(255^2 count / ssd) in float64 from the exact ssd (inf for equal images)
  compute_psnr_f32    the reference's compute_psnr: float32 means over pixels, then over the three channels
  ssim_filter         skimage.metrics.structural_similarity(a, b, win_size=win, channel_axis=2, data_range=255), restated in float64
                      with scipy.ndimage.uniform_filter (needs scipy)
  ssim_exact          the same quantity from exact integer window sums: what the device kernel evaluates, operation for operation

Images are uint8 [h, w, c].  Both SSIM functions return (mssim, S) with S the map over the windows that lie inside the image,
[h - win + 1, w - win + 1, c]: skimage takes its mean over exactly those."""
import numpy as np

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def to_uint8(x):
    with np.errstate(over='ignore'):               # a huge value becomes inf, which clips to 255
        x = np.asarray(x, np.float32) * 255
    return np.clip(x, 0, 255).astype(np.uint8)


def ssd_exact(a, b):
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def psnr_exact(a, b):
    ssd = ssd_exact(a, b)
    return float('inf') if ssd == 0 else float(10.0 * np.log10(np.float64(255.0 * 255.0 * np.asarray(a).size) / np.float64(ssd)))


def compute_psnr_f32(img_gt, img_pr):
    gt = np.asarray(img_gt).reshape(-1, 3).astype(np.float32)
    pr = np.asarray(img_pr).reshape(-1, 3).astype(np.float32)
    with np.errstate(divide='ignore'):
        return 10 * np.log10(255 * 255 / np.mean(np.mean((gt - pr) ** 2, 0)))


def _ssim_from_moments(ux, uy, vx, vy, vxy):
    a1, a2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
    b1, b2 = ux * ux + uy * uy + C1, vx + vy + C2
    return (a1 * a2) / (b1 * b2)


def ssim_filter(a, b, win=11):
    from scipy.ndimage import uniform_filter
    a, b = np.asarray(a), np.asarray(b)
    npix = win * win
    cov_norm = npix / (npix - 1.0)
    pad = (win - 1) // 2
    maps = []
    for ch in range(a.shape[2]):
        x, y = a[..., ch].astype(np.float64), b[..., ch].astype(np.float64)
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        s = _ssim_from_moments(ux, uy, cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy))
        maps.append(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad])
    smap = np.stack(maps, -1)
    return float(np.mean([m.mean() for m in maps])), smap


def window_sums(v, win):
    """int64 [h - win + 1, w - win + 1, c]: the sum of v over every win x win window, exactly."""
    from numpy.lib.stride_tricks import sliding_window_view
    v = np.asarray(v, np.int64)
    rows = sliding_window_view(v, win, axis=1).sum(-1)
    return sliding_window_view(rows, win, axis=0).sum(-1)


def ssim_exact(a, b, win=11):
    x, y = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    npix = win * win
    sx, sy = window_sums(x, win), window_sums(y, win)
    sxx, syy, sxy = window_sums(x * x, win), window_sums(y * y, win), window_sums(x * y, win)
    assert max(int(sxx.max()), int(syy.max()), int(sxy.max())) < 2 ** 24 or win > 15
    den = float(npix) * float(npix - 1)
    ux, uy = sx / float(npix), sy / float(npix)
    vx, vy, vxy = (npix * sxx - sx * sx) / den, (npix * syy - sy * sy) / den, (npix * sxy - sx * sy) / den
    smap = _ssim_from_moments(ux, uy, vx, vy, vxy)
    return float(smap.mean()), smap
