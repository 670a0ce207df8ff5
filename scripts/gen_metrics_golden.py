"""Writes tests/golden/metrics_skimage.npz: image pairs and what scikit-image itself says about them.

Run once, under an interpreter that has scikit-image (written against 0.18.3, which spells channel_axis=2 as multichannel=True):

    python scripts/gen_metrics_golden.py

The test suite needs neither this script nor scikit-image, only the .npz.  Per case NAME the file holds NAME_a, NAME_b (uint8
[h, w, c]), NAME_win, NAME_mssim (float64, structural_similarity(a, b, win_size=win, channel_axis=2, data_range=255)) and, for
the cases in FULL, NAME_smap: the full=True map cropped to the windows that lie inside the image, [h - win + 1, w - win + 1, c].
`cases` lists the names.  Inputs come from the seed below."""
import os

import numpy as np
import skimage
from skimage.metrics import structural_similarity

SEED = 20260
FULL = ('odd_37x23',)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'metrics_skimage.npz')


def cases():
    g = np.random.Generator(np.random.PCG64(SEED))
    u8 = lambda x: np.clip(np.rint(x), 0, 255).astype(np.uint8)
    out = {}
    out['noise_64x80'] = (g.integers(0, 256, (64, 80, 3)).astype(np.uint8), g.integers(0, 256, (64, 80, 3)).astype(np.uint8), 11)
    yy, xx = np.mgrid[0:96, 0:128]
    smooth = np.stack([127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 40 + 1.5 * xx, 255 - 2.0 * yy], -1)
    out['smooth_96x128'] = (u8(smooth), u8(smooth + g.normal(0, 6.0, smooth.shape)), 11)
    same = g.integers(0, 256, (32, 40, 3)).astype(np.uint8)
    out['identical_32x40'] = (same, same.copy(), 11)
    # 16-pixel bands of 0 and 255 against white: windows inside a white band carry the largest sums there are (121 * 255^2)
    stripes = np.where((np.arange(64) // 16) % 2 == 0, 255, 0).astype(np.uint8)
    out['saturated_48x64'] = (np.broadcast_to(stripes[None, :, None], (48, 64, 3)).copy(), np.full((48, 64, 3), 255, np.uint8), 11)
    out['single_11x11'] = (g.integers(0, 256, (11, 11, 3)).astype(np.uint8), g.integers(0, 256, (11, 11, 3)).astype(np.uint8), 11)
    base = g.integers(0, 256, (37, 23, 3))
    out['odd_37x23'] = (u8(base), u8(base + g.normal(0, 20.0, base.shape)), 11)
    out['dark_40x40'] = (g.integers(0, 6, (40, 40, 3)).astype(np.uint8), g.integers(0, 6, (40, 40, 3)).astype(np.uint8), 11)
    base = g.integers(0, 256, (45, 50, 3))
    out['win7_45x50'] = (u8(base), u8(base + g.normal(0, 35.0, base.shape)), 7)
    base = g.integers(0, 256, (33, 29, 1))
    out['gray_33x29'] = (u8(base), u8(base + g.normal(0, 25.0, base.shape)), 11)
    return out


def main():
    rec = {'skimage_version': np.array(skimage.__version__)}
    names = []
    for name, (a, b, win) in cases().items():
        gray = a.shape[2] == 1
        args = (a[..., 0], b[..., 0]) if gray else (a, b)
        mssim, smap = structural_similarity(*args, win_size=win, multichannel=not gray, data_range=255, full=True)
        pad = (win - 1) // 2
        smap = smap.reshape(a.shape)[pad:a.shape[0] - pad, pad:a.shape[1] - pad]
        rec[name + '_a'], rec[name + '_b'], rec[name + '_win'] = a, b, np.array(win)
        rec[name + '_mssim'] = np.array(mssim, np.float64)
        if name in FULL:
            rec[name + '_smap'] = np.ascontiguousarray(smap, np.float64)
        names.append(name)
        print(f'{name:18s} win {win:2d}  mssim {float(mssim)!r}')
    rec['cases'] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print('wrote', os.path.normpath(OUT), os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
