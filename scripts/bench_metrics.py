"""Report aid: PSNR + SSIM (win 11) of an 8 x 800 x 800 x 3 uint8 batch.

  python scripts/bench_metrics.py device    nu_nerf_amd.metrics.psnr + ssim on the GPU: ms per batch, GPU events, median of the repeats
  python scripts/bench_metrics.py host      the scipy oracle of tests/metrics_oracle.py (ssim_filter + the float32 compute_psnr) on the
                                            host, image by image as the reference's metric classes do; wall time, thread count reported
One JSON line each; the host line carries the device's values when given the device's JSON line as a third argument."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

N, H, W, REPS = 8, 800, 800, 7


def batch():
    g = np.random.Generator(np.random.PCG64(800))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([127 + 100 * np.sin(xx / 37) * np.cos(yy / 23), 40 + 0.25 * xx, 255 - 0.3 * yy], -1)[None] + g.normal(0, 10, (N, 1, 1, 3))
    a = np.clip(base, 0, 255).astype(np.uint8)
    return a, np.clip(base + g.normal(0, 6.0, base.shape), 0, 255).astype(np.uint8)


def device():
    import torch
    from nu_nerf_amd.metrics import psnr, ssim
    dev = torch.device('cuda:0')
    a, b = (torch.from_numpy(x).to(dev) for x in batch())
    ms = {'psnr': [], 'ssim': []}
    for i in range(REPS + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        p = psnr(a, b)
        ev[1].record()
        s = ssim(a, b, win_size=11)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 2:
            ms['psnr'].append(ev[0].elapsed_time(ev[1]))
            ms['ssim'].append(ev[1].elapsed_time(ev[2]))
    print(json.dumps({'where': 'device', 'n': N, 'h': H, 'w': W, 'psnr_ms': float(np.median(ms['psnr'])), 'ssim_ms': float(np.median(ms['ssim'])),
                      'psnr': p.tolist(), 'ssim': s.tolist()}))


def host(device_line=None):
    import metrics_oracle as O
    a, b = batch()
    t0 = time.perf_counter()
    p = [float(O.compute_psnr_f32(a[i], b[i])) for i in range(N)]
    t1 = time.perf_counter()
    s = [O.ssim_filter(a[i], b[i], 11)[0] for i in range(N)]
    t2 = time.perf_counter()
    res = {'where': 'host', 'n': N, 'h': H, 'w': W, 'psnr_ms': 1e3 * (t1 - t0), 'ssim_ms': 1e3 * (t2 - t1),
           'threads': os.environ.get('OMP_NUM_THREADS'), 'psnr': p, 'ssim': s}
    if device_line:
        d = json.loads(device_line)
        res['max_abs_ssim_difference'] = float(np.abs(np.array(d['ssim']) - np.array(s)).max())
        res['max_abs_psnr_difference_db'] = float(np.abs(np.array(d['psnr']) - np.array(p)).max())
    print(json.dumps(res))


if __name__ == '__main__':
    device() if sys.argv[1] == 'device' else host(sys.argv[2] if len(sys.argv) > 2 else None)
