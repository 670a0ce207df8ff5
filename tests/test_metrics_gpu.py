"""Device PSNR / SSIM (csrc/metrics.hip, nu_nerf_amd/metrics.py) against the numpy oracles of tests/metrics_oracle.py and against what
scikit-image returned for the fixture pairs (tests/golden/metrics_skimage.npz).

Bounds.  Against the exact-integer oracle the device evaluates the same formula on the same integers; only the order of the sum
behind the mean differs, so every map value must lie within 16 ulp (fp64) and the mean within 1e-12.  Against skimage the bound
is 10 x the largest |exact-integer oracle - skimage| measured on the CPU over the fixture (2.665e-15, skimage's own float64
rounding).  PSNR: the device value is exact; the reference's float32 compute_psnr is off by up to 1.365e-4 dB on the fixture pairs
(measured on the CPU against int64), and the device is held to 10 x that against it.  tests/test_metrics_host.py re-measures both."""
import os

import numpy as np
import pytest
import torch

import metrics_oracle as O
from helpers import golden

pytestmark = pytest.mark.gpu

EXACT_VS_SKIMAGE = 2.665e-15
PSNR_F32_ERR_DB = 1.365e-4


def cases():
    g = golden("metrics_skimage.npz")
    return g, [str(n) for n in g['cases']]


def dev_pair(gpu, a, b):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu), torch.from_numpy(np.ascontiguousarray(b)).to(gpu)


def within_ulps(x, ref, ulps):
    return bool(np.all(np.abs(x - ref) <= ulps * np.spacing(np.abs(ref))))


_pairs = {}


def random_pair(n, h, w, c):
    """n image pairs, the second a noisy copy of the first; the first n of the same eight for every n."""
    if (h, w, c) not in _pairs:
        g = np.random.Generator(np.random.PCG64(h * 1000 + w * 10 + c))
        a = g.integers(0, 256, (8, h, w, c)).astype(np.uint8)
        smooth = (a.astype(np.float32) + np.roll(a, 1, 1) + np.roll(a, 1, 2) + np.roll(a, 2, 1)) / 4
        b = np.clip(smooth + g.normal(0, 12.0, a.shape), 0, 255).astype(np.uint8)
        _pairs[(h, w, c)] = (smooth.astype(np.uint8), b)
    a, b = _pairs[(h, w, c)]
    return a[:n], b[:n]


def test_quantize_is_numpy_byte_for_byte(gpu):
    from nu_nerf_amd.metrics import to_uint8
    g = np.random.Generator(np.random.PCG64(11))
    k = np.arange(256, dtype=np.float32)
    exact = (k / np.float32(255)).astype(np.float32)                 # the exact multiples of 1/255 as float32 has them ...
    special = np.concatenate([exact, np.nextafter(exact, np.float32(2)), np.nextafter(exact, np.float32(-1)),      # ... and their neighbours
                              np.array([0.0, -0.0, 1.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3e38, -3e38,
                                        255.0, 1.0039216, 0.99999994], np.float32)]).astype(np.float32)
    body = np.concatenate([g.normal(0.5, 1.0, 600_000), g.uniform(0, 1, 1_000_000 - 600_000 - special.size)]).astype(np.float32)
    x = np.concatenate([special, body])
    assert x.size == 1_000_000 and (x < 0).any() and (x > 1).any()
    want = O.to_uint8(x)
    xd = torch.from_numpy(x).to(gpu)
    assert np.array_equal(to_uint8(xd).cpu().numpy(), want)
    assert np.array_equal(to_uint8(xd[1:]).cpu().numpy(), want[1:])                     # an unaligned start, a ragged end
    assert np.array_equal(to_uint8(xd[:1001].reshape(7, 11, 13)).cpu().numpy(), want[:1001].reshape(7, 11, 13))
    assert to_uint8(torch.tensor([float('nan'), 0.5], device=gpu)).tolist() == [0, 127]  # NaN -> 0 by definition here
    assert to_uint8(torch.empty(0, 3, device=gpu)).shape == (0, 3)


def test_sqdiff_equals_int64_numpy_as_integers(gpu):
    from nu_nerf_amd.metrics import sqdiff
    g, names = cases()
    for n in names:
        a, b = dev_pair(gpu, g[n + '_a'], g[n + '_b'])
        got = sqdiff(a, b)
        assert got.dtype == torch.int64 and got.tolist() == [O.ssd_exact(g[n + '_a'], g[n + '_b'])], n
    a, b = random_pair(8, 800, 800, 3)
    ad, bd = dev_pair(gpu, a, b)
    want = [O.ssd_exact(a[i], b[i]) for i in range(8)]
    assert sqdiff(ad, bd).tolist() == want
    # images that start at odd addresses: 37 * 23 * 3 bytes each, and a batch sliced off its first image
    a, b = random_pair(8, 37, 23, 3)
    ad, bd = dev_pair(gpu, a, b)
    assert sqdiff(ad[1:], bd[3:4].expand(7, 37, 23, 3)).tolist() == [O.ssd_exact(a[i], b[3]) for i in range(1, 8)]


def test_ssim_map_and_mean_against_the_exact_integer_oracle_and_skimage(gpu):
    from nu_nerf_amd.metrics import ssim
    g, names = cases()
    for n in names:
        a, b, win = g[n + '_a'], g[n + '_b'], int(g[n + '_win'])
        ad, bd = dev_pair(gpu, a, b)
        m, smap = ssim(ad, bd, win_size=win, full=True)
        assert m.dtype == torch.float64 and m.shape == (1,) and m.is_cuda
        want_m, want_map = O.ssim_exact(a, b, win)
        got_m, got_map = float(m[0]), smap[0].cpu().numpy()
        assert got_map.shape == want_map.shape, n
        err_ulp = float((np.abs(got_map - want_map) / np.spacing(np.abs(want_map))).max())
        print(f"{n:18s} map: {err_ulp:.1f} ulp   mean - exact: {got_m - want_m:+.3e}   mean - skimage: {got_m - float(g[n + '_mssim']):+.3e}")
        assert within_ulps(got_map, want_map, 16), n
        assert abs(got_m - want_m) <= 1e-12, n
        assert abs(got_m - float(g[n + '_mssim'])) <= 10 * EXACT_VS_SKIMAGE, n
        assert float(ssim(ad, bd, win_size=win)[0]) == got_m                              # with and without the map: the same mean
        if n + '_smap' in g:
            assert np.abs(got_map - g[n + '_smap']).max() < 1e-12
    a, b = dev_pair(gpu, g['identical_32x40_a'], g['identical_32x40_b'])
    assert float(ssim(a, b)[0]) == 1.0


def test_psnr_against_exact_and_float32_restatement(gpu):
    from nu_nerf_amd.metrics import psnr, compute_psnr
    g, names = cases()
    for n in names:
        a, b = g[n + '_a'], g[n + '_b']
        got = psnr(*dev_pair(gpu, a, b))
        assert got.dtype == torch.float64 and got.is_cuda and got.shape == (1,)
        got, exact = float(got[0]), O.psnr_exact(a, b)
        if O.ssd_exact(a, b) == 0:
            assert got == float('inf') and compute_psnr(a, b) == float('inf')
            continue
        assert abs(got - exact) <= 1e-12 * abs(exact), n                  # one fp64 division and log10 on either side
        assert float(compute_psnr(a, b)) == got, n                        # any shape, arrays or tensors
        if a.shape[2] == 3:
            f32 = float(O.compute_psnr_f32(a, b))
            print(f"{n:18s} psnr {got:.9f} dB   float32 restatement {f32:.9f} dB   difference {got - f32:+.3e}")
            assert abs(got - f32) <= 10 * PSNR_F32_ERR_DB, n


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [(11, 11), (37, 23), (64, 80), (800, 800)])
def test_ssim_shapes_and_batched_equals_per_image_bit_for_bit(gpu, hw, c):
    from nu_nerf_amd.metrics import ssim, psnr
    h, w = hw
    a, b = random_pair(8, h, w, c)
    ad, bd = dev_pair(gpu, a, b)
    for win in (7, 11):
        single = torch.cat([ssim(ad[i], bd[i], win_size=win) for i in range(8)])          # [h, w, c] inputs
        for n in (1, 3, 8):
            got = ssim(ad[:n], bd[:n], win_size=win)
            assert got.shape == (n,) and torch.equal(got, single[:n]), (n, win)
        assert torch.equal(ssim(ad[5:], bd[5:], win_size=win), single[5:])                # a batch that starts mid-buffer
        for i in (0, 7):
            want, _ = O.ssim_exact(a[i], b[i], win)
            assert abs(float(single[i]) - want) <= 1e-12, (i, win)
    m, smap = ssim(ad[:3], bd[:3], win_size=11, full=True)
    if h * w <= 64 * 80:
        for i in range(3):
            assert within_ulps(smap[i].cpu().numpy(), O.ssim_exact(a[i], b[i], 11)[1], 16)
    else:                                                                                 # the far corner of the large map, every tile remainder
        want = O.ssim_exact(a[2][-40:, -90:], b[2][-40:, -90:], 11)[1]
        assert within_ulps(smap[2, -30:, -80:].cpu().numpy(), want, 16)
    p = psnr(ad, bd)
    assert torch.equal(p[:3], psnr(ad[:3], bd[:3])) and torch.equal(p[4:5], psnr(ad[4], bd[4]))


def test_ssim_is_bit_identical_run_to_run(gpu):
    from nu_nerf_amd.metrics import ssim
    a, b = random_pair(8, 800, 800, 3)
    ad, bd = dev_pair(gpu, a, b)
    first = ssim(ad, bd)
    for _ in range(3):
        assert torch.equal(ssim(ad, bd), first)
    assert bool(((first > 0) & (first < 1)).all())


def test_ssim_error_codes(gpu):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd.metrics import ssim
    lib = L.load()
    a = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device=gpu)
    m = torch.empty(2, dtype=torch.float64, device=gpu)
    nbytes = lib.nu_img_ssim_workspace_bytes(2, 20, 24, 3)
    assert nbytes > 0 and lib.nu_img_ssim_workspace_bytes(2, 20, 24, 2) == 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=gpu)

    def call(n, h, w, c, win, work_bytes):
        return lib.nu_img_ssim(L.ptr(a), L.ptr(a), n, h, w, c, win, L.ptr(m), None, L.ptr(work), work_bytes, L.stream())

    for bad in [(2, 20, 24, 3, 10, nbytes), (2, 20, 24, 3, 1, nbytes), (2, 20, 24, 3, 17, nbytes),      # even, too small, too large
                (2, 9, 24, 3, 11, nbytes), (2, 20, 9, 3, 11, nbytes), (2, 20, 24, 2, 11, nbytes)]:      # h < win, w < win, two channels
        with pytest.raises(L.NuNerfLibraryError, match="code -1"):
            call(*bad)
    with pytest.raises(L.NuNerfLibraryError, match="code -3"):
        call(2, 20, 24, 3, 11, nbytes - 1)
    assert call(0, 20, 24, 3, 11, 0) == 0 and call(2, 20, 24, 3, 11, nbytes) == 0
    torch.cuda.synchronize()
    assert m.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        ssim(a, a, win_size=8)
    with pytest.raises(ValueError):
        ssim(a[:, :5], a[:, :5])
    with pytest.raises(ValueError):
        ssim(a, a.float())


def build(gpu, g):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    cfg = {'name': 'golden', 'network': 'shape', 'database_name': 'synthetic/64', 'apply_occ_loss': True,
           'occ_loss_step': 15000, 'is_nerf': True, 'freeze_inv_s_step': 15000,
           'n_samples': 32, 'n_importance': 32, 'n_bg_samples': 16}
    net = NeROShapeRenderer(cfg, training=False)
    params = randomize_for_parity(init_stage1_params(6033), seed=1)
    for k in g:
        if k.startswith('override__'):
            params[k[len('override__'):]] = g[k]
    net.load_param_dict(params)
    return net.to(gpu)


def test_shape_render_metrics_on_a_validation_render(gpu, tmp_path, monkeypatch):
    from nu_nerf_amd.metrics import name2metrics, panel, to_uint8, _SHAPE_KEYS
    from nu_nerf_amd.synthetic import make_image_rays
    from nu_nerf_amd.validation import render_eval
    g = golden("eval_step20000_r40.npz")
    net = build(gpu, g)
    rays, h, w = make_image_rays(2, hw=32, downsample=0.5)
    assert (h, w) == (16, 16)
    out = render_eval(net, {k: torch.from_numpy(v).to(gpu) for k, v in rays.items()}, int(g['step']), chunk=100)
    data_pr = {k: v.reshape(h, w, -1) for k, v in out.items() if v.shape[0] == h * w}        # the per-ray images
    # a synthetic ground truth near the render, so that neither metric is degenerate
    noise = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).normal(0, 0.05, (h, w, 3)).astype(np.float32)).to(gpu)
    data_pr['gt_rgb'] = (data_pr['ray_rgb'] + noise).clamp(0, 1)
    monkeypatch.chdir(tmp_path)
    res = name2metrics['shape_render']({})(data_pr, {}, 300, data_index=4, model_name='unit-val')
    gt_u8, pr_u8 = O.to_uint8(data_pr['gt_rgb'].cpu().numpy()), O.to_uint8(data_pr['ray_rgb'].cpu().numpy())
    assert set(res) == {'psnr', 'ssim'} and all(isinstance(v, np.ndarray) and v.shape == (1,) and v.dtype == np.float64 for v in res.values())
    exact = O.psnr_exact(gt_u8, pr_u8)
    assert abs(res['psnr'][0] - exact) <= 1e-12 * exact and abs(res['psnr'][0] - float(O.compute_psnr_f32(gt_u8, pr_u8))) <= 10 * PSNR_F32_ERR_DB
    assert abs(res['ssim'][0] - O.ssim_exact(gt_u8, pr_u8, 11)[0]) <= 1e-12 and 0.0 < res['ssim'][0] < 1.0
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        pass
    else:
        assert abs(res['ssim'][0] - O.ssim_filter(gt_u8, pr_u8, 11)[0]) <= 10 * EXACT_VS_SKIMAGE
    # the picture: gt | pr | normal | 0 over three rows of four material maps
    img = panel(data_pr).cpu().numpy()
    assert img.shape == (4 * h, 4 * w, 3) and img.dtype == np.uint8
    assert np.array_equal(img[:h, :w], gt_u8) and np.array_equal(img[:h, w:2 * w], pr_u8)
    assert np.array_equal(img[:h, 2 * w:3 * w], O.to_uint8(data_pr['normal'].cpu().numpy())) and not img[:h, 3 * w:].any()
    for i, k in enumerate(_SHAPE_KEYS):
        want = O.to_uint8(data_pr[k].cpu().numpy())
        tile = img[(1 + i // 4) * h:(2 + i // 4) * h, (i % 4) * w:(i % 4 + 1) * w]
        assert np.array_equal(tile, np.repeat(want, 3, -1) if want.shape[-1] == 1 else want), k
    s2 = panel(data_pr, stage2=True).cpu().numpy()
    assert s2.shape == (2 * h, 3 * w, 3) and np.array_equal(s2[:h], img[:h, :3 * w])
    assert np.array_equal(s2[h:, :w], to_uint8(data_pr['specular_light']).cpu().numpy())
    res2 = name2metrics['stage2']({})(data_pr, {}, 300, data_index=5, model_name='unit-val')
    assert res2['psnr'][0] == res['psnr'][0] and res2['ssim'][0] == res['ssim'][0]
    try:
        from PIL import Image
    except ImportError:
        return
    for i, shape in ((4, img.shape), (5, s2.shape)):
        path = os.path.join('data', 'train_vis', 'unit-val', f'300-index-{i}.jpg')
        assert os.path.exists(path)
        with Image.open(path) as im:
            assert im.format == 'JPEG' and (im.height, im.width) == shape[:2]
