"""Validation metrics, host side (no GPU): the two numpy oracles of SSIM against each other and against what scikit-image itself
returned (tests/golden/metrics_skimage.npz, scripts/gen_metrics_golden.py), the C ABI declarations and their binding, the command
line on a stub of the device functions, and the opt-in compat switch in a fresh interpreter."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import metrics_oracle as O
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the CPU over the fixture cases (the figures the GPU tests take their bounds from):
#   largest |ssim_exact - skimage| of the mean: 2.665e-15 (smooth_96x128) -- skimage's float64 rounding in its running-sum filters
#   largest |compute_psnr_f32 - psnr_exact|:    1.365e-4 dB (noise_64x80) -- the reference's float32 mean over pixels
EXACT_VS_SKIMAGE = 2.665e-15
PSNR_F32_ERR_DB = 1.365e-4


def fixture_cases():
    g = golden("metrics_skimage.npz")
    return g, [str(n) for n in g['cases']]


def test_fixture_has_the_cases_the_checks_rely_on():
    g, names = fixture_cases()
    assert len(names) == 9 and all(g[n + '_a'].dtype == np.uint8 and g[n + '_a'].shape == g[n + '_b'].shape for n in names)
    assert float(g['identical_32x40_mssim']) == 1.0 and O.ssd_exact(g['identical_32x40_a'], g['identical_32x40_b']) == 0
    assert int(g['win7_45x50_win']) == 7 and g['gray_33x29_a'].shape[2] == 1 and g['single_11x11_a'].shape == (11, 11, 3)
    assert g['odd_37x23_smap'].shape == (27, 13, 3) and int(g['dark_40x40_a'].max()) <= 5
    # the saturated pair reaches the largest window sums an 11 x 11 window can have, and they stay below 2^24
    a, b = g['saturated_48x64_a'].astype(np.int64), g['saturated_48x64_b'].astype(np.int64)
    assert O.window_sums(a * b, 11).max() == 121 * 255 * 255 < 2 ** 24 and 225 * 255 * 255 < 2 ** 24


def test_exact_integer_oracle_agrees_with_skimage():
    g, names = fixture_cases()
    worst = 0.0
    for n in names:
        m, smap = O.ssim_exact(g[n + '_a'], g[n + '_b'], int(g[n + '_win']))
        worst = max(worst, abs(m - float(g[n + '_mssim'])))
        if n + '_smap' in g:
            assert smap.shape == g[n + '_smap'].shape
            assert np.abs(smap - g[n + '_smap']).max() < 1e-12
    print(f"largest |exact-integer oracle - skimage| over the fixture: {worst:.3e}")
    assert worst <= 10 * EXACT_VS_SKIMAGE


def test_filter_oracle_agrees_with_skimage_and_with_the_exact_one():
    pytest.importorskip("scipy")
    g, names = fixture_cases()
    for n in names:
        win = int(g[n + '_win'])
        mf, sf = O.ssim_filter(g[n + '_a'], g[n + '_b'], win)
        me, se = O.ssim_exact(g[n + '_a'], g[n + '_b'], win)
        assert abs(mf - float(g[n + '_mssim'])) <= 10 * EXACT_VS_SKIMAGE, n
        assert abs(mf - me) <= 10 * EXACT_VS_SKIMAGE and sf.shape == se.shape and np.abs(sf - se).max() < 1e-11, n


def test_float32_psnr_restatement_error_is_what_was_measured():
    g, names = fixture_cases()
    worst = 0.0
    for n in names:
        a, b = g[n + '_a'], g[n + '_b']
        if a.shape[2] == 3 and O.ssd_exact(a, b) > 0:
            worst = max(worst, abs(float(O.compute_psnr_f32(a, b)) - O.psnr_exact(a, b)))
    print(f"largest |float32 compute_psnr - exact| over the fixture: {worst:.3e} dB")
    assert 0.0 < worst <= 10 * PSNR_F32_ERR_DB
    assert O.psnr_exact(g['identical_32x40_a'], g['identical_32x40_b']) == float('inf')
    assert np.isinf(O.compute_psnr_f32(g['identical_32x40_a'], g['identical_32x40_b']))


def test_quantisation_oracle_truncates_and_clamps():
    x = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, 254.999 / 255, 1 / 255, np.inf, -np.inf], np.float32)
    assert O.to_uint8(x).tolist() == [0, 0, 0, 127, 255, 255, 254, 1, 255, 0]


def test_header_declares_the_metric_entries_and_the_binding_maps_them():
    import ctypes
    from nu_nerf_amd import _lib
    sig = {name: (res, args) for name, res, args in _lib._signatures()}
    p, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert sig['nu_img_quantize'] == (i, [p, ll, p, p])
    assert sig['nu_img_sqdiff'] == (i, [p, p, i, ll, p, p])
    assert sig['nu_img_ssim_workspace_bytes'] == (ll, [i, i, i, i])
    assert sig['nu_img_ssim'] == (i, [p, p, i, i, i, i, i, p, p, p, ll, p])


def _write_images(d, items):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for name, arr in items.items():
        Image.fromarray(arr[..., 0] if arr.shape[2] == 1 else arr).save(os.path.join(d, name))


def test_command_line_matches_directories_by_stem_and_prints_one_json_line(tmp_path, monkeypatch, capsys):
    pytest.importorskip("PIL")
    from nu_nerf_amd import metrics as M
    g = np.random.Generator(np.random.PCG64(5))
    img = lambda c: g.integers(0, 256, (20, 24, c)).astype(np.uint8)
    pr = {'a.png': img(3), 'b.png': img(3), 'only_pr.png': img(3), 'grey.png': img(1)}
    gt = {'a.png': img(3), 'b.bmp': pr['b.png'].copy(), 'only_gt.png': img(3), 'grey.png': img(1)}
    _write_images(str(tmp_path / 'pr'), pr)
    _write_images(str(tmp_path / 'gt'), gt)
    assert [m[0] for m in M.match_files(str(tmp_path / 'pr'), str(tmp_path / 'gt'))] == ['a', 'b', 'grey']
    with pytest.raises(ValueError):
        M.match_files(str(tmp_path / 'pr'), str(tmp_path / 'gt' / 'a.png'))
    # the device functions, stood in for by the numpy oracle on CPU tensors
    monkeypatch.setattr(M, '_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(M, 'psnr', lambda gt_, pr_: torch.tensor([O.psnr_exact(gt_.numpy(), pr_.numpy())], dtype=torch.float64))
    monkeypatch.setattr(M, 'ssim', lambda gt_, pr_, win_size=11: torch.tensor([O.ssim_exact(gt_.numpy(), pr_.numpy(), win_size)[0]],
                                                                                dtype=torch.float64))
    res = M.main([str(tmp_path / 'pr'), str(tmp_path / 'gt'), '--win-size', '7'])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == res
    assert set(res) == {'images', 'psnr', 'ssim', 'win_size', 'count'} and res['count'] == 3 and res['win_size'] == 7
    assert [i['name'] for i in res['images']] == ['a', 'b', 'grey'] and all(set(i) == {'name', 'psnr', 'ssim'} for i in res['images'])
    assert res['images'][0]['psnr'] == O.psnr_exact(gt['a.png'], pr['a.png'])
    assert res['images'][0]['ssim'] == O.ssim_exact(gt['a.png'], pr['a.png'], 7)[0]
    assert res['images'][1] == {'name': 'b', 'psnr': float('inf'), 'ssim': 1.0} and res['psnr'] == float('inf')
    assert res['images'][2]['ssim'] == O.ssim_exact(gt['grey.png'], pr['grey.png'], 7)[0]          # read as one channel
    # two files
    one = M.main([str(tmp_path / 'pr' / 'a.png'), str(tmp_path / 'gt' / 'a.png')])
    assert one['count'] == 1 and one['win_size'] == 11 and one['images'][0]['psnr'] == res['images'][0]['psnr']
    with pytest.raises(SystemExit):
        M.main([str(tmp_path / 'pr' / 'a.png'), str(tmp_path / 'gt' / 'grey.png')])                # shapes differ


def test_registries_have_the_reference_entries_without_the_material_stage():
    from nu_nerf_amd import metrics as M
    assert set(M.name2metrics) == {'shape_render', 'stage2'} and set(M.name2key_metrics) == {'psnr'}
    assert M.name2key_metrics['psnr']({'psnr': np.array([30.0, 32.0])}) == 31.0
    assert M.name2metrics['stage2']({}).stage2 and not M.name2metrics['shape_render']({}).stage2


COMPAT_DRIVER = '''
import os
import network.loss as refloss
import network.metrics as m
assert refloss.MARK == "checkout"
if os.environ.get("NU_NERF_DEVICE_METRICS") == "1":
    import nu_nerf_amd.metrics
    from network.metrics import name2metrics, name2key_metrics         # what train/trainer_zero.py:15 and train_valid.py:7 import
    from network import metrics as again
    assert m is nu_nerf_amd.metrics and again is m and set(name2metrics) == {"shape_render", "stage2"} and "psnr" in name2key_metrics
    print("device metrics")
else:
    assert m.MARK == "checkout metrics"
    print("checkout metrics")
'''


@pytest.mark.parametrize("setting, expect", [("1", "device metrics"), (None, "checkout metrics"), ("0", "checkout metrics")])
def test_compat_answers_network_metrics_only_when_asked(tmp_path, setting, expect):
    ck = tmp_path / "checkout"
    (ck / "network").mkdir(parents=True)
    (ck / "network" / "loss.py").write_text('MARK = "checkout"\n')
    (ck / "network" / "metrics.py").write_text('MARK = "checkout metrics"\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nu_nerf_amd", "compat"), ROOT, str(ck)]))
    env.pop("NU_NERF_DEVICE_METRICS", None)
    if setting is not None:
        env["NU_NERF_DEVICE_METRICS"] = setting
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(COMPAT_DRIVER)], cwd=str(ck), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and expect in r.stdout, r.stdout + r.stderr
