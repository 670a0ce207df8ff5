"""Host side of the environment export (no GPU): the Radiance writer against relight.read_hdr, the lat-long directions against float64
and against relight's lookup formula, the float64 oracle against the reference fixture, the clamp overrides, argument parsing."""
import os

import numpy as np
import pytest

import environment_oracle as EO
from helpers import golden


# ---- write_hdr / read_hdr ------------------------------------------------------------------------------------------------------------
def rgbe_bound(img):
    return 2.0 ** -8 * np.maximum(img, 0).max(-1, keepdims=True)


def test_hdr_round_trip(tmp_path):
    from nu_nerf_amd.environment import write_hdr
    from nu_nerf_amd.relight import read_hdr
    g = np.random.Generator(np.random.PCG64(1))
    h, w = 12, 37
    img = (g.random((h, w, 3)) * np.exp2(g.uniform(-20, 7, (h, w, 1)))).astype(np.float32)      # values across 2^-20 .. 2^7
    img[0, 0] = 0.0                                                  # a pixel of zeros
    img[0, 1] = (0.0, 2.0 ** -20, 0.0)
    img[0, 2] = (127.99, 1e-3, 100.0)
    img[0, 3] = (0.99999, 0.5, 0.25)                                 # the largest channel rounds up to 256 units: held to 255
    img[0, 4] = (1.0, 1.0, 1.0)
    img[1, 0] = (2.0, 2.0, 0.0)
    assert img.max() < 2.0 ** 7 and img[img > 0].min() < 2.0 ** -19
    p = write_hdr(str(tmp_path / 'a.hdr'), img)
    back = read_hdr(p)
    assert back.dtype == np.float32 and back.shape == img.shape
    assert (np.abs(back.astype(np.float64) - img) <= rgbe_bound(img.astype(np.float64))).all()
    assert (back[0, 0] == 0).all() and (back[0, 4] == 1.0).all() and back[0, 1, 1] == 2.0 ** -20
    # powers of two and their multiples by a byte come back exactly
    exact = np.exp2(np.arange(-20, 7, dtype=np.float64))[:, None, None] * np.asarray([1.0, 0.5, 0.75])[None, None]
    assert np.array_equal(read_hdr(write_hdr(str(tmp_path / 'b.hdr'), exact)), exact.astype(np.float32))
    # flat scanlines: header + 4 bytes per pixel
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 12 +X 37\n"
    data = open(p, 'rb').read()
    assert data.startswith(head) and len(data) == len(head) + 4 * h * w
    # widths at which a run-length scanline could start (8 .. 32767): a flat line is never taken for one
    wide = (g.random((3, 514, 3)) * np.exp2(g.uniform(-100, 7, (3, 514, 1)))).astype(np.float64)
    back = read_hdr(write_hdr(str(tmp_path / 'c.hdr'), wide))
    assert (np.abs(back - wide) <= rgbe_bound(wide)).all()
    # negative values are stored as 0; tiny pixels as (0, 0, 0, 0)
    neg = np.asarray([[[-1.0, 0.5, 0.25], [1e-45, 0.0, 0.0]]])
    assert np.array_equal(read_hdr(write_hdr(str(tmp_path / 'd.hdr'), neg)), np.asarray([[[0.0, 0.5, 0.25], [0.0, 0.0, 0.0]]], np.float32))


def test_hdr_writer_rejects_what_it_cannot_store(tmp_path):
    from nu_nerf_amd.environment import write_hdr
    for bad in (np.zeros((4, 4)), np.zeros((4, 4, 4)), np.zeros((0, 4, 3)), np.full((2, 2, 3), np.nan), np.full((2, 2, 3), np.inf),
                np.full((2, 2, 3), 1e39)):
        with pytest.raises(ValueError):
            write_hdr(str(tmp_path / 'x.hdr'), bad)


# ---- latlong_dirs ----------------------------------------------------------------------------------------------------------------------
def test_latlong_dirs_against_float64_and_the_lookup_formula():
    from nu_nerf_amd.environment import latlong_dirs
    for h, w in ((1, 1), (8, 16), (5, 7), (256, 512)):
        d = latlong_dirs(h, w)
        assert d.dtype == np.float32 and d.shape == (h * w, 3) and d.flags['C_CONTIGUOUS']
        r, c = np.divmod(np.arange(h * w), w)
        theta, phi = (r + 0.5) * np.pi / h, 2.0 * np.pi * (0.5 - (c + 0.5) / w)
        want = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
        assert np.abs(d - want).max() <= 2.0 ** -24                  # rounded once from float64 (|d| <= 1: half an ulp is 2^-25)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-7
        # relight's lookup (csrc/relight.h nu_relight_env) maps the direction of texel (r, c) to its centre (c + 1/2, r + 1/2)
        d64 = d.astype(np.float64)
        u = (0.5 - np.arctan2(d64[:, 1], d64[:, 0]) / (2.0 * np.pi)) * w
        v = np.arctan2(np.hypot(d64[:, 0], d64[:, 1]), d64[:, 2]) / np.pi * h
        assert np.abs(u - (c + 0.5)).max() < 1e-4 * w and np.abs(v - (r + 0.5)).max() < 1e-4 * h
    d = latlong_dirs(8, 16).reshape(8, 16, 3)
    assert (d[0, :, 2] > 0.9).all() and (d[-1, :, 2] < -0.9).all()   # row 0 = +z
    assert d[4, 7, 0] > 0.9 and abs(d[4, 7, 1]) < 0.25               # the map's centre looks along +x
    assert d[4, 3, 1] > 0.6 and d[4, 11, 1] < -0.6                   # +y is left of the centre
    with pytest.raises(ValueError):
        latlong_dirs(0, 4)


# ---- the oracle against the reference fixture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_oracle_against_the_reference_fixture(sphere):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    g = golden('environment_stage1.npz')
    pre = f'sd{int(sphere)}__'
    p = randomize_for_parity(init_stage1_params(6033, sphere_direction=sphere), seed=1)
    over = {k[len(pre + 'override__'):]: v for k, v in g.items() if k.startswith(pre + 'override__')}
    assert sorted(over) == sorted(EO.head_gain_overrides(p))
    for k, v in EO.head_gain_overrides(p).items():
        assert np.array_equal(over[k], v)
    p.update(over)
    d, rho, x = EO.rows(int(g['n_rows']), int(g['row_seed']))
    assert d.shape[0] == 512 and set(np.unique(rho)) == {np.float32(0.0), np.float32(0.03), np.float32(0.5), np.float32(1.0)}
    nx = np.linalg.norm(x.astype(np.float64), axis=1)
    assert int((nx > 0.999).sum()) >= 16 and nx.max() < 1.0
    assert np.array_equal(d[:2], [[0, 0, 1], [0, 0, -1]])           # the poles are among the rows ...
    v = g[pre + 'valid']
    assert np.array_equal(~v, (d[:, 0] == 0) & (d[:, 1] == 0))      # ... and are exactly the rows the reference has no result on
    o = EO.light64(p, d, rho, x, sphere=sphere, exp_max=float(g['exp_max']), probe=True)
    assert np.isfinite(o['light']).all()
    slack = 1.0 + 1e-9
    for k in ('direct', 'light'):
        e = float((np.abs(g[pre + k].astype(np.float64) - o[k]) / o[k])[v].max())
        assert e <= float(g[pre + 'dev_' + k]) * slack and e < 5e-5, (k, e)
    assert float(np.abs(g[pre + 'indirect'] - o['indirect'])[v].max()) <= float(g[pre + 'dev_indirect']) * slack
    assert float(np.abs(g[pre + 'occ_raw'] - o['occ_raw']).max()) <= float(g[pre + 'dev_occ']) * slack < 2e-6
    sh = EO.shares(o, float(g['exp_max']))
    assert sh[5] >= 0.1 and max(sh[4], sh[6]) >= 0.1
    assert o['light'].max() / o['light'].min() > 1.1               # the radiance varies a thousand times the tolerance of the GPU tests


@pytest.mark.parametrize("sphere", [False, True])
def test_clamp_overrides_meet_the_shares_on_the_oracle_alone(sphere):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    p = randomize_for_parity(init_stage1_params(6033, sphere_direction=sphere), seed=1)
    p.update(EO.head_gain_overrides(p))
    d, rho, x = EO.rows(512, 2027)                                   # the rows of test_both_sides_of_every_clamp
    over = EO.clamp_overrides(p, d, rho, x, sphere=sphere, exp_max=3.0)
    assert sorted(k.split('.', 1)[1] for k in over) == ['inner_light.6.bias', 'inner_weight.6.bias', 'inner_weight.6.weight_g', 'outer_light.6.bias']
    p.update(over)
    sh = EO.shares(EO.light64(p, d, rho, x, sphere=sphere, exp_max=3.0, probe=True), 3.0)
    assert min(sh) >= 0.1, sh
    assert abs(sh[4] - 0.25) < 0.02 and abs(sh[6] - 0.25) < 0.02


def test_oracle_modes_agree():
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    p = randomize_for_parity(init_stage1_params(6033, sphere_direction=True), seed=1)
    d, rho, x = EO.rows(40, 3)
    a = EO.light64(p, d, rho, None, sphere=True)
    b = EO.light64(p, d, rho, np.zeros(3), sphere=True, probe=True)
    assert np.array_equal(a['light'], b['direct']) and set(a) == {'direct', 'light', 'raw'}
    assert np.allclose(EO.light64(p, d, rho, x[7], sphere=True)['light'], EO.light64(p, d, rho, np.tile(x[7], (40, 1)), sphere=True)['light'], rtol=1e-12, atol=0)
    assert np.allclose(b['light'], b['indirect'] + b['direct'] * (1 - b['occ'][:, None]))


# ---- the command's arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_parsing():
    from nu_nerf_amd.extract_environment import output_dir, parse_args
    f = parse_args(['--cfg', 'a.yaml'])
    assert (f.height, f.width, f.roughness, f.point, f.probe, f.stage2, f.which) == (256, 512, [0.0, 0.25, 0.5, 0.75, 1.0], None, False, False, None)
    assert output_dir(f, 'bear', 300000) == os.path.join('data', 'environment', 'bear-300000')
    f = parse_args(['--cfg', 'a.yaml', '--stage2', '--which', 'inner', '--height', '64', '--width', '128', '--roughness', '0', '1',
                    '--point', '0.1', '-0.2', '0.3', '--probe', '--out', 'somewhere'])
    assert (f.stage2, f.which, f.height, f.width, f.roughness, f.point, f.probe) == (True, 'inner', 64, 128, [0.0, 1.0], [0.1, -0.2, 0.3], True)
    assert output_dir(f, 'bear', 1) == 'somewhere'
    for bad in ([], ['--cfg', 'a.yaml', '--which', 'inner'], ['--cfg', 'a.yaml', '--which', 'middle', '--stage2'],
                ['--cfg', 'a.yaml', '--height', '0'], ['--cfg', 'a.yaml', '--roughness', '-0.5'], ['--cfg', 'a.yaml', '--point', '1', '2'],
                ['--cfg', 'a.yaml', '--roughness']):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_the_entry_is_declared_and_its_kernel_has_no_spill():
    """nu_light_bake_fwd takes the existing NuShadeNet: no new struct, no size entry.  The kernel keeps its accumulators in registers:
    no spilled VGPR and no scratch memory (scripts/kernel_regs.py on the built object), and its LDS fits one workgroup per CU."""
    import sys
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert len(lib.nu_light_bake_fwd.argtypes) == 15 and 'LbNet' not in _lib.STRUCTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    from kernel_regs import kernel_table
    table = dict(kernel_table(os.path.join(root, 'nu_nerf_amd', 'build', 'light_bake.o')))
    (name, r), = [(k, v) for k, v in table.items() if k.startswith('light_bake_fwd_kernel')]
    assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] <= 160 * 1024, (name, r)
