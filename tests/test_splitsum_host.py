"""Host side of split-sum relighting (no GPU): the float64 oracle against the closed forms, the tap rule, the file-format fall-backs of
--pyramid, argument parsing of the two commands, the declared entries and the kernels' resource figures."""
import os

import numpy as np
import pytest

import splitsum_oracle as SO

A_LIN = (0.3, -0.5, 0.4)


def _table(env):
    from nu_nerf_amd.environment import source_table
    return source_table(env)


def _linear_env(h, w):
    from nu_nerf_amd.environment import latlong_dirs
    return SO.linear_map(h, w, A_LIN, latlong_dirs).astype(np.float32)


# ---- the oracle's closed forms ---------------------------------------------------------------------------------------------------------
def test_oracle_closed_forms():
    """On the 64 x 128 map of E = 1 + a.omega the quadrature (texel centres, w = sin theta) is what separates the oracle from the closed
    forms: 6.9e-5 for the cosine lobe, at most 1.4e-4 for the vMF lobes -- the GPU test allows 2e-4 / 4e-4 in all."""
    from nu_nerf_amd.environment import latlong_dirs
    sd, rgb = _table(_linear_env(64, 128))
    d = latlong_dirs(6, 12)
    lobes = ['cosine'] + [('vmf', r) for r in (0.1, 0.25, 0.5, 1.0)]
    got = SO.prefilter(sd, rgb, d, lobes)
    e_cos = np.abs(got[0] - SO.cosine_of_linear(A_LIN, d)[:, None]).max()
    e_vmf = [np.abs(got[1 + k] - SO.vmf_of_linear(A_LIN, d, r)[:, None]).max() for k, r in enumerate((0.1, 0.25, 0.5, 1.0))]
    print(f"oracle vs closed forms: cosine {e_cos:.2e}, vMF {['%.2e' % e for e in e_vmf]}")
    assert e_cos < 1e-4 and max(e_vmf) < 2e-4
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])


def test_oracle_constant_map_and_lobes():
    from nu_nerf_amd.environment import latlong_dirs, lobe_falloff, lobe_param
    sd, rgb = _table(np.full((5, 9, 3), 3.25, np.float32))
    d = latlong_dirs(3, 4)
    got = SO.prefilter(sd, rgb, d, ['cosine', ('ggx', 0.2), ('ggx', 1.0), ('vmf', 0.3)])
    assert np.abs(got - 3.25).max() < 1e-14
    # the package's parameters and fall-off are the oracle's
    for kind, rho in (('ggx', 0.0), ('ggx', 0.01), ('ggx', 0.5), ('vmf', 0.25), ('cosine', None)):
        assert abs(lobe_param(kind, rho) - SO.lobe_param(kind, rho)) <= 1e-7 * max(1.0, SO.lobe_param(kind, rho))
        for ang in (0.0, 0.05, 0.7, 2.0):
            p = SO.lobe_param(kind, rho)
            want = SO.lobe(kind, p, np.cos(ang)) / SO.lobe(kind, p, 1.0)
            assert abs(lobe_falloff(kind, rho, ang) - want) <= 1e-6 * max(want, 1e-30) + 1e-300
    assert lobe_param('ggx', 0.0) == 1e-3 and lobe_param('vmf', 0.5) == 2.0
    with pytest.raises(ValueError):
        lobe_param('vmf', 0.0)
    with pytest.raises(ValueError):
        lobe_param('phong', 0.5)


def test_oracle_pyramid_lookup_and_resolve():
    g = np.random.Generator(np.random.PCG64(3))
    pyr = g.random((3, 4, 8, 3))
    levels = np.asarray([0.1, 0.5, 0.9])
    d = g.normal(size=(7, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    import relight_oracle as RO
    for k, lv in enumerate(levels):
        assert np.array_equal(SO.pyramid_lookup(pyr, levels, d, np.full(7, lv)), RO.env_lookup(pyr[k], d))
    assert np.array_equal(SO.pyramid_lookup(pyr, levels, d, np.full(7, -1.0)), RO.env_lookup(pyr[0], d))
    assert np.array_equal(SO.pyramid_lookup(pyr, levels, d, np.full(7, 7.0)), RO.env_lookup(pyr[2], d))
    mid = SO.pyramid_lookup(pyr, levels, d, np.full(7, 0.3))
    assert np.allclose(mid, 0.5 * (RO.env_lookup(pyr[0], d) + RO.env_lookup(pyr[1], d)), rtol=1e-14)
    assert np.array_equal(SO.pyramid_lookup(pyr[:1], levels[:1], d, np.full(7, 0.3)), RO.env_lookup(pyr[0], d))
    # white furnace of the resolve: ones in, (1 - m) a + F0 A + B out
    from nu_nerf_amd.params import load_fg_lut
    lut = load_fg_lut()[0].astype(np.float64)
    rows = np.zeros((5, 20))
    rows[:, 7:10] = rows[:, 15:18] = d[:5]
    rows[:, 15:18] += 0.3 * d[1:6]
    rows[:, 15:18] /= np.linalg.norm(rows[:, 15:18], axis=1, keepdims=True)
    rows[:, 10:13], rows[:, 13], rows[:, 14] = g.random((5, 3)), g.random(5), g.random(5)
    got = SO.resolve(rows, np.ones((2, 4, 8, 3)), [0.0, 1.0], np.ones((4, 8, 3)), lut)
    nov = np.sum(rows[:, 7:10] * rows[:, 15:18], 1)
    ab = RO.fg_lookup(lut, nov, rows[:, 14])
    m, a = rows[:, 13:14], rows[:, 10:13]
    assert np.allclose(got, (1 - m) * a + (0.04 * (1 - m) + m * a) * ab[:, :1] + ab[:, 1:], rtol=1e-13)


# ---- the tap rule ------------------------------------------------------------------------------------------------------------------------
def test_tap_rule():
    from nu_nerf_amd.environment import lobe_is_tapped
    for H in (1, 8, 256, 4096):
        assert lobe_is_tapped('ggx', 0.0, H) and lobe_is_tapped('vmf', 0.0, H)          # roughness 0 always
        assert not lobe_is_tapped('cosine', None, H) and not lobe_is_tapped('cosine', 0.0, H)
    # the rule itself, from the lobes in float64: weight one pitch off axis below half the peak
    for kind in ('ggx', 'vmf'):
        for H in (16, 64, 256):
            for rho in (0.02, 0.05, 0.1, 0.25, 0.5, 1.0):
                p = SO.lobe_param(kind, rho)
                ratio = SO.lobe(kind, p, np.cos(np.pi / H)) / SO.lobe(kind, p, 1.0)
                assert lobe_is_tapped(kind, rho, H) == bool(ratio < 0.5), (kind, H, rho, ratio)
    # monotone in the roughness and in the resolution; the default pyramid on the default map regresses every level but the first
    assert [lobe_is_tapped('ggx', r, 256) for r in (0.0, 0.25, 0.5, 0.75, 1.0)] == [True, False, False, False, False]
    assert lobe_is_tapped('ggx', 0.25, 16) and not lobe_is_tapped('ggx', 0.5, 16)
    assert lobe_is_tapped('vmf', 0.01, 16) and not lobe_is_tapped('vmf', 0.01, 64)       # kappa (1 - cos(pi / H)) against ln 2


def test_source_table():
    from nu_nerf_amd.environment import latlong_dirs, source_table
    env = np.arange(5 * 7 * 3, dtype=np.float32).reshape(5, 7, 3)
    sd, rgb = source_table(env)
    assert sd.dtype == rgb.dtype == np.float32 and sd.shape == rgb.shape == (35, 4)
    assert np.array_equal(sd[:, :3], latlong_dirs(5, 7)) and np.array_equal(rgb[:, :3], env.reshape(-1, 3)) and (rgb[:, 3] == 0).all()
    theta = (np.arange(5) + 0.5) * np.pi / 5
    assert np.array_equal(sd[:, 3], np.repeat(np.sin(theta), 7).astype(np.float32)) and (sd[:, 3] > 0).all()
    assert abs(sd[:, 3].astype(np.float64).sum() * (np.pi / 5) * (2 * np.pi / 7) / (4 * np.pi) - 1.0) < 0.02      # the sphere's area
    for bad in (np.zeros((4, 4)), np.zeros((4, 4, 4)), np.zeros((0, 4, 3)), np.full((2, 2, 3), np.nan)):
        with pytest.raises(ValueError):
            source_table(bad)


# ---- file formats ------------------------------------------------------------------------------------------------------------------------
def test_pyramid_directory_fall_backs(tmp_path):
    from nu_nerf_amd.relight import load_pyramid_dir, pack_pyramid
    g = np.random.Generator(np.random.PCG64(5))
    pyr = g.random((3, 4, 8, 3)).astype(np.float32)
    d = tmp_path / 'a'
    d.mkdir()
    np.save(d / 'env_pyramid.npy', pyr)
    np.save(d / 'roughness.npy', np.asarray([0.0, 0.5, 1.0], np.float32))
    p, lv, dif = load_pyramid_dir(str(d))                              # as extract_environment writes it: diffuse = the level of roughness 1
    assert np.array_equal(p, pyr) and np.array_equal(lv, [0.0, 0.5, 1.0]) and np.array_equal(dif, pyr[2])
    own = g.random((2, 4, 3)).astype(np.float32)
    np.save(d / 'env_diffuse.npy', own)
    assert np.array_equal(load_pyramid_dir(str(d))[2], own)            # its own diffuse map wins
    e = tmp_path / 'b'
    e.mkdir()
    np.save(e / 'env_pyramid.npy', pyr)
    np.save(e / 'roughness.npy', np.asarray([1.0, 0.0, 0.5], np.float32))
    p, lv, dif = load_pyramid_dir(str(e))                              # levels in any order: sorted, the diffuse map still roughness 1
    assert np.array_equal(lv, [0.0, 0.5, 1.0]) and np.array_equal(p, pyr[[1, 2, 0]]) and np.array_equal(dif, pyr[0])
    np.save(e / 'roughness.npy', np.asarray([0.0, 0.25, 0.5], np.float32))
    with pytest.raises(ValueError, match="roughness 1"):
        load_pyramid_dir(str(e))
    np.save(e / 'roughness.npy', np.asarray([0.0, 1.0], np.float32))
    with pytest.raises(ValueError):
        load_pyramid_dir(str(e))
    packed, lv = pack_pyramid(pyr, [0.0, 0.5, 1.0])
    assert packed.shape == (3, 4, 8, 4) and packed.dtype == np.float32 and (packed[..., 3] == 1).all() and lv.dtype == np.float32
    for bad_p, bad_l in ((pyr, [0.0, 0.5]), (pyr, [0.0, 0.5, 0.5]), (pyr, [0.5, 0.0, 1.0]), (pyr, [0.0, np.nan, 1.0]), (pyr[0], [0.0]),
                         (np.full_like(pyr, np.inf), [0.0, 0.5, 1.0]), (np.zeros((17, 1, 1, 3)), np.arange(17))):
        with pytest.raises(ValueError):
            pack_pyramid(bad_p, bad_l)


# ---- the commands' arguments ---------------------------------------------------------------------------------------------------------------
def test_relight_arguments():
    from nu_nerf_amd.relight import parse_args
    base = ['--mesh', 'm.ply', '--material', 'mat', '--name', 'x']
    f = parse_args(base + ['--hdr', 'e.hdr'])
    assert (f.splitsum, f.pyramid, f.levels, f.samples) == (False, None, None, 1024)          # the defaults do not change
    f = parse_args(base + ['--splitsum', '--hdr', 'e.hdr'])
    assert f.splitsum and f.hdr == 'e.hdr' and f.pyramid is None and f.levels is None
    f = parse_args(base + ['--splitsum', '--hdr', 'e.hdr', '--levels', '0', '0.5', '1'])
    assert f.levels == [0.0, 0.5, 1.0]
    f = parse_args(base + ['--splitsum', '--pyramid', 'dir'])
    assert f.pyramid == 'dir' and f.hdr is None
    for bad in (base,                                                                          # no map at all
                base + ['--pyramid', 'dir', '--hdr', 'e.hdr'],                                 # --pyramid without --splitsum
                base + ['--hdr', 'e.hdr', '--levels', '0', '1'],
                base + ['--splitsum'], base + ['--splitsum', '--hdr', 'e.hdr', '--pyramid', 'dir'],
                base + ['--splitsum', '--pyramid', 'dir', '--levels', '0', '1'],
                base + ['--splitsum', '--hdr', 'e.hdr', '--levels', '1', '0'],
                base + ['--splitsum', '--hdr', 'e.hdr', '--levels', '-1', '0'],
                ['--mesh', 'm.ply', '--name', 'x', '--splitsum', '--hdr', 'e.hdr', '--inner', 'i.ply', '--inner-material', 'im']):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_prefilter_environment_arguments():
    from nu_nerf_amd.prefilter_environment import output_dir, parse_args
    f = parse_args(['--hdr', 'maps/sky.hdr'])
    assert (f.height, f.width, f.roughness, f.lobe, f.diffuse) == (None, None, [0.0, 0.25, 0.5, 0.75, 1.0], 'ggx', 'cosine')
    assert output_dir(f) == os.path.join('data', 'environment', 'sky-prefiltered')
    f = parse_args(['--hdr', 'a.npy', '--out', 'o', '--height', '8', '--width', '16', '--roughness', '0', '1', '--lobe', 'vmf', '--diffuse', 'vmf'])
    assert (f.height, f.width, f.roughness, f.lobe, f.diffuse, output_dir(f)) == (8, 16, [0.0, 1.0], 'vmf', 'vmf', 'o')
    for bad in ([], ['--hdr', 'a', '--height', '0'], ['--hdr', 'a', '--roughness', '1', '0'], ['--hdr', 'a', '--roughness', '-1'],
                ['--hdr', 'a', '--lobe', 'cosine'], ['--hdr', 'a', '--diffuse', 'ggx']):
        with pytest.raises(SystemExit):
            parse_args(bad)


# ---- the entries and their kernels -----------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_the_kernels_have_no_spill():
    """The three entries take flat arguments (no new struct) and are bound from the header; the workspace size is a pure host function.
    Found (scripts/kernel_regs.py on the built objects): no spilled VGPR, no scratch; the prefilter kernel 80 .. 203 VGPRs (1 .. 16
    lobes; 123 at the 6 of the default pyramid) and 8 KiB of LDS, the lookup 53 and the resolve 75 VGPRs, no LDS."""
    import sys
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert len(lib.nu_env_prefilter.argtypes) == 12 and len(lib.nu_env_pyramid_lookup.argtypes) == 10
    assert len(lib.nu_relight_splitsum.argtypes) == 14 and len(lib.nu_env_prefilter_workspace_bytes.argtypes) == 3
    assert (_lib.NU_LOBE_COSINE, _lib.NU_LOBE_GGX, _lib.NU_LOBE_VMF, _lib.NU_ENV_MAX_LOBES) == (0, 1, 2, 16)
    assert not [k for k in _lib.STRUCTS if 'Env' in k or 'Prefilter' in k or 'Split' in k]
    ws = lib.nu_env_prefilter_workspace_bytes
    assert ws(0, 512, 5) == 0 and ws(64, 0, 5) == 0 and ws(64, 256, 5) == 0              # nothing to do, or one tile: no split
    assert ws(64, 512, 5) == 2 * 5 * 64 * 16 and ws(64, 131072, 3) == 512 * 3 * 64 * 16  # few queries: every tile's contribution is kept
    assert ws(128 * 256, 131072, 6) == 0                                                 # the query blocks fill the chip
    assert ws(32767, 131072, 16) == 0                                                    # the workspace would be too large
    for bad in ((-1, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 17)):
        with pytest.raises(_lib.NuNerfLibraryError):
            ws(*bad)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    from kernel_regs import kernel_table
    pf = {k: v for k, v in kernel_table(os.path.join(root, 'nu_nerf_amd', 'build', 'env_prefilter.o')) if k.startswith('pf_')}
    assert len(pf) == 33, sorted(pf)                                  # 16 lobe counts x (whole, split) + the fold
    for name, r in pf.items():
        assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] <= 8192 and r['vgpr'] <= 256, (name, r)
    rl = dict(kernel_table(os.path.join(root, 'nu_nerf_amd', 'build', 'relight.o')))
    for prefix in ('relight_pyramid_lookup_kernel', 'relight_splitsum_kernel'):
        (name, r), = [(k, v) for k, v in rl.items() if k.startswith(prefix)]
        assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] == 0, (name, r)
    print({k[:22]: (v['vgpr'], v['sgpr'], v['lds']) for k, v in pf.items() if '<6,' in k or '<16,' in k or '<1,' in k})
