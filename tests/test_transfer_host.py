"""Visibility transfer, the parts that need no GPU: the SH projection of an environment against its closed forms, the
unoccluded transfer vector, the sample oracle's invariants, the analytic sphere occluder the GPU test leans on, command arguments,
the file layout and the ABI."""
import os
import re

import numpy as np
import pytest

import splitsum_oracle as SO
import transfer_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_LIN = (0.3, -0.5, 0.4)
Y00, Y1 = 0.282095, 0.488603
# the header gives the SH constants to six decimals: a coefficient carries their rounding, at most 5e-7 absolute on a constant >= 0.28
CONST_REL = 5e-7 / Y00


def _dirs64(h, w):
    """latlong_dirs before its rounding to float32."""
    theta = (np.arange(h) + 0.5) * np.pi / h
    phi = 2.0 * np.pi * (0.5 - (np.arange(w) + 0.5) / w)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    return np.stack([st * np.cos(phi)[None], st * np.sin(phi)[None], np.broadcast_to(ct, (h, w))], -1).reshape(h * w, 3)


def test_project_sh_closed_forms():
    """A constant map c: L_0 = 2 sqrt(pi) c, the rest 0.  E = 1 + a.omega: L_1m = 0.488603 (4 pi / 3) a_m, band 2 = 0.  The tolerance is the
    quadrature's own error at 64 x 128 -- its distance to the 256 x 512 quadrature of the same function, computed here -- plus the
    rounding of the six-decimal constants where the closed form is written with the exact 2 sqrt(pi)."""
    from nu_nerf_amd.environment import project_sh
    c = np.asarray([0.7, 1.3, 2.1])
    coarse, fine = (project_sh(np.broadcast_to(c, (h, w, 3))) for h, w in ((64, 128), (256, 512)))
    # the midpoint rule is of second order: the 4 x finer map is 16 x closer to the limit, so the coarse map's own error is 16/15 of the
    # distance between the two
    quad = np.abs(coarse - fine).max() * (16.0 / 15.0)
    assert coarse.shape == (9, 3) and coarse.dtype == np.float64
    assert np.abs(coarse[0] - 2.0 * np.sqrt(np.pi) * c).max() <= quad + CONST_REL * 2.0 * np.sqrt(np.pi) * c.max() + 1e-15
    assert np.abs(coarse[0] - 4.0 * np.pi * Y00 * c).max() <= quad + 1e-14         # with the constant as given: the quadrature alone
    assert np.abs(coarse[1:]).max() <= quad + 1e-12                                # (2,0) carries the quadrature error, the others cancel
    lin_c, lin_f = (project_sh(SO.linear_map(h, w, A_LIN, _dirs64)) for h, w in ((64, 128), (256, 512)))
    quad = np.abs(lin_c - lin_f).max()
    tol = quad * (16.0 / 15.0) + 1e-14
    a = np.asarray(A_LIN)
    want1 = Y1 * (4.0 * np.pi / 3.0) * np.asarray([a[1], a[2], a[0]])              # order (1,-1) (1,0) (1,1) = y, z, x
    print(f"project_sh at 64 x 128: quadrature error {quad:.3e}; band 1 off by {np.abs(lin_c[1:4] - want1[:, None]).max():.3e}, "
          f"band 2 at {np.abs(lin_c[4:]).max():.3e}")
    assert np.abs(lin_c[1:4] - want1[:, None]).max() <= tol
    assert np.abs(lin_c[4:]).max() <= tol
    assert np.abs(lin_c[0] - 4.0 * np.pi * Y00).max() <= tol
    with pytest.raises(ValueError):
        project_sh(np.zeros((4, 8)))
    with pytest.raises(ValueError):
        project_sh(np.full((4, 8, 3), np.nan))


def test_unoccluded_transfer_lights_like_the_cosine_lobe():
    """sum_k unoccluded_transfer(n)_k L_k = 1 + (2/3) a.n for E = 1 + a.omega (section 28's closed form of the diffuse map)."""
    from nu_nerf_amd.environment import project_sh
    from nu_nerf_amd.transfer import sh_basis, unoccluded_transfer
    g = np.random.Generator(np.random.PCG64(5))
    n = g.normal(size=(200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    T = unoccluded_transfer(n)
    assert T.shape == (200, 9) and np.array_equal(T, TO.unoccluded(n)) and np.array_equal(sh_basis(n), TO.sh9(n))
    coarse, fine = (project_sh(SO.linear_map(h, w, A_LIN, _dirs64)) for h, w in ((64, 128), (256, 512)))
    quad = np.abs(coarse - fine).max() * (16.0 / 15.0)
    got = T @ coarse[:, 0]
    # |T_k| <= 0.49 and nine terms; the constants enter squared (Y_k in T and in L): 2 CONST_REL of a value <= 2
    tol = 9 * 0.49 * quad + 4.0 * CONST_REL + 1e-14
    dev = np.abs(got - SO.cosine_of_linear(A_LIN, n)).max()
    print(f"unoccluded transfer . env SH vs 1 + (2/3) a.n: {dev:.3e} (bound {tol:.3e})")
    assert dev <= tol


def test_sample_oracle_invariants():
    """The uniforms are multiples of 2^-24 in [0, 1), the directions are unit and strictly above the horizon; one lobe of S points: the
    first coordinates of a point's samples are the S shifted multiples of 2^32 / S."""
    g = np.random.Generator(np.random.PCG64(6))
    n = g.normal(size=(7, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[0] = (0, 0, 1)
    n[1] = (0, 0, -1)
    p = g.uniform(-1, 1, (7, 3))
    for S in (16, 32, 48, 1024):
        b1, b2 = TO.sample_bits(np.arange(7) + 3, 11, S)
        assert b1.shape == (7, S) and b1.dtype == np.int64 and b1.min() >= 0 and max(b1.max(), b2.max()) < 2 ** 24
        assert (np.sort(np.diff(np.sort(b1, 1), axis=1), 1)[:, 0] >= (2 ** 24 // S) - 1).all()          # stratified in u1
        o, d = TO.rays(p, n, b1, b2, 1e-4)
        assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() < 1e-14
        assert (np.sum(d * n[:, None], 2) > 0).all()
        assert np.abs(o - (p + 1e-4 * n)[:, None]).max() == 0
    a1, _ = TO.sample_bits([5], 0, 32)
    c1, _ = TO.sample_bits([5], 1, 32)
    e1, _ = TO.sample_bits([6], 0, 32)
    assert not np.array_equal(a1, c1) and not np.array_equal(a1, e1)
    # the cosine-weighted estimator on the oracle's own samples: E[Y_k] over the hemisphere = the unoccluded transfer
    b1, b2 = TO.sample_bits(np.arange(7), 0, 4096)
    _, d = TO.rays(p, n, b1, b2, 0.0)
    rows = TO.transfer_rows(d, np.ones((7, 4096)), n)
    assert np.abs(rows[:, :9] - TO.unoccluded(n)).max() < 2e-3 and (rows[:, 9] == 1).all() and (rows[:, 13:] == 0).all()
    assert np.abs(rows[:, 10:13] - n).max() < 2e-3


def test_sphere_closed_form_and_icosphere_level():
    """AO under a sphere wholly above the horizon = 1 - (r/d)^2 cos(theta); the oracle's estimate on the transfer's own samples sits near
    it, and the icosphere level the GPU test uses differs from the analytic sphere in fewer than 1 % of the verdicts."""
    from nu_nerf_amd.lbvh import icosphere
    r, S = 0.3, 1024
    centre = np.asarray([0.0, 0.0, 0.35])                    # the hovering sphere of the GPU tests
    pts = np.asarray([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.3, -0.3, 0.0]])
    nrm = np.tile([0.0, 0.0, 1.0], (3, 1))
    b1, b2 = TO.sample_bits(np.arange(3), 0, S)
    o, d = TO.rays(pts, nrm, b1, b2, 1e-4)
    V, F = icosphere(3, r)
    tri = (V.astype(np.float64) + centre)[F.astype(np.int64)]
    for k in range(3):
        dist = np.linalg.norm(centre - pts[k])
        cos_t = centre[2] / dist
        assert dist * cos_t >= r
        occ = TO.sphere_occludes(o[k], d[k], centre, r)
        closed = 1.0 - (r / dist) ** 2 * cos_t
        mesh = TO.any_hit(tri, o[k], d[k])
        differ = float((mesh != occ).mean())
        print(f"sphere over vertex {k}: closed form {closed:.5f}, analytic sphere on the samples {1 - occ.mean():.5f}, "
              f"verdicts that differ on the 1 280-face icosphere {differ:.4f}")
        assert abs((1.0 - occ.mean()) - closed) < 0.01 and differ < 0.01


def test_command_arguments(tmp_path, monkeypatch):
    from nu_nerf_amd import bake_transfer as B
    from nu_nerf_amd import extract_environment as X
    from nu_nerf_amd import prefilter_environment as P
    from nu_nerf_amd import relight as R
    f = B.parse_args(['--mesh', 'a/pot.ply'])
    assert f.samples == 1024 and f.radius is None and f.seed == 0 and B.output_dir(f) == os.path.join('data', 'materials', 'pot')
    assert B.output_dir(B.parse_args(['--mesh', 'pot.ply', '--out', 'x'])) == 'x'
    for bad in (['--samples', '8'], ['--samples', '40'], ['--radius', '0'], ['--radius', '-1'], ['--radius', 'inf'], ['--eps', 'nan']):
        with pytest.raises(SystemExit):
            B.parse_args(['--mesh', 'pot.ply'] + bad)
    base = ['--mesh', 'm.ply', '--material', 'mat', '--name', 'n']
    ok = R.parse_args(base + ['--splitsum', '--hdr', 'e.hdr', '--transfer', 't'])
    assert ok.transfer == 't' and ok.occlusion is None
    assert R.parse_args(base + ['--splitsum', '--pyramid', 'p', '--transfer', 't', '--occlusion', 'sh']).occlusion == 'sh'
    assert R.parse_args(base + ['--hdr', 'e.hdr']).transfer is None
    for bad in (base + ['--hdr', 'e.hdr', '--transfer', 't'],                                   # without --splitsum
                ['--mesh', 'm.ply', '--name', 'n', '--hdr', 'e.hdr', '--inner', 'i.ply', '--inner-material', 'im', '--transfer', 't'],
                ['--mesh', 'm.ply', '--name', 'n', '--hdr', 'e.hdr', '--splitsum', '--inner', 'i.ply', '--inner-material', 'im', '--transfer', 't'],
                base + ['--splitsum', '--hdr', 'e.hdr', '--occlusion', 'ao'],                   # --occlusion without --transfer
                base + ['--splitsum', '--hdr', 'e.hdr', '--transfer', 't', '--occlusion', 'bent']):
        with pytest.raises(SystemExit):
            R.parse_args(bad)
    assert P.parse_args(['--hdr', 'e.hdr']).sh is False and P.parse_args(['--hdr', 'e.hdr', '--sh']).sh is True
    assert X.parse_args(['--cfg', 'c.yaml']).sh is False and X.parse_args(['--cfg', 'c.yaml', '--sh']).sh is True


def test_file_layout_round_trip(tmp_path):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import transfer as T
    from nu_nerf_amd.environment import project_sh
    g = np.random.Generator(np.random.PCG64(7))
    rows = g.normal(size=(11, 16)).astype(np.float32)
    rows[:, 13:] = 0
    paths = T.save_transfer_dir(str(tmp_path / 'm'), rows)
    assert sorted(os.listdir(tmp_path / 'm')) == ['ao.npy', 'bent_normal.npy', 'transfer.npy'] and sorted(paths) == sorted(T.FILES)
    assert np.load(paths['ao']).shape == (11, 1) and np.load(paths['bent_normal']).shape == (11, 3) and np.load(paths['transfer']).shape == (11, 9)
    assert all(np.load(p).dtype == np.float32 for p in paths.values())
    assert np.array_equal(T.load_transfer_dir(str(tmp_path / 'm')), rows) and np.array_equal(T.load_transfer_dir(str(tmp_path / 'm'), 11), rows)
    with pytest.raises(ValueError):
        T.load_transfer_dir(str(tmp_path / 'm'), 12)
    with pytest.raises(ValueError):
        T.join_rows(rows[:, :9], rows[:5, 9], rows[:, 10:13])
    with pytest.raises(ValueError):
        T.split_rows(rows[:, :9])
    packed = T.pack_env_sh(np.arange(27.0).reshape(9, 3))
    assert packed.shape == (9, 4) and packed.dtype == np.float32 and (packed[:, 3] == 0).all() and packed[2, 1] == 7
    with pytest.raises(ValueError):
        T.pack_env_sh(np.zeros((9, 4)))
    # the environment's SH of a pyramid directory: env_sh.npy, else env.npy, else the level of lowest roughness -- and which is said
    d = tmp_path / 'env'
    os.makedirs(d)
    pyr = g.random((2, 4, 8, 3)).astype(np.float32)
    np.save(d / 'env_pyramid.npy', pyr[::-1])
    np.save(d / 'roughness.npy', np.asarray([1.0, 0.0], np.float32))
    sh, src = R.load_env_sh(str(d))
    assert np.array_equal(sh, project_sh(pyr[0])) and 'env_pyramid.npy' in src and 'roughness 0' in src
    np.save(d / 'env.npy', pyr[1])
    sh, src = R.load_env_sh(str(d))
    assert np.array_equal(sh, project_sh(pyr[1])) and 'env.npy' in src
    np.save(d / 'env_sh.npy', np.arange(27.0).reshape(9, 3))
    sh, src = R.load_env_sh(str(d))
    assert np.array_equal(sh, np.arange(27.0).reshape(9, 3)) and src.endswith('env_sh.npy')


def test_header_declares_and_binds_the_new_entries():
    from nu_nerf_amd import _lib as L
    with open(os.path.join(ROOT, 'include', 'nu_nerf.h')) as fh:
        text = fh.read()
    names = ('nu_transfer_bake', 'nu_transfer_bake_dump', 'nu_transfer_rays', 'nu_relight_splitsum_occluded')
    sigs = {name: argtypes for name, _, argtypes in L._signatures()}
    for name in names:
        assert re.search(r'\bint ' + name + r'\(', text), name
        assert name in sigs
    assert len(sigs['nu_transfer_bake']) == 12 and len(sigs['nu_transfer_bake_dump']) == 13 and len(sigs['nu_transfer_rays']) == 10
    assert len(sigs['nu_relight_splitsum_occluded']) == len(sigs['nu_relight_splitsum']) + 6
    assert L.NU_OCC_AO == 0 and L.NU_OCC_SH == 1
    if os.path.exists(L.lib_path()):
        lib = L.load()
        for name in names:
            assert getattr(lib, name).argtypes == sigs[name]
