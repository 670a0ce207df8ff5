"""Host-side checks of the thin-shell relighting, no GPU: the float64 oracle's crossing against
oracle/stage2_oracle.shell_refraction, its Fresnel factors, how many rows / pixels of the GPU tests sit within 1e-4 of a branch point,
the scenes' path statistics (with hits at negative curvature on the torus), argument validation of ThinShellScene and --shell, the
shell files' round trip."""
import numpy as np
import pytest

import relight_oracle as O
import thin_relight_oracle as TO
from thin_relight_oracle import MARGIN, MARGIN_CAP, N_FLAT, N_ROWS, SCENES
from thin_relight_oracle import meshes as _meshes, poses as _poses


@pytest.mark.parametrize("inside", [False, True])
def test_oracle_crossing_is_shell_refraction(inside):
    rows = [a.astype(np.float64) for a in TO.random_rows(N_ROWS + N_FLAT, inside, 21 + int(inside), flat=N_FLAT)]
    a, b = TO.cross(*rows, inside), TO.cross_ref(*rows, inside)
    assert np.array_equal(a['refracts'], b['refracts']) and np.array_equal(a['tir_ok'], b['tir_ok'])
    err = max(np.abs(a[k] - b[k]).max() for k in ('normal', 'end', 'next_start', 'next_dir'))
    first, every = (a['margin1'] <= MARGIN).mean(), (a['margin'] <= MARGIN).mean()
    print(f"{'leaving' if inside else 'entering'}: oracle vs shell_refraction {err:.3e}; refracts {a['refracts'].mean():.1%}, tir_ok "
          f"{a['tir_ok'].mean():.1%}; within {MARGIN} of a branch point: first face {first:.3%}, any face {every:.3%}")
    assert err < 1e-12 and every <= MARGIN_CAP and first <= every
    assert 0.5 < a['refracts'].mean() < 0.95 and (a['refracts'] & ~a['tir_ok']).sum() > 50
    r = a['refracts']
    assert np.abs(np.linalg.norm(a['next_dir'][r], axis=1) - 1).max() < 2e-4          # x / (|x| + 1e-4)
    if not inside:                                                                  # the logits give back the baked index: eta = 1 / n_g
        assert np.abs(1.0 / rows[3] - b['eta']).max() < 1e-12


def test_oracle_fresnel_factors():
    g = np.random.Generator(np.random.PCG64(9))
    n1, n2 = g.uniform(0.6, 1.7, 5000), g.uniform(0.6, 1.7, 5000)
    c1, c2 = g.uniform(-0.2, 1.0, 5000), g.uniform(-0.2, 1.0, 5000)
    F = TO.schlick(n1, n2, c1, c2)
    assert (F >= 0).all() and (F <= 1).all()
    assert np.array_equal(F, TO.schlick(n2, n1, c2, c1))                           # a face transmits the same both ways
    f0 = ((n1 - n2) / (n1 + n2)) ** 2
    assert np.allclose(TO.schlick(n1, n2, np.ones(5000), np.ones(5000)), f0) and (F >= f0 - 1e-15).all()
    assert not TO.schlick(n1, n1, c1, c2).any()                                    # index-matched: nothing reflected
    low = np.where(n1 <= n2, c1, c2)
    assert np.allclose(F, f0 + (1 - f0) * np.clip(1 - low, 0, 1) ** 5)
    for inside in (False, True):
        ev = TO.cross(*TO.random_rows(2000, inside, 5), inside)
        for k in ('F_a', 'F_b', 'keep'):
            assert (ev[k] >= 0).all() and (ev[k] <= 1).all()
        lost = ~ev['refracts']
        assert lost.any() and (ev['F_a'][lost] == 1).all() and not ev['F_b'][lost].any() and not ev['keep'][lost].any()
        assert np.allclose(ev['keep'], (1 - ev['F_a']) * (1 - ev['F_b']))


def test_crossing_a_sphere_wall_follows_snell_twice():
    """On an exact sphere the two concentric spheres are the geometry: the direction in the cavity obeys Snell's law air -> cavity at the
    second face's normal, and the ray has moved sideways by less than the wall's thickness over the cosines."""
    g = np.random.Generator(np.random.PCG64(4))
    n = 3000
    p = g.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where((np.sum(d * p, 1) > 0)[:, None], -d, d)
    keep = -np.sum(d * p, 1) > 0.3
    p, d = p[keep], d[keep]
    m = len(p)
    ev = TO.cross(d, p, 0.5 * p, np.full(m, 1.5), np.full(m, 0.01), np.full(m, 4.0), False)     # radius 0.5: curvature 4
    assert ev['refracts'].all() and ev['tir_ok'].all()
    q = ev['next_start']
    rad = np.linalg.norm(q, axis=1)
    assert (rad < 0.5 - 0.01 + 1e-9).all() and (rad > 0.5 - 0.01 - 0.0011).all()      # 0.001 past the inner sphere
    nq = q / rad[:, None]
    sin_air = np.linalg.norm(np.cross(p, d), axis=1) * 0.5                              # n sin(theta) r is conserved through concentric spheres
    sin_cav = np.linalg.norm(np.cross(nq, ev['next_dir']), axis=1) * rad * TO.CAVITY
    assert np.abs(sin_air - sin_cav).max() < 2e-3                                       # (the 0.001 step and the 1e-4 normalisations)


@pytest.mark.parametrize("name", ['ico2', 'ico3', 'torus'])
def test_scene_paths_and_share_near_a_branch_point(name):
    """What the GPU tests rely on, confirmed with the oracle alone: every kind of path occurs, at most 2 % of the hit pixels decide within
    1e-4 of a branch point, and the torus has crossings at negative curvature both entering and leaving."""
    import torch
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.lbvh import vertex_normals_and_curvature
    h, w = SCENES[name]
    Vo, Fo, ior, th, Vi, Fi, _ = _meshes(name)
    gk = vertex_normals_and_curvature(torch.from_numpy(Vo), torch.from_numpy(np.asarray(Fo)).long())[1].clamp(-10, 10).numpy().reshape(-1)
    Vo, Vi, Fo, Fi = Vo.astype(np.float64), Vi.astype(np.float64), np.asarray(Fo).astype(np.int64), np.asarray(Fi).astype(np.int64)
    VNo, VNi = O.vertex_normals(Vo, Fo), O.vertex_normals(Vi, Fi)
    o, d = O.pinhole_rays(R.intrinsics(h, w), _poses(name)[0], h, w)
    hit, f, _ = O.brute_trace(Vo, Fo, o, d)
    p = np.flatnonzero(hit)
    mat = np.zeros((len(Vo), 5))
    mat[:, 0], mat[:, 1], mat[:, 2] = ior - 1.0, th, gk
    rows = O.gbuffer_rows(Vo, Fo, VNo, mat, o[p], d[p], f[p], 0, p)
    c = TO.chain((Vo, Fo, VNo), (Vi, Fi, VNi), ior.astype(np.float64), th.astype(np.float64), gk.astype(np.float64), rows, R.ORIGIN_EPS)
    share = (c['margin'] <= MARGIN).mean()
    kinds = [int((c['kind'] == k).sum()) for k in (TO.DARK, TO.INNER, TO.EXIT)]
    neg = int((rows[:, 12] < 0).sum())
    print(f"{name}: {len(p)} hit pixels, dark / inner / exit {kinds}, {share:.2%} within {MARGIN} of a branch point, curvature at the primary hits "
          f"{rows[:, 12].min():.2f} .. {rows[:, 12].max():.2f} ({neg} negative)")
    assert len(p) > 100 and kinds[0] > 10 and kinds[1] > 10 and kinds[2] > 50 and share <= MARGIN_CAP
    assert (c['T'][c['kind'] != TO.DARK] > 0).all() and (c['T'] + c['F'] <= 1 + 1e-12).all()
    if name == 'torus':
        assert neg > 50 and (rows[:, 12] > 0).sum() > 50
    else:
        assert np.abs(gk - 4.0).max() < 0.7                                           # a sphere of radius 0.5


def test_thin_shell_scene_validates_its_arguments():
    from nu_nerf_amd import relight as R
    Vo, Fo, ior, th, Vi, Fi, mat = _meshes('ico2')
    for bad_ior in (0.0, -1.0, np.nan, np.inf, ior[:-1], np.where(np.arange(len(ior)) == 3, 0.0, ior)):
        with pytest.raises(ValueError, match="ior"):
            R.ThinShellScene(Vo, Fo, bad_ior, th, Vi, Fi, mat, device='cpu')
    for bad_th in (-1e-3, np.nan, np.inf, th[:-1], np.where(np.arange(len(th)) == 3, -1e-6, th)):
        with pytest.raises(ValueError, match="thickness"):
            R.ThinShellScene(Vo, Fo, ior, bad_th, Vi, Fi, mat, device='cpu')
    for bad_gk in (np.nan, np.zeros(len(Vo) + 1)):
        with pytest.raises(ValueError, match="curvature"):
            R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, curvature=bad_gk, device='cpu')


def test_shell_option_parsing(tmp_path):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.extract_materials import save_shell
    assert R.parse_shell('1.45,0.005') == (1.45, 0.005) and R.parse_shell('0.7,0') == (0.7, 0.0)
    assert R.parse_shell('some/dir') == ('some/dir/shell_ior.npy', 'some/dir/shell_thickness.npy')
    for bad in ('1.4', '1.4,0.01,3', '0,0.01', '-1,0.01', '1.4,-0.01', 'nan,0.01', '1.4,inf'):
        with pytest.raises(ValueError):
            R.parse_shell(bad)
    base = ['--mesh', 'o.ply', '--hdr', 'e.hdr', '--name', 'n']
    f = R.parse_args(base + ['--inner', 'i.ply', '--inner-material', 'm', '--shell', '1.4,0.01'])
    assert f.shell == '1.4,0.01' and f.inner == 'i.ply' and f.material is None
    assert R.parse_args(base + ['--inner', 'i.ply', '--inner-material', 'm', '--shell', 'dir']).shell == 'dir'
    f = R.parse_args(base + ['--inner', 'i.ply', '--inner-material', 'm'])                  # without it: as before
    assert f.shell is None and f.ior == '1.5'
    for argv in (base + ['--inner', 'i.ply', '--inner-material', 'm', '--shell', '1.4,0.01', '--ior', '1.5'],
                 base + ['--inner', 'i.ply', '--inner-material', 'm', '--shell', '1.4'],
                 base + ['--inner', 'i.ply', '--inner-material', 'm', '--shell', '0,0.01'],
                 base + ['--material', 'm', '--shell', '1.4,0.01']):
        with pytest.raises(SystemExit):
            R.parse_args(argv)
    ior, th = np.linspace(0.7, 1.6, 7).astype(np.float32), np.linspace(0.002, 0.01, 7).astype(np.float32)
    paths = save_shell(str(tmp_path), {'ior': ior, 'thickness': th})
    assert paths == [str(tmp_path / 'shell_ior.npy'), str(tmp_path / 'shell_thickness.npy')]
    assert all(np.load(p).shape == (7, 1) and np.load(p).dtype == np.float32 for p in paths)
    a, b = R.load_shell(R.parse_shell(str(tmp_path)), 7)
    assert np.array_equal(a, ior) and np.array_equal(b, th)
    with pytest.raises(ValueError):
        R.load_shell(R.parse_shell(str(tmp_path)), 8)
    a, b = R.load_shell(R.parse_shell('1.45,0.005'), 3)
    assert np.array_equal(a, np.full(3, 1.45, np.float32)) and np.array_equal(b, np.full(3, 0.005, np.float32))


def test_predict_shell_refuses_what_is_not_the_thick_model():
    from nu_nerf_amd import materials as M
    with pytest.raises(ValueError, match="non-zero-thickness"):
        M.predict_shell(object(), None)
