"""Host-side checks of the nested-object relighting, no GPU: the float64 oracle against physics (Snell's law, reciprocity
of a crossing, no total internal reflection on a straight pass through a sphere), how many pixels of the GPU tests' scenes sit within
1e-4 of the refract / reflect threshold, --ior parsing, the unchanged old command line, the ior.npy round trip."""
import numpy as np
import pytest

import nested_relight_oracle as NO
import relight_oracle as O


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _random_events(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    ns = _unit(g.normal(size=(n, 3)))
    d = _unit(g.normal(size=(n, 3)))
    return d, ns, g.uniform(1.05, 1.9, n)


def test_oracle_refraction_obeys_snells_law():
    d, ns, ior = _random_events(4000, 1)
    for entering in (True, False):
        ev = NO.interface(d, ns, ior, entering)
        r = ev['refr']
        assert r.any() and (entering or (~r).any())
        n, dn = ev['n'][r], ev['dn'][r]
        assert (np.sum(ev['n'] * d, 1) <= 0).all() and np.abs(np.linalg.norm(dn, axis=1) - 1).max() < 1e-12
        sin_i = np.linalg.norm(np.cross(n, d[r]), axis=1)
        sin_t = np.linalg.norm(np.cross(n, dn), axis=1)
        n1, n2 = (1.0, ior[r]) if entering else (ior[r], 1.0)
        assert np.abs(n1 * sin_i - n2 * sin_t).max() < 1e-12 and (np.sum(dn * n, 1) < 0).all()
        # coplanar with d and n
        assert np.abs(np.sum(np.cross(n, d[r]) * dn, 1)).max() < 1e-12
        # total internal reflection mirrors, with all the energy
        m = ev['dn'][~r]
        assert np.allclose(np.sum(m * ev['n'][~r], 1), -np.sum(d[~r] * ev['n'][~r], 1)) and (ev['F'][~r] == 1).all()
        assert ((ev['k2'] > 0.999) == ~r).all()
    assert NO.interface(d, ns, ior, True)['refr'].all()            # entering a denser medium always refracts (ior >= 1.05 here)


def test_oracle_crossing_is_reciprocal():
    d, ns, ior = _random_events(4000, 2)
    d, ns, ior = (v[1.0 - np.sum(ns * d, 1) ** 2 < 0.998] for v in (d, ns, ior))      # (the 0.999 rule cuts the grazing way back off)
    a = NO.interface(d, ns, ior, True)
    b = NO.interface(-a['dn'], ns, ior, False)                     # the same path walked backwards
    assert len(ior) > 3000 and b['refr'].all()
    assert np.abs(b['dn'] + d).max() < 1e-9 and np.abs(a['F'] - b['F']).max() < 1e-12
    f0 = ((ior - 1) / (ior + 1)) ** 2
    assert (a['F'] >= f0 - 1e-15).all() and (a['F'] <= 1).all()
    head_on = NO.interface(-ns, ns, ior, True)
    assert np.abs(head_on['F'] - f0).max() < 1e-15 and np.abs(head_on['dn'] + ns).max() < 1e-12
    matched = NO.interface(d, ns, np.ones_like(ior), True)         # an index-matched interface: straight on, nothing reflected
    ok = matched['refr']
    assert ok.mean() > 0.9 and np.abs(matched['dn'][ok] - d[ok]).max() < 1e-12 and not matched['F'].any()


def test_straight_pass_through_an_exact_sphere_never_reflects_totally():
    g = np.random.Generator(np.random.PCG64(3))
    n = 4000
    p = _unit(g.normal(size=(n, 3)))                               # entry point on the unit sphere; its normal
    d = _unit(g.normal(size=(n, 3)))
    d = np.where((np.sum(d * p, 1) > 0)[:, None], -d, d)
    ior = g.uniform(1.0, 2.0, n)
    a = NO.interface(d, p, ior, True)
    # physically the chord always leaves; the trained rule calls eta^2 sin^2 > 0.999 total reflection, which on the way out is the entry's
    # own sin^2_i -- so: every ray whose entry is clear of that cut
    ok = a['refr'] & (1.0 - a['cos_i'] ** 2 < 0.999 - 1e-9)
    assert ok.mean() > 0.95
    q = p[ok] - 2.0 * np.sum(p[ok] * a['dn'][ok], 1, keepdims=True) * a['dn'][ok]          # where the chord leaves the sphere
    b = NO.interface(a['dn'][ok], q, ior[ok], False)
    assert b['refr'].all() and np.abs(b['k2'] - (1 - a['cos_i'][ok] ** 2)).max() < 1e-9     # leaves at the angle it came in with
    assert np.abs(b['F'] - a['F'][ok]).max() < 1e-9


@pytest.mark.parametrize("name", ['ico2', 'ico3', 'box'])
def test_share_of_pixels_near_the_threshold_stays_under_the_cap(name):
    """The cap of the GPU comparison (2 % of the hit pixels within 1e-4 of eta^2 sin^2 = 0.999), confirmed with the oracle alone."""
    from nu_nerf_amd import relight as R
    from test_relight_nested_gpu import MARGIN, MARGIN_CAP, SCENES, _meshes, _poses
    h, w = SCENES[name]
    Vo, Fo, ior, Vi, Fi, _ = _meshes(name)
    Vo, Vi, Fo, Fi = Vo.astype(np.float64), Vi.astype(np.float64), Fo.astype(np.int64), Fi.astype(np.int64)
    VNo, VNi = O.vertex_normals(Vo, Fo), O.vertex_normals(Vi, Fi)
    o, d = O.pinhole_rays(R.intrinsics(h, w), _poses(name)[0], h, w)
    hit, f, _ = O.brute_trace(Vo, Fo, o, d)
    p = np.flatnonzero(hit)
    mat = np.zeros((len(Vo), 5))
    mat[:, 0] = ior - 1.0
    rows = O.gbuffer_rows(Vo, Fo, VNo, mat, o[p], d[p], f[p], 0, p)
    c = NO.chain((Vo, Fo, VNo), (Vi, Fi, VNi), ior.astype(np.float64), rows, R.ORIGIN_EPS)
    share = (c['margin'] <= MARGIN).mean()
    kinds = [int((c['kind'] == k).sum()) for k in (NO.DARK, NO.INNER, NO.EXIT)]
    print(f"{name}: {len(p)} hit pixels, dark / inner / exit {kinds}, {share:.2%} within {MARGIN} of the threshold")
    assert len(p) > 100 and kinds[1] > 10 and kinds[2] > 50 and share <= MARGIN_CAP
    assert (c['T'][c['kind'] != NO.DARK] > 0).all() and (c['T'] <= 1).all()
    if name == 'box':                                              # rays that enter the top and meet a side face are totally reflected
        assert ((c['kind'] == NO.DARK).sum() + (c['T'] > 0).sum()) == len(p)


def test_ior_option_parsing(tmp_path):
    from nu_nerf_amd import relight as R
    assert R.parse_ior('1.5') == 1.5 and R.parse_ior('1') == 1.0 and isinstance(R.parse_ior('2'), float)
    assert R.parse_ior('some/dir') == 'some/dir/ior.npy'
    for bad in ('0.9', '-2', 'nan', 'inf'):
        with pytest.raises(ValueError):
            R.parse_ior(bad)
    assert np.array_equal(R.load_ior(1.25, 4), np.full(4, 1.25, np.float32))
    base = ['--mesh', 'o.ply', '--hdr', 'e.hdr', '--name', 'n']
    f = R.parse_args(base + ['--inner', 'i.ply', '--inner-material', 'm'])
    assert f.inner == 'i.ply' and f.inner_material == 'm' and f.ior == '1.5' and f.material is None
    assert R.parse_args(base + ['--inner', 'i.ply', '--inner-material', 'm', '--ior', 'dir']).ior == 'dir'
    for argv in (base + ['--inner', 'i.ply'], base + ['--inner', 'i.ply', '--inner-material', 'm', '--ior', '0.5'],
                 base + ['--material', 'm', '--inner-material', 'm'], base):
        with pytest.raises(SystemExit):
            R.parse_args(argv)


def test_old_command_line_is_unchanged_without_inner(capsys):
    from nu_nerf_amd import relight as R
    f = R.parse_args(['--mesh', 'a.ply', '--material', 'mat', '--hdr', 'e.hdr', '--name', 'x', '--trans', '--num', '5'])
    assert (f.mesh, f.material, f.hdr, f.name, f.trans, f.num, f.inner) == ('a.ply', 'mat', 'e.hdr', 'x', True, 5, None)
    assert (f.width, f.height, f.samples, f.cam_dist, f.azimuth, f.elevation, f.seed, f.chunk) == (800, 800, 1024, 3.0, 0.0, 45.0, 0, 256)
    with pytest.raises(SystemExit):
        R.parse_args(['--mesh', 'a.ply', '--hdr', 'e.hdr', '--name', 'x'])
    assert 'the following arguments are required: --material' in capsys.readouterr().err


def test_ior_file_round_trip(tmp_path):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.extract_materials import save_ior
    ior = np.linspace(1.1, 1.9, 7).astype(np.float32)
    path = save_ior(str(tmp_path), ior)
    assert path == str(tmp_path / 'ior.npy') and np.load(path).shape == (7, 1) and np.load(path).dtype == np.float32
    assert np.array_equal(R.load_ior(R.parse_ior(str(tmp_path)), 7), ior)
    with pytest.raises(ValueError):
        R.load_ior(R.parse_ior(str(tmp_path)), 8)
