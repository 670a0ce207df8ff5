"""GPU closest point on a triangle mesh (nu_lbvh_closest / nu_brute_closest through LBVH.closest_points): face ids identical to
the numpy float32 oracle (tests/closest_point_oracle.py), d2 and the closest point the same float32 bits; the LBVH equal to the
device sweep on large meshes; an independent float64 distance; max_dist bounds; the analytic sphere."""
import numpy as np
import pytest
import torch

from closest_point_oracle import brute_force_closest, exact_d2, exact_min_d2, MISS_INDEX

pytestmark = pytest.mark.gpu


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _queries(V, F, n, seed, radius=0.5):
    """inside / outside / far points, exact vertices, exact points on edges, surface points offset by +-1e-5 along the normal."""
    g = np.random.Generator(np.random.PCG64(seed))
    k = n // 6
    inside = _unit(g.normal(size=(k, 3))) * g.uniform(0, 0.9 * radius, (k, 1))
    outside = _unit(g.normal(size=(k, 3))) * g.uniform(1.1 * radius, 2 * radius, (k, 1))
    far = _unit(g.normal(size=(k, 3))) * g.uniform(3, 10, (k, 1))
    verts = V[g.integers(0, len(V), k)]
    T = V[F[g.integers(0, len(F), k)]].astype(np.float32)
    e = g.integers(0, 3, k)
    a, b = T[np.arange(k), e], T[np.arange(k), (e + 1) % 3]
    edges = a + (b - a) * g.uniform(0, 1, (k, 1)).astype(np.float32)
    m = n - 5 * k
    T = V[F[g.integers(0, len(F), m)]].astype(np.float64)
    r1, r2 = np.sqrt(g.uniform(0, 1, (m, 1))), g.uniform(0, 1, (m, 1))
    s = T[:, 0] * (1 - r1) + T[:, 1] * (r1 * (1 - r2)) + T[:, 2] * (r1 * r2)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    surf = s + 1e-5 * nrm * g.choice([-1.0, 1.0], (m, 1))
    return np.concatenate([inside, outside, far, verts, edges, surf]).astype(np.float32)


def _soup(seed=3):
    """Random triangles + exact duplicates (d2 ties) + zero-area ones: collinear (axis-aligned and dyadic diagonal), two coincident
    vertices, single points, and near-degenerate slivers."""
    g = np.random.Generator(np.random.PCG64(seed))
    nf = 600
    tri = g.uniform(-0.5, 0.5, (nf, 1, 3)) + g.normal(size=(nf, 3, 3)) * 0.08
    dup = tri[:40]
    o = np.round(g.uniform(-0.5, 0.5, (40, 1, 3)) * 64) / 64
    d = np.round(g.uniform(-0.2, 0.2, (40, 1, 3)) * 64) / 64
    collinear_diag = np.concatenate([o, o + d, o + 2 * d], 1)
    ax = np.zeros((40, 3, 3))
    ax[:] = o
    ax[:, :, 0] += g.uniform(-0.3, 0.3, (40, 3))
    seg = tri[40:80].copy()
    seg[:, 1] = seg[:, 0]
    point = np.repeat(tri[80:120, :1], 3, 1)
    sliver = tri[120:160].copy()
    sliver[:, 2] = sliver[:, 0] + (sliver[:, 1] - sliver[:, 0]) * 0.37 + g.normal(size=(40, 3)) * 1e-7
    allt = np.concatenate([tri, dup, collinear_diag, ax, seg, point, sliver]).astype(np.float32)
    perm = g.permutation(len(allt))
    allt = allt[perm]
    return allt.reshape(-1, 3), np.arange(len(allt) * 3, dtype=np.int32).reshape(-1, 3)


def _meshes():
    from nu_nerf_amd.lbvh import icosphere
    out = {f"ico{s}": icosphere(s, 0.5) for s in (0, 2, 5)}
    out["soup"] = _soup()
    return out


MESHES = ["ico0", "ico2", "ico5", "soup"]


@pytest.fixture(scope="module")
def meshes():
    return _meshes()


def _bvh(V, F, gpu):
    from nu_nerf_amd.lbvh import LBVH
    return LBVH(torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu))


def _run(bvh, P, gpu, **kw):
    d2, idx, q = bvh.closest_points(torch.from_numpy(P).to(gpu), **kw)
    return d2.cpu().numpy(), idx.cpu().numpy(), q.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", MESHES)
def test_bit_exact_vs_oracle_and_float64(gpu, meshes, name):
    V, F = meshes[name]
    P = _queries(V, F, 8192, seed=len(F))
    d2, idx, q = _run(_bvh(V, F, gpu), P, gpu)
    od2, oidx, oq = brute_force_closest(V, F, P)
    assert np.array_equal(idx, oidx)
    assert _same_bits(d2, od2) and _same_bits(q, oq)
    assert np.isfinite(d2).all() and np.isfinite(q).all() and (idx != MISS_INDEX).all()
    # independent float64 distance (plane projection / clamped segments): the fp32 d2 within 1e-6 max(1, |p|^2), and a face other
    # than the float64 closest one only where the two tie within that tolerance
    tol = 1e-6 * np.maximum(1.0, np.sum(P.astype(np.float64) ** 2, 1))
    m = exact_min_d2(V, F, P)
    assert (np.abs(d2 - m) <= tol).all()
    assert (exact_d2(V, F, P, idx) - m <= tol).all()


def test_degenerate_triangles_are_finite(gpu):
    """Every zero-area kind alone (the soup mixes them with ordinary triangles): finite, and equal to the oracle."""
    V, F = _soup()
    T = V[F]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    deg = np.nonzero(np.einsum('ij,ij->i', n, n) == 0)[0]
    assert len(deg) >= 150
    Fd = F[deg]
    P = _queries(V, Fd, 4096, seed=11)
    d2, idx, q = _run(_bvh(V, Fd, gpu), P, gpu)
    od2, oidx, oq = brute_force_closest(V, Fd, P)
    assert np.isfinite(d2).all() and np.isfinite(q).all()
    assert np.array_equal(idx, oidx) and _same_bits(d2, od2) and _same_bits(q, oq)


@pytest.mark.parametrize("subdiv", [6, 7])
def test_lbvh_equals_device_brute_force(gpu, subdiv):
    """81 920 and 327 680 faces: the traversal never culls the closest face (the padded boxes are conservative)."""
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(subdiv, 0.5)
    bvh = _bvh(V, F, gpu)
    P = torch.from_numpy(_queries(V, F, 32768, seed=subdiv)).to(gpu)
    a = bvh.closest_points(P)
    b = bvh.closest_points_brute(P)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("max_dist", [0.0, 0.02, 0.3])
def test_max_dist_bound(gpu, meshes, max_dist):
    V, F = meshes["ico2"]
    P = _queries(V, F, 4096, seed=5)
    bvh = _bvh(V, F, gpu)
    d2, idx, q = _run(bvh, P, gpu)
    bd2, bidx, bq = _run(bvh, P, gpu, max_dist=max_dist)
    lim = np.float32(max_dist * max_dist)
    within = d2 <= lim
    assert 0 < within.sum() < len(P) or max_dist == 0.0
    assert np.array_equal(bidx[within], idx[within]) and _same_bits(bd2[within], d2[within]) and _same_bits(bq[within], q[within])
    assert (bidx[~within] == MISS_INDEX).all() and np.isposinf(bd2[~within]).all() and (bq[~within] == 0).all()
    for fn in ("closest_points_brute",):
        b2 = [x.cpu().numpy() for x in getattr(bvh, fn)(torch.from_numpy(P).to(gpu), max_dist=max_dist)]
        assert np.array_equal(b2[1], bidx) and _same_bits(b2[0], bd2) and _same_bits(b2[2], bq)
    od2, oidx, oq = brute_force_closest(V, F, P, max_d2=lim)
    assert np.array_equal(oidx, bidx) and _same_bits(od2, bd2) and _same_bits(oq, bq)


def test_empty_queries_single_face_and_errors(gpu):
    from nu_nerf_amd.lbvh import LBVH
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F = np.array([[0, 1, 2]], np.int32)
    bvh = _bvh(V, F, gpu)
    d2, idx, q = bvh.closest_points(torch.zeros(0, 3, device=gpu))
    assert d2.shape == (0,) and idx.shape == (0,) and q.shape == (0, 3)
    P = _queries(V, F, 2048, seed=1, radius=1.0)
    d2, idx, q = _run(bvh, P, gpu)
    od2, oidx, oq = brute_force_closest(V, F, P)
    assert (idx == 0).all() and np.array_equal(idx, oidx) and _same_bits(d2, od2) and _same_bits(q, oq)
    with pytest.raises(ValueError):
        LBVH(torch.from_numpy(V).to(gpu), torch.zeros(0, 3, dtype=torch.int32, device=gpu))
    bad = torch.tensor([[0.0, float('nan'), 0.0]], device=gpu)
    with pytest.raises(ValueError):
        bvh.closest_points(bad)
    with pytest.raises(ValueError):
        bvh.closest_points(torch.tensor([[float('inf'), 0.0, 0.0]], device=gpu))


def test_two_calls_same_bits(gpu, meshes):
    V, F = meshes["ico5"]
    bvh = _bvh(V, F, gpu)
    P = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (65536, 3)).astype(np.float32)).to(gpu)
    a, b = bvh.closest_points(P), bvh.closest_points(P)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_icosphere_distance_is_radial_within_the_sagitta(gpu):
    from nu_nerf_amd.lbvh import icosphere
    r = 0.5
    V, F = icosphere(4, r)
    T = V[F].astype(np.float64)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    inr = np.abs(np.einsum('ij,ij->i', nrm / np.linalg.norm(nrm, axis=1, keepdims=True), T[:, 0]))
    sag = r - inr.min()                                      # the mesh lies between the spheres r - sag and r
    g = np.random.default_rng(8)
    P = (_unit(g.normal(size=(20000, 3))) * g.uniform(0.0, 1.5, (20000, 1))).astype(np.float32)
    d2, _, q = _run(_bvh(V, F, gpu), P, gpu)
    d = np.sqrt(d2.astype(np.float64))
    rad = np.abs(np.linalg.norm(P.astype(np.float64), axis=1) - r)
    assert (np.abs(d - rad) <= sag + 1e-6).all()
    assert (np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - (r - sag / 2)) <= sag / 2 + 1e-6).all()


# ---- stage-2 mesh cleanup and mesh distances -----------------------------------------------------------------------------------

def _two_shell_inner():
    from nu_nerf_amd.lbvh import icosphere
    Vs, Fs = icosphere(2, 0.47)                              # on the outer shell: within 0.055 of the r = 0.5 mesh
    Vk, Fk = icosphere(2, 0.3)                               # kept
    return np.concatenate([Vs, Vk]), np.concatenate([Fs, Fk + len(Vs)]), Vk, Fk


def test_remove_faces_near_keeps_the_inner_component(gpu):
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import remove_faces_near
    Vo, Fo = icosphere(3, 0.5)
    Vi, Fi, Vk, Fk = _two_shell_inner()
    V, F = remove_faces_near(Vi, Fi, Vo, Fo, min_dist=0.055)
    assert V.dtype == np.float32 and F.dtype == np.int32
    assert np.array_equal(V, Vk) and np.array_equal(F, Fk)
    # a face survives only with all three vertices beyond the bound: a threshold above 0.3 - sag drops everything
    V0, F0 = remove_faces_near(Vi, Fi, Vo, Fo, min_dist=0.25)
    assert len(F0) == 0 and len(V0) == 0


def test_postprocess_cli(gpu, tmp_path):
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import write_ply, read_ply
    from nu_nerf_amd import postprocess_mesh
    Vo, Fo = icosphere(3, 0.5)
    Vi, Fi, Vk, Fk = _two_shell_inner()
    write_ply(tmp_path / "outer.ply", Vo, Fo)
    write_ply(tmp_path / "s2.ply", Vi, Fi)
    out = postprocess_mesh.main(["--inner", str(tmp_path / "s2.ply"), "--outer", str(tmp_path / "outer.ply")])
    assert out == str(tmp_path / "s2_cleaned.ply")
    V, F = read_ply(out)
    assert np.array_equal(V, Vk) and np.array_equal(F, Fk)
    out2 = postprocess_mesh.main(["--inner", str(tmp_path / "s2.ply"), "--outer", str(tmp_path / "outer.ply"), "--min-dist", "0.01",
                                  "--out", str(tmp_path / "all.ply")])
    V2, F2 = read_ply(out2)
    assert np.array_equal(V2, Vi) and np.array_equal(F2, Fi)


def test_sample_surface_is_deterministic_and_on_the_mesh(gpu):
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import sample_surface
    V, F = icosphere(3, 0.5)
    a = sample_surface(V, F, 50000, seed=3)
    b = sample_surface(V, F, 50000, seed=3)
    c = sample_surface(V, F, 50000, seed=4)
    assert a.shape == (50000, 3) and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b) and not torch.equal(a, c)
    d2, _, _ = _bvh(V, F, gpu).closest_points(a)
    assert float(d2.max()) < 1e-12
    # area-weighted: the octants of a sphere receive equal shares
    octant = ((a > 0).long() * torch.tensor([1, 2, 4], device=a.device)).sum(1)
    share = torch.bincount(octant, minlength=8).double() / len(a)
    assert float((share - 0.125).abs().max()) < 0.01


def test_mesh_distance(gpu):
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import mesh_distance
    A = icosphere(5, 0.5)
    B = icosphere(5, 0.4)
    same = mesh_distance(A, A, n_samples=100000, seed=1)
    assert same['chamfer'] < 1e-6 and same['hausdorff'] < 1e-5
    r = mesh_distance(A, B, n_samples=200000, seed=2)
    for k in ('a_to_b_mean', 'b_to_a_mean', 'chamfer', 'a_to_b_max', 'b_to_a_max', 'hausdorff'):
        assert abs(r[k] - 0.1) < 1e-3, (k, r[k])
    s = mesh_distance(B, A, n_samples=200000, seed=2)
    assert s['a_to_b_mean'] == r['b_to_a_mean'] and s['b_to_a_mean'] == r['a_to_b_mean'] and s['chamfer'] == r['chamfer']
    assert s['hausdorff'] == r['hausdorff'] and s['a_to_b_max'] == r['b_to_a_max']
    assert mesh_distance(A, B, n_samples=200000, seed=2) == r


def test_mesh_distance_cli(gpu, tmp_path, capsys):
    import json
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import write_ply, mesh_distance
    from nu_nerf_amd import mesh_distance as cli
    A, B = icosphere(3, 0.5), icosphere(3, 0.45)
    write_ply(tmp_path / "a.ply", *A)
    write_ply(tmp_path / "b.ply", *B)
    cli.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--samples", "20000", "--seed", "7"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res == mesh_distance(A, B, n_samples=20000, seed=7)
