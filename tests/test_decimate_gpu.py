"""Quadric-error decimation on the GPU (nu_nerf_amd.decimate, csrc/decimate.hip): every stage of a round and a full run against the
float64 port bit for bit, the properties of full runs (budget window, topology, valences, boundaries, determinism, the surface
bound), the refusals, adaptivity against remesh_isotropic, and what comes after it (LBVH, texture baking, glTF, extract_mesh)."""
import json
import os

import numpy as np
import pytest
import torch

import decimate_oracle as D
from test_decimate_host import boundary_vertices, on_cube_surface, open_grid, oracle_runs, unit_cube, volume
from test_mesh_host import directed_edge_defects
from test_remesh_gpu import _dev, _golden_mc, _run
from test_remesh_host import perturbed_icosphere, euler

pytestmark = pytest.mark.gpu
MIN_Q2 = 0.1 * 0.1


def _meshes():
    return {"icosphere": perturbed_icosphere(3, 0.2, seed=1), "golden24": _golden_mc()}


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", ["icosphere", "golden24"])
def test_round_matches_the_port_bit_for_bit(gpu, name):
    """Quadrics, per-edge cost / position / rejection, keys, threshold, winners and the applied mesh of one round.  sqrt and divide in
    float64 on the device are the IEEE correctly rounded ones: the quadrics -- the only place they enter -- match numpy's bits."""
    from nu_nerf_amd import decimate as M
    from nu_nerf_amd.remesh import compact
    V, F = _meshes()[name]
    Vt, Ft = compact(*_dev(V, F, gpu))
    Vc, Fc = _np(Vt), _np(Ft)
    floor = D.cost_floor(V)
    need = 40                                               # below the candidate count: the threshold cuts
    want = D.one_round(Vc, Fc, need, floor, MIN_Q2)
    rnd = M.Round(Vt, Ft, MIN_Q2)
    assert _np(rnd.Q).tobytes() == want['Q'].tobytes()
    assert np.array_equal(_np(rnd.npts), want['npts']) and 0 < want['ncand'] < len(want['npts']) and int(rnd.ncand) == want['ncand']
    assert _np(rnd.cost).tobytes() == want['cost'].tobytes() and _np(rnd.pos).tobytes() == want['pos'].tobytes()
    assert np.array_equal(_np(rnd.keys(floor)), want['ckey'])
    assert int(rnd.threshold(need)) == want['thr'] and int((want['ckey'] <= want['thr']).sum()) == need
    win = _np(rnd.winners())
    assert np.array_equal(win, want['win']) and 1 <= int(win.sum()) <= need
    rnd.apply()
    assert _np(Vt).tobytes() == want['V'].tobytes() and np.array_equal(_np(Ft), want['F'])
    print(f"{name}: {len(Fc)} faces, {want['ncand']} candidates, {int(win.sum())} winners of {need} competitors")


def test_full_run_matches_the_port_bit_for_bit(gpu):
    from nu_nerf_amd.mesh import decimate
    V, F = _meshes()["icosphere"]
    so, sg = {}, {}
    Vo, Fo = D.decimate(V, F, 320, stats=so)
    Vg, Fg = decimate(V, F, 320, stats=sg)
    assert Vg.tobytes() == Vo.tobytes() and np.array_equal(Fg, Fo)
    assert sg['per_round'] == so['per_round'] and sg['rounds'] == so['rounds'] and sg['max_cost'] == so['max_cost']
    print(f"icosphere 1280 -> {len(Fg)} faces in {sg['rounds']} rounds, winners / candidates "
          f"{sum(r[2] for r in sg['per_round']) / sum(r[1] for r in sg['per_round']):.4f}")


def _area2(V, F):
    W = V.astype(np.float64)
    return np.linalg.norm(np.cross(W[F[:, 1]] - W[F[:, 0]], W[F[:, 2]] - W[F[:, 0]]), axis=1)


def _euler(F):
    """V - E + F from the faces alone (open meshes too)."""
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return len(np.unique(F)) - len(np.unique(e, axis=0)) + len(F)


# The 24^3 golden mesh is cut by its grid's box: 228 boundary half-edges, whose vertices are locked.  It converges to a budget its
# interior can reach (1200) and is checked as what it is: the boundary kept bit for bit, the Euler characteristic kept.
CONVERGING = [("icosphere", 320), ("icosphere", 100), ("golden24", 1200), ("cube", 100), ("cube", 12)]


@pytest.fixture(scope="module")
def full_runs(gpu):
    from nu_nerf_amd.mesh import decimate
    meshes = dict(_meshes(), cube=unit_cube(), grid=open_grid())
    out = {}
    for name, target in CONVERGING + [("grid", 64)]:
        V, F = meshes[name]
        stats = {}
        Vd, Fd = decimate(V, F, target, stats=stats)
        out[name, target] = (V, F, Vd, Fd, stats)
    return out


@pytest.mark.parametrize("name,target", CONVERGING)
def test_converged_runs_end_inside_the_budget_window(full_runs, name, target):
    V, F, Vd, Fd, stats = full_runs[name, target]
    print(f"{name}: {len(F)} -> {len(Fd)} faces (target {target}) in {stats['rounds']} rounds, max cost {stats['max_cost']:.3e}")
    assert Vd.dtype == np.float32 and Fd.dtype == np.int32
    assert (directed_edge_defects(F) == 0) == (name != "golden24")
    assert stats['converged'] and stats['faces_in'] == len(F) and stats['faces_out'] == len(Fd)
    assert target <= len(Fd) <= int(np.ceil(1.02 * target))
    assert directed_edge_defects(Fd) == directed_edge_defects(F) and len(np.unique(Fd)) == len(Vd) and _euler(Fd) == _euler(F)
    assert boundary_vertices(Vd, Fd) == boundary_vertices(V, F)
    if name != "golden24":
        assert euler(Vd, Fd) == 2
    assert (_area2(Vd, Fd) > 0).all()
    interior = np.ones(len(Vd), bool)
    interior[np.nonzero(D.Tables(Vd, Fd).vbound)[0]] = False
    assert int(np.bincount(Fd.reshape(-1), minlength=len(Vd))[interior].min()) >= 3      # the check on the hold set
    assert volume(Vd, Fd) * volume(V, F) > 0                # the input's orientation


def test_cube_and_grid_equal_the_host_runs(full_runs):
    ref = oracle_runs()
    for key, name in ((("cube", 100), "cube100"), (("cube", 12), "cube12"), (("grid", 64), "grid64")):
        _, _, Vd, Fd, stats = full_runs[key]
        Vo, Fo, so = ref[name]
        assert Vd.tobytes() == Vo.tobytes() and np.array_equal(Fd, Fo), name
        assert stats['per_round'] == so['per_round'] and stats['converged'] == so['converged']
    for target in (100, 12):
        _, _, Vd, Fd, _ = full_runs["cube", target]
        assert on_cube_surface(Vd) and volume(Vd, Fd) == 1.0


def test_open_meshes_keep_their_boundary(gpu, full_runs):
    from nu_nerf_amd.mesh import decimate
    V, F, Vd, Fd, stats = full_runs["grid", 64]
    assert stats['converged'] is False and 64 < len(Fd) < len(F)
    assert (Vd[:, 2] == 0).all() and (_area2(Vd, Fd) > 0).all()
    assert boundary_vertices(Vd, Fd) == boundary_vertices(V, F) and len(boundary_vertices(V, F)) == 64
    V, F = perturbed_icosphere(3, 0.2, seed=1)
    Fo = F[V[F].mean(1)[:, 2] < 0.3]                        # a cap cut off: one boundary loop
    used = np.unique(Fo)
    remap = np.full(len(V), -1)
    remap[used] = np.arange(len(used))
    Vo, Fo = V[used], remap[Fo].astype(np.int32)
    b0 = boundary_vertices(Vo, Fo)
    assert len(b0) > 10
    Vd, Fd = decimate(Vo, Fo, 300)
    assert boundary_vertices(Vd, Fd) == b0 and 300 <= len(Fd) <= 306


def test_two_calls_same_bits_and_torch_in_torch_out(gpu):
    from nu_nerf_amd.mesh import decimate
    V, F = _meshes()["golden24"]
    a = decimate(*_dev(V, F, gpu), 1200)
    b = decimate(*_dev(V, F, gpu), 1200)
    assert a[0].is_cuda and a[0].dtype == torch.float32 and a[1].dtype == torch.int32
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    c = decimate(V, F, 1200)
    assert isinstance(c[0], np.ndarray) and c[0].tobytes() == _np(a[0]).tobytes() and np.array_equal(c[1], _np(a[1]))


def _checked_points(V, F):
    """The points the bound is enforced at, in the kernels' fp32 arithmetic: every vertex, then per face the centroid ((a + b) + c) / 3
    and the edge midpoints (a + b) / 2, (b + c) / 2, (c + a) / 2."""
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    h = np.float32(0.5)
    return np.concatenate([V, ((a + b) + c) / np.float32(3), (a + b) * h, (b + c) * h, (c + a) * h]).astype(np.float32)


@pytest.mark.parametrize("pct", [1.0, 2.5])
def test_surface_bound_holds(gpu, pct):
    """With max_surf_dist every point of the output lies within the bound of the input: the one-sided distance of mesh_distance
    (200 000 surface samples of the output) stays within it, and so do the queried points themselves.  The input's relief (vertices
    moved by up to 0.2 edge lengths, about 0.7 % of the diagonal) is of the size of the tighter bound, and a 100-face output would
    have faces a dozen input faces wide: the case seven points per face cannot see unless each is allowed only the bound minus the
    face's covering radius.  That allowance caps the edge length at sqrt(12) x bound, so both runs stop above the budget the
    unbounded run reaches.  Measured on an MI355X: 1 % (1.76e-2) -- nothing can be certified (the input's own edges are longer than
    the cap) and the input comes back; 2.5 % (4.40e-2) -- 854 faces, sampled distance 1.2e-2; the unbounded run: 102 faces, 2.9e-2."""
    from nu_nerf_amd.lbvh import LBVH
    from nu_nerf_amd.mesh import decimate, mesh_distance
    V, F = _meshes()["icosphere"]
    bound = pct / 100.0 * float(np.linalg.norm(V.max(0).astype(np.float64) - V.min(0).astype(np.float64)))
    bvh = LBVH(*_dev(V, F, gpu))
    free = decimate(V, F, 100)
    stats = {}
    Vd, Fd = decimate(V, F, 100, max_surf_dist=bound, stats=stats)
    worst = float(bvh.closest_points(torch.from_numpy(_checked_points(Vd, Fd)).to(gpu))[0].max())
    sampled = mesh_distance((Vd, Fd), (V, F), n_samples=200_000)['a_to_b_max']
    sampled_free = mesh_distance(free, (V, F), n_samples=200_000)['a_to_b_max']
    edge = float(np.linalg.norm(Vd[Fd] - Vd[np.roll(Fd, -1, 1)], axis=2).max())
    edge_in = float(np.linalg.norm(V[F] - V[np.roll(F, -1, 1)], axis=2).max())
    print(f"bound {bound:.4e}: sampled one-sided distance {sampled:.4e} (unbounded run {sampled_free:.4e}, {len(free[1])} faces); "
          f"worst squared distance at the queried points {worst:.4e} against {bound * bound:.4e}; {len(Fd)} faces, longest edge "
          f"{edge:.4e}, converged {stats['converged']}, {stats['rounds']} rounds")
    assert sampled <= bound
    assert worst <= float(np.float32(bound * bound))
    assert edge <= max(np.sqrt(12.0) * bound, edge_in)
    assert len(free[1]) < len(Fd) <= len(F) and (pct < 2.5 or len(Fd) < len(F))          # the bound binds; the looser one still decimates
    assert directed_edge_defects(Fd) == 0


def test_refusals_and_identity(gpu):
    from nu_nerf_amd.lbvh import EmptyMeshError
    from nu_nerf_amd.mesh import decimate
    V, F = perturbed_icosphere()
    with pytest.raises(EmptyMeshError):
        decimate(V, F[:0], 100)
    with pytest.raises(ValueError):
        decimate(V, np.array([[0, 0, 1]], np.int32), 100)
    with pytest.raises(ValueError):
        decimate(V, np.array([[0, 1, len(V)]], np.int32), 100)
    with pytest.raises(ValueError):
        decimate(V[:, :2], F, 100)
    bad = V.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        decimate(bad, F, 100)
    for target in (3, 0, -5, 10.5):
        with pytest.raises(ValueError):
            decimate(V, F, target)
    with pytest.raises(ValueError):
        decimate(V, F, 100, max_surf_dist=-1.0)
    with pytest.raises(ValueError):
        decimate(V, F, 100, min_quality=2.0)
    # a target at or above the face count: the compacted input, bit for bit
    Vx = np.concatenate([V[:5], np.zeros((2, 3), np.float32), V[5:]])          # two unreferenced vertices
    Fx = np.where(F >= 5, F + 2, F).astype(np.int32)
    for target in (len(F), len(F) + 100):
        stats = {}
        Vd, Fd = decimate(Vx, Fx, target, stats=stats)
        assert Vd.tobytes() == V.tobytes() and np.array_equal(Fd, F) and stats['rounds'] == 0 and stats['faces_out'] == len(F)


def _rounded_box(res):
    x = torch.linspace(-1.0, 1.0, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(x, x, x, indexing='ij')
    q = torch.stack([X.abs() - 0.45, Y.abs() - 0.35, Z.abs() - 0.25], -1)      # half-extents 0.6 x 0.5 x 0.4, corner radius 0.15
    return (q.clamp(min=0).norm(dim=-1) + q.max(-1).values.clamp(max=0) - 0.15).float()


def test_adaptive_beats_uniform_at_equal_face_count(gpu):
    """A rounded box (flat sides, curved edges), 64^3 marching cubes: decimation to the face count remesh_isotropic reaches must be
    closer to the input in the mean than the uniform remesh is."""
    from nu_nerf_amd.mesh import decimate, marching_cubes, mesh_distance, remesh_isotropic, _to_world
    V, F = marching_cubes(_rounded_box(64).to(gpu), 0.0)
    V, F = _to_world(V, 64, (-1, -1, -1), (1, 1, 1)), np.ascontiguousarray(np.fliplr(F.cpu().numpy()))
    diag = float(np.linalg.norm(V.max(0) - V.min(0)))
    Vr, Fr = remesh_isotropic(V, F, target_len=0.06 * diag, max_surf_dist=0.02 * diag, iterations=2)
    Vd, Fd = decimate(V, F, len(Fr))
    assert len(Fr) <= len(Fd) <= int(np.ceil(1.02 * len(Fr))) and directed_edge_defects(Fd) == 0
    dr = mesh_distance((Vr, Fr), (V, F), n_samples=200_000)
    dd = mesh_distance((Vd, Fd), (V, F), n_samples=200_000)
    mr, md = (dr['a_to_b_mean'] + dr['b_to_a_mean']) / 2, (dd['a_to_b_mean'] + dd['b_to_a_mean']) / 2
    print(f"rounded box {len(F)} faces -> remesh {len(Fr)} / decimate {len(Fd)}: mean distance {mr:.4e} / {md:.4e} "
          f"(ratio {mr / md:.2f}), hausdorff {dr['hausdorff']:.4e} / {dd['hausdorff']:.4e}")
    assert md < mr


def test_decimated_mesh_feeds_the_tracer_and_the_exporters(gpu, tmp_path, monkeypatch, capsys):
    import yaml
    from nu_nerf_amd import bake_textures as B
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.lbvh import LBVH
    from nu_nerf_amd.mesh import decimate, read_ply, write_ply
    from test_texture_gpu import golden, overrides_of, stage1_net
    V, F = _meshes()["golden24"]
    Vd, Fd = decimate(V, F, 1200)
    bvh = LBVH(*_dev(Vd, Fd, gpu))
    c, r = Vd.mean(0), float(np.linalg.norm(Vd - Vd.mean(0), axis=1).max())
    dirs = np.random.default_rng(5).normal(size=(256, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([c + 2 * r * dirs, -dirs], 1).astype(np.float32)      # from outside, towards the centroid
    hit, idx = bvh.intersect(torch.from_numpy(rays).to(gpu))
    assert bool((hit > 0).all()) and int(idx.min()) >= 0 and int(idx.max()) < len(Fd)
    # bake_textures --decimate: the atlas and the exports are those of the decimated mesh
    net, _ = stage1_net(gpu, overrides_of(golden('materials_stage1.npz')))
    scale = 0.5 / r
    Vw = ((V - c) * scale).astype(np.float32)                                    # into the networks' unit ball
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    os.makedirs('data/meshes')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 'data/model/tiny/model.pth')
    write_ply('data/meshes/tiny-1234.ply', Vw, F)
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = B.main(['--cfg', 'tiny.yaml', '--size', '256', '--decimate', '1200'])
    stem = 'tiny-1234_decimated'
    assert sorted(os.listdir(out)) == ['albedo.png', 'atlas.npz', 'orm.png'] + [stem + e for e in ('.bin', '.gltf', '.mtl', '.obj', '.ply')]
    Vp, Fp = read_ply(os.path.join(out, stem + '.ply'))
    Vq, Fq = decimate(Vw, F, 1200)
    assert Vp.tobytes() == Vq.tobytes() and np.array_equal(Fp, Fq) and 1200 <= len(Fp) <= 1224
    assert f'{len(Fp)} faces' in capsys.readouterr().out
    want = X.bake_textures(net, Vp, Fp, size=256)
    back = X.load_textures(out, len(Fp))
    for k in ('albedo', 'metallic', 'roughness', 'face'):
        assert np.array_equal(back[k], want[k].cpu().numpy()), k
    doc = json.load(open(os.path.join(out, stem + '.gltf')))
    acc = doc['accessors'][doc['meshes'][0]['primitives'][0]['attributes']['POSITION']]
    assert acc['count'] == 3 * len(Fp) and os.path.getsize(os.path.join(out, stem + '.bin')) == doc['buffers'][0]['byteLength']


def test_cli_round_trips_a_ply(gpu, tmp_path):
    from nu_nerf_amd.mesh import decimate, read_ply, write_ply
    V, F = _meshes()["icosphere"]
    write_ply(str(tmp_path / "s.ply"), V, F)
    r = _run("nu_nerf_amd.decimate", ["s.ply", "--faces", "200", "--max-surf-dist-pct", "2"], str(tmp_path))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    Vc, Fc = read_ply(str(tmp_path / "s_decimated.ply"))
    diag = float(np.linalg.norm(V.max(0).astype(np.float64) - V.min(0).astype(np.float64)))
    Vd, Fd = decimate(V, F, 200, max_surf_dist=0.02 * diag)
    assert Vc.tobytes() == Vd.tobytes() and np.array_equal(Fc, Fd)
    assert line['faces_in'] == 1280 and line['faces_out'] == len(Fd) and line['out'].endswith("s_decimated.ply") and 'per_round' in line


def test_extract_mesh_decimate_writes_its_file_and_remesh_consumes_it(gpu, tmp_path):
    import yaml
    from nu_nerf_amd.mesh import decimate, read_ply, remesh_isotropic
    from nu_nerf_amd.train_glue import save_checkpoint
    from test_mesh_gpu import S1CFG, golden_net
    net, _ = golden_net(gpu)
    (tmp_path / "s1.yaml").write_text(yaml.safe_dump(dict(S1CFG, zero_thickness=True)))
    os.makedirs(tmp_path / "data" / "model" / "golden")
    save_checkpoint(str(tmp_path / "data" / "model" / "golden" / "model.pth"), net, torch.optim.Adam(net.parameters()), 1234)
    _run("nu_nerf_amd.extract_mesh", ["--cfg", "s1.yaml", "--resolution", "64", "--decimate", "4000", "--remesh"], str(tmp_path))
    V, F = read_ply(str(tmp_path / "data" / "meshes" / "golden-1234.ply"))
    Vd, Fd = read_ply(str(tmp_path / "data" / "meshes" / "golden-1234_decimated.ply"))
    Vs, Fs = read_ply(str(tmp_path / "data" / "meshes" / "golden-1234_simplified.ply"))
    assert 4000 <= len(Fd) < len(F) and directed_edge_defects(Fd) == directed_edge_defects(F)
    Vq, Fq = decimate(V, F, 4000)
    assert Vd.tobytes() == Vq.tobytes() and np.array_equal(Fd, Fq)
    Vr, Fr = remesh_isotropic(Vd, Fd)                       # --remesh started from the decimated mesh
    assert Vs.tobytes() == Vr.tobytes() and np.array_equal(Fs, Fr)
