"""Mesh component labelling, statistics and floater removal on the GPU (nu_nerf_amd.components, csrc/components.hip) against the
numpy oracle (components_oracle.py): hand-built meshes, convergence of hook-and-compress, a scene of floaters and a bubble, meshes of
many workgroups, identity, determinism, marching cubes end to end, and the error paths."""
import functools

import numpy as np
import pytest
import torch

import components_oracle as O

pytestmark = pytest.mark.gpu

INT_KEYS = ('faces', 'vertices', 'edges', 'boundary_edges', 'nonmanifold_edges', 'euler')


def _ico(subdiv, radius):
    from nu_nerf_amd.lbvh import icosphere
    return icosphere(subdiv, radius)


@functools.lru_cache(maxsize=None)
def _scene():
    """The floater scene and its oracle results, computed once and shared (read-only)."""
    V, F, part = O.floater_scene(_ico)
    fl, vl, C = O.connected_components(V, F)
    return V, F, part, fl, vl, C, O.component_stats(V, F, fl, C)


def _check_stats(got, want, nfaces):
    """Integer statistics and the AABB exactly; area and volume within (n_faces + 32) 2^-52 S of the float64 oracle, S = the sum
    of the terms' magnitudes (each term rounds a few times at 2^-53 relative to its magnitude, and a sum of n terms in any order adds
    at most (n - 1) 2^-53 S)."""
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got['aabb_min'], want['aabb_min']) and np.array_equal(got['aabb_max'], want['aabb_max'])
    for k in ('area', 'volume'):
        assert got[k].dtype == np.float64
        err, bound = np.abs(got[k] - want[k]), (nfaces + 32) * 2.0 ** -52 * want[k + '_scale']
        print(k, "max err / bound", float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
        assert (err <= bound).all(), (k, err, bound)


# ------------------------------------------------------------------------------------------------ 1. hand-built meshes
def test_two_tetrahedra_and_a_stray_vertex(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = O.two_tets_and_a_stray()
    fl, vl, C = connected_components(V, F)
    assert C == 2 and vl[4] == -1 and fl.dtype == np.int32 and vl.dtype == np.int32
    ofl, ovl, _ = O.connected_components(V, F)
    assert np.array_equal(fl, ofl) and np.array_equal(vl, ovl)
    _check_stats(component_stats(V, F, fl, C), O.component_stats(V, F, ofl, 2), 4)


def test_tetrahedra_sharing_a_vertex(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = O.two_tets_sharing_a_vertex()
    fl, vl, C = connected_components(V, F, connectivity='vertex')
    assert C == 1 and (fl == 0).all() and (vl == 0).all()
    fl, vl, C = connected_components(V, F, connectivity='edge')
    assert C == 2 and vl is None and fl.tolist() == [0] * 4 + [1] * 4
    t = component_stats(V, F, fl, C)
    assert t['vertices'].tolist() == [4, 4] and t['euler'].tolist() == [2, 2]
    _check_stats(t, O.component_stats(V, F, fl, 2), 4)


def test_three_triangles_on_one_edge(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = O.fan_on_one_edge()
    fl, _, C = connected_components(V, F, connectivity='edge')
    assert C == 1 and (fl == 0).all()
    t = component_stats(V, F, fl, C)
    assert t['nonmanifold_edges'].tolist() == [1] and t['edges'].tolist() == [7]
    _check_stats(t, O.component_stats(V, F, fl, 1), 3)


def test_open_strip(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = O.strip(10)
    fl, _, C = connected_components(V, F)
    t = component_stats(V, F, fl, C)
    assert C == 1 and t['boundary_edges'].tolist() == [12] and t['euler'].tolist() == [1]
    _check_stats(t, O.component_stats(V, F, fl, 1), 10)


# ------------------------------------------------------------------------------------------------ 2. convergence
@pytest.mark.parametrize("perm_seed", [3, None])
@pytest.mark.parametrize("connectivity", ['vertex', 'edge'])
def test_strip_converges_in_few_rounds(gpu, perm_seed, connectivity):
    """4 096 triangles in one chain.  A synchronous simulation with every read taken at the round's start needs 7 rounds at this
    size; propagation without pointer jumping would need thousands."""
    from nu_nerf_amd.mesh import connected_components
    V, F = O.strip(4096, perm_seed=perm_seed)
    stats = {}
    fl, vl, C = connected_components(V, F, connectivity=connectivity, stats=stats)
    ofl, ovl, oC = O.connected_components(V, F, connectivity)
    print("rounds", stats['rounds'])
    assert C == oC == 1 and np.array_equal(fl, ofl) and (vl is None or np.array_equal(vl, ovl))
    assert 1 <= stats['rounds'] <= 32


# ------------------------------------------------------------------------------------------------ 3. floater scene
def test_floater_scene_labels_and_statistics(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F, part, ofl, ovl, oC, otable = _scene()
    fl, vl, C = connected_components(V, F)
    assert C == oC == 42 and np.array_equal(fl, ofl) and np.array_equal(vl, ovl)
    _check_stats(component_stats(V, F, fl, C), otable, len(F))
    efl, _, eC = connected_components(V, F, connectivity='edge')                  # closed manifold pieces: the same partition
    oefl, _, oeC = O.connected_components(V, F, 'edge')
    assert eC == oeC == 42 and np.array_equal(efl, oefl)
    _check_stats(component_stats(V, F, efl, eC), O.component_stats(V, F, oefl, oeC), len(F))


def _expected(V, F, fl, kept):
    return O.keep_components(V, F, fl, kept)


def test_floater_scene_removal(gpu):
    from nu_nerf_amd.mesh import remove_floaters
    V, F, part, ofl, _, _, otable = _scene()
    sphere, bubble = int(ofl[part == 0][0]), int(ofl[part == 1][0])
    # the largest component alone (the defaults)
    Vk, Fk = remove_floaters(V, F)
    Ve, Fe = _expected(V, F, ofl, O.select(otable))
    assert O.select(otable) == [sphere] and Vk.tobytes() == Ve.tobytes() and np.array_equal(Fk, Fe)
    # the big sphere plus the bubble, in the original relative order: the two largest components (keep=2; the bubble is the
    # second by area, and by the ranking rule the default keep=1 is the sphere alone, checked above)
    stats = {}
    Vk, Fk = remove_floaters(V, F, keep=2, stats=stats)
    assert sorted(stats['kept']) == sorted([sphere, bubble]) == O.select(otable, keep=2)
    Ve, Fe = _expected(V, F, ofl, [sphere, bubble])
    assert Vk.dtype == np.float32 and Fk.dtype == np.int32 and Vk.tobytes() == Ve.tobytes() and np.array_equal(Fk, Fe)
    assert len(Fk) == 5120 + 320 and np.array_equal(Vk[Fk], V[F[part <= 1]])     # the same triangles in the same order
    # drop_cavities: exactly the big sphere, under either orientation convention
    for Fin in (F, np.ascontiguousarray(np.fliplr(F))):
        Vk, Fk = remove_floaters(V, Fin, keep=2, drop_cavities=True)
        assert len(Fk) == 5120 and np.array_equal(Vk[Fk], V[Fin[part == 0]])
    # keep = 3 and min_faces = 81: the expected set comes from the oracle's rule.  The 40 blobs are translates of one another and
    # their areas agree to the last bits (two are equal in the oracle's own sums), so the third place is ranked on the table
    # remove_floaters itself used -- which test_floater_scene_labels_and_statistics holds to the oracle's
    stats = {}
    Vk, Fk = remove_floaters(V, F, keep=3, min_faces=81, stats=stats)
    want = O.select(stats['table'], keep=3, min_faces=81)
    Ve, Fe = _expected(V, F, ofl, want)
    assert stats['kept'] == want and len(want) == 3 and {sphere, bubble} < set(want)
    assert Vk.tobytes() == Ve.tobytes() and np.array_equal(Fk, Fe) and len(Fk) == 5120 + 320 + 80
    want = O.select(otable, keep=0, min_area_frac=0.1)
    Vk, Fk = remove_floaters(V, F, keep=0, min_area_frac=0.1)
    Ve, Fe = _expected(V, F, ofl, want)
    assert want == sorted([sphere, bubble]) and Vk.tobytes() == Ve.tobytes() and np.array_equal(Fk, Fe)


# ------------------------------------------------------------------------------------------------ 4. many workgroups
def test_two_large_spheres_and_floaters(gpu):
    from nu_nerf_amd.mesh import connected_components
    Vs, Fs = _ico(6, 0.4)
    rng = np.random.default_rng(11)
    parts = [(Vs + np.float32([-0.5, 0, 0]), Fs), (Vs + np.float32([0.5, 0, 0]), Fs)]
    parts += [(_ico(1, 0.004)[0] + c.astype(np.float32), _ico(1, 0.004)[1]) for c in rng.uniform(-1, 1, (12, 3)) * [0.05, 1, 1]]
    V, F, _, _ = O.shuffle(*O.merge(parts), seed=12)
    assert len(F) == 2 * 81920 + 12 * 80
    for connectivity in ('vertex', 'edge'):
        stats = {}
        fl, vl, C = connected_components(torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu), connectivity=connectivity, stats=stats)
        ofl, ovl, oC = O.connected_components(V, F, connectivity)
        print(connectivity, "rounds", stats['rounds'])
        assert fl.is_cuda and C == oC == 14 and np.array_equal(fl.cpu().numpy(), ofl)
        assert vl is None or np.array_equal(vl.cpu().numpy(), ovl)
        assert stats['rounds'] <= 32


def test_one_sphere_of_327680_faces(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = _ico(7, 0.5)
    Vd, Fd = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    fl, vl, C = connected_components(Vd, Fd)
    assert C == 1 and int(fl.max()) == 0 and int(vl.min()) == 0
    t = component_stats(Vd, Fd, fl, C)
    assert t['euler'].tolist() == [2] and t['faces'].tolist() == [327680] and t['boundary_edges'].tolist() == [0]
    assert abs(float(t['volume'][0]) - 4 / 3 * np.pi * 0.125) < 1e-3 * 4 / 3 * np.pi * 0.125


# ------------------------------------------------------------------------------------------------ 5. identity, 6. determinism
def test_clean_mesh_comes_back_bit_for_bit(gpu):
    from nu_nerf_amd.mesh import remove_floaters
    V, F = _ico(3, 0.5)
    for connectivity in ('vertex', 'edge'):
        Vk, Fk = remove_floaters(V, F, connectivity=connectivity)
        assert Vk.tobytes() == V.tobytes() and Fk.tobytes() == F.tobytes()
    Vd, Fd = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    Vk, Fk = remove_floaters(Vd, Fd)
    assert Vk.is_cuda and torch.equal(Vk, Vd) and torch.equal(Fk, Fd)


def test_two_calls_give_the_same_bits(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components
    V, F = _scene()[:2]
    Vd, Fd = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    runs = []
    for _ in range(2):
        fl, vl, C = connected_components(Vd, Fd)
        runs.append((fl, vl, component_stats(Vd, Fd, fl, C)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k, v in runs[0][2].items():
        assert v.cpu().numpy().tobytes() == runs[1][2][k].cpu().numpy().tobytes(), k


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_marching_cubes_mesh_loses_its_blobs_and_bubble(gpu):
    from nu_nerf_amd.lbvh import LBVH
    from nu_nerf_amd.mesh import _to_world, component_stats, connected_components, marching_cubes, remove_floaters
    res, r = 48, 0.6
    x = torch.linspace(-1.0, 1.0, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(x, x, x, indexing='ij')

    def ball(c, rad):
        return torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - rad
    blobs = [(0.85, 0.0, 0.0), (-0.6, 0.62, 0.0), (0.0, -0.6, 0.6), (-0.55, -0.55, -0.55)]
    u = torch.maximum(ball((0, 0, 0), r), -ball((0.1, 0.0, 0.05), 0.2))            # the sphere with a bubble cut out of it
    for c in blobs:
        u = torch.minimum(u, ball(c, 0.09))
    V, F = marching_cubes(u.float().to(gpu), 0.0)
    W = torch.from_numpy(_to_world(V, res, (-1, -1, -1), (1, 1, 1))).to(gpu)
    assert connected_components(W, F)[2] == 6
    Wk, Fk = remove_floaters(W, F, drop_cavities=True)
    fl, _, C = connected_components(Wk, Fk)
    t = {k: v.cpu().numpy() for k, v in component_stats(Wk, Fk, fl, C).items()}
    exact = 4.0 / 3.0 * np.pi * r ** 3
    assert C == 1 and t['boundary_edges'].tolist() == [0] and t['euler'].tolist() == [2]
    assert abs(abs(t['volume'][0]) - exact) < 0.02 * exact, (t['volume'], exact)
    # rays from outside aimed at the blob centres: they hit the blobs before cleaning, the sphere or nothing after
    rng = np.random.default_rng(5)
    c = np.repeat(np.asarray(blobs), 8, 0)
    o = c * 1.0 + rng.normal(size=c.shape) * 0.02 + c / np.linalg.norm(c, axis=1, keepdims=True) * 0.8
    d = c - o
    rays = torch.from_numpy(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)).to(gpu)
    hit, idx, tt = LBVH(W, F).intersect(rays, return_t=True)
    p = (rays[:, :3] + rays[:, 3:] * tt[:, None]).cpu().numpy()
    assert bool((hit > 0).all()) and (np.linalg.norm(p - c, axis=1) < 0.09 + 2.0 / (res - 1)).all()
    hit, idx, tt = LBVH(Wk, Fk).intersect(rays, return_t=True)
    h = (hit > 0).cpu().numpy()
    p = (rays[:, :3] + rays[:, 3:] * tt[:, None]).cpu().numpy()[h]
    assert h.any() and (np.abs(np.linalg.norm(p, axis=1) - r) < 2.0 / (res - 1)).all()


# ------------------------------------------------------------------------------------------------ 8. errors
def test_bad_input_raises(gpu):
    from nu_nerf_amd.mesh import component_stats, connected_components, remove_floaters
    V, F = O.two_tets_and_a_stray()
    bad = F.copy()
    bad[3, 1] = len(V)
    with pytest.raises(ValueError, match="out of range"):
        connected_components(V, bad)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="out of range"):
        remove_floaters(V, bad)
    Vn = V.copy()
    Vn[2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        remove_floaters(Vn, F)
    with pytest.raises(ValueError, match="connectivity"):
        connected_components(V, F, connectivity='corner')
    with pytest.raises(ValueError, match="face_label"):
        component_stats(V, F, np.full(len(F), 2, np.int32), 2)
    fl, vl, C = connected_components(V, np.zeros((0, 3), np.int32))             # an empty mesh: empty arrays
    assert C == 0 and len(fl) == 0 and (vl == -1).all()
    Vk, Fk = remove_floaters(V, np.zeros((0, 3), np.int32))
    assert Vk.shape == (0, 3) and Fk.shape == (0, 3)


def test_max_rounds_raises(gpu):
    """One round cannot label the permuted strip (several hooks land on one root and only the smallest survives): the driver stops
    and raises -- an ordinary early stop."""
    from nu_nerf_amd.components import connected_components
    V, F = O.strip(4096, perm_seed=3)
    with pytest.raises(RuntimeError, match="did not converge in 1 rounds"):
        connected_components(V, F, max_rounds=1)


# ------------------------------------------------------------------------------------------------ commands
def test_clean_mesh_command_writes_the_main_component(gpu, tmp_path, capsys):
    import json
    from nu_nerf_amd import clean_mesh
    from nu_nerf_amd.mesh import read_ply, write_ply
    V, F, part = _scene()[:3]
    src = str(tmp_path / "bear-300000.ply")
    write_ply(src, V, F)
    out = clean_mesh.main([src])
    assert out == str(tmp_path / "bear-300000_fixed.ply")
    Vk, Fk = read_ply(out)
    assert len(Fk) == 5120 and np.array_equal(Vk[Fk], V[F[part == 0]])
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report['out'] == out and report['faces'] == 5120 and len(report['before']) == 42 and len(report['after']) == 1
    assert report['after'][0]['euler'] == 2 and report['after'][0]['boundary_edges'] == 0 and len(report['kept']) == 1
    out = clean_mesh.main([src, "--keep", "2", "--out", str(tmp_path / "two.ply")])
    assert len(read_ply(out)[1]) == 5120 + 320


def test_extract_mesh_fix_writes_raw_fixed_and_simplified(gpu, tmp_path, monkeypatch):
    import yaml
    from test_mesh_gpu import S1CFG, golden_net
    from nu_nerf_amd import extract_mesh
    from nu_nerf_amd.mesh import read_ply, remove_floaters
    from nu_nerf_amd.train_glue import save_checkpoint
    net, _ = golden_net(gpu)
    (tmp_path / "s1.yaml").write_text(yaml.safe_dump(dict(S1CFG, zero_thickness=True)))
    (tmp_path / "data" / "model" / "golden").mkdir(parents=True)
    save_checkpoint(str(tmp_path / "data" / "model" / "golden" / "model.pth"), net, torch.optim.Adam(net.parameters()), 1234)
    monkeypatch.chdir(tmp_path)
    extract_mesh.main(["--cfg", "s1.yaml", "--resolution", "40", "--out", "plain/golden-1234.ply"])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["golden-1234.ply"]
    extract_mesh.main(["--cfg", "s1.yaml", "--resolution", "40", "--fix", "--remesh"])
    meshes = tmp_path / "data" / "meshes"
    assert sorted(p.name for p in meshes.iterdir()) == ["golden-1234.ply", "golden-1234_fixed.ply", "golden-1234_simplified.ply"]
    assert (meshes / "golden-1234.ply").read_bytes() == (tmp_path / "plain" / "golden-1234.ply").read_bytes()
    V, F = read_ply(str(meshes / "golden-1234.ply"))
    Vf, Ff = read_ply(str(meshes / "golden-1234_fixed.ply"))
    Ve, Fe = remove_floaters(V, F)
    assert Vf.tobytes() == Ve.tobytes() and np.array_equal(Ff, Fe) and len(Ff) > 100
    assert len(read_ply(str(meshes / "golden-1234_simplified.ply"))[1]) > 50
