"""Host side of mesh component labelling (nu_nerf_amd.components, clean_mesh): the numpy oracle against a plain BFS, the hand-built
meshes through the oracle, the selection rule, and the command line's defaults and output path.  No GPU."""
import numpy as np
import pytest

import components_oracle as O


@pytest.mark.parametrize("seed", range(6))
def test_union_find_matches_bfs_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    links = rng.integers(0, n, (int(rng.integers(0, 2 * n)), 2))
    uf, bfs = O.union_find(n, links), O.bfs_roots(n, links)
    assert np.array_equal(uf, bfs)
    assert (uf <= np.arange(n)).all() and (uf[uf] == uf).all()              # the root is the smallest id of its component


def test_two_tetrahedra_and_a_stray_vertex():
    V, F = O.two_tets_and_a_stray()
    fl, vl, C = O.connected_components(V, F)
    assert C == 2 and vl[4] == -1
    assert fl.tolist() == [0] * 4 + [1] * 4 and vl.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1]
    t = O.component_stats(V, F, fl, C)
    assert t['euler'].tolist() == [2, 2] and t['boundary_edges'].tolist() == [0, 0] and t['edges'].tolist() == [6, 6]
    np.testing.assert_allclose(t['volume'], [1 / 6, 1 / 6], rtol=1e-12)      # outward winding: positive


def test_tetrahedra_sharing_a_vertex_split_only_by_edge_connectivity():
    V, F = O.two_tets_sharing_a_vertex()
    assert O.connected_components(V, F, 'vertex')[2] == 1
    fl, vl, C = O.connected_components(V, F, 'edge')
    assert C == 2 and vl is None and fl.tolist() == [0] * 4 + [1] * 4
    t = O.component_stats(V, F, fl, C)
    assert t['vertices'].tolist() == [4, 4] and t['euler'].tolist() == [2, 2]  # the shared vertex counts in both


def test_three_triangles_on_one_edge():
    V, F = O.fan_on_one_edge()
    fl, _, C = O.connected_components(V, F, 'edge')
    assert C == 1
    t = O.component_stats(V, F, fl, C)
    assert t['nonmanifold_edges'].tolist() == [1] and t['edges'].tolist() == [7] and t['boundary_edges'].tolist() == [6]


def test_open_strip():
    V, F = O.strip(10)
    fl, _, C = O.connected_components(V, F)
    t = O.component_stats(V, F, fl, C)
    assert C == 1 and t['boundary_edges'].tolist() == [12] and t['euler'].tolist() == [1]
    np.testing.assert_allclose(t['area'], [5.0], rtol=1e-12)


def test_synchronous_hook_and_compress_needs_few_rounds():
    """Every read taken at the start of the round -- the stalest the device can be -- still converges in a handful of rounds."""
    for seed in (None, 3):
        V, F = O.strip(4096, perm_seed=seed)
        links = np.concatenate([F[:, :2], F[:, 1:]], 0)
        rounds = O.hook_compress_rounds(len(V), links)
        assert 1 <= rounds <= 12, rounds
    assert O.hook_compress_rounds(len(V), links) > 1                          # the permuted strip: max_rounds=1 cannot converge


def _table(area, faces, boundary, volume):
    return dict(area=np.asarray(area, np.float64), faces=np.asarray(faces, np.int32), boundary_edges=np.asarray(boundary, np.int32),
                volume=np.asarray(volume, np.float64))


def test_selection_rule_matches_the_oracle():
    from nu_nerf_amd.components import select_components
    rng = np.random.default_rng(0)
    for _ in range(50):
        C = int(rng.integers(1, 9))
        t = _table(rng.choice([0.5, 1.0, 2.0, 3.0], C), rng.integers(1, 200, C), rng.integers(0, 2, C), rng.choice([-1.0, 0.0, 2.0], C))
        kw = dict(keep=int(rng.integers(0, 4)), min_area_frac=[None, 0.4, 1.0][int(rng.integers(3))],
                  min_faces=[None, 50][int(rng.integers(2))], drop_cavities=bool(rng.integers(2)))
        assert np.nonzero(select_components(t, **kw))[0].tolist() == O.select(t, **kw), (t, kw)


def test_selection_rule_by_hand():
    from nu_nerf_amd.components import select_components
    t = _table([3.0, 0.5, 3.0, 0.01], [100, 40, 100, 80], [0, 0, 4, 0], [1.0, -0.2, 0.0, 0.001])
    assert select_components(t).tolist() == [True, False, False, False]                       # tie in area: the smaller id
    assert select_components(t, keep=2).tolist() == [True, False, True, False]
    assert select_components(t, keep=3, drop_cavities=True).tolist() == [True, False, True, False]   # the bubble goes, the open one stays
    assert select_components(t, min_faces=80).tolist() == [True, False, True, True]
    assert select_components(t, min_area_frac=0.1, min_faces=30).tolist() == [True, True, True, False]
    assert select_components(t, keep=0).tolist() == [False] * 4
    flipped = dict(t, volume=-t['volume'])                                                   # the other orientation convention
    assert select_components(flipped, keep=3, drop_cavities=True).tolist() == [True, False, True, False]
    with pytest.raises(ValueError):
        select_components(t, keep=-1)
    with pytest.raises(ValueError):
        select_components(t, min_area_frac=1.5)


def test_clean_mesh_command_line_defaults_and_output_path():
    from nu_nerf_amd import clean_mesh
    a = clean_mesh.parse_args(["data/meshes/bear-300000.ply"])
    assert (a.out, a.keep, a.min_area_frac, a.min_faces, a.drop_cavities, a.connectivity) == (None, 1, None, None, False, 'vertex')
    assert clean_mesh.fix_kwargs(a) == dict(keep=1, min_area_frac=None, min_faces=None, drop_cavities=False, connectivity='vertex')
    assert clean_mesh.fixed_path("data/meshes/bear-300000.ply") == "data/meshes/bear-300000_fixed.ply"
    assert clean_mesh.fixed_path("X.ply") == "X_fixed.ply"
    a = clean_mesh.parse_args(["X.ply", "--keep", "2", "--min-area-frac", "0.01", "--min-faces", "100", "--drop-cavities",
                               "--connectivity", "edge", "--out", "Y.ply"])
    assert clean_mesh.fix_kwargs(a) == dict(keep=2, min_area_frac=0.01, min_faces=100, drop_cavities=True, connectivity='edge')
    assert a.out == "Y.ply"


def test_extract_mesh_fix_is_off_by_default():
    from nu_nerf_amd import extract_mesh
    a = extract_mesh.parse_args(["--cfg", "c.yaml"])
    assert a.fix is False and a.remesh is False and a.keep == 1 and a.drop_cavities is False
    a = extract_mesh.parse_args(["--cfg", "c.yaml", "--fix", "--remesh", "--drop-cavities"])
    assert a.fix and a.remesh and a.drop_cavities


def test_header_declares_the_component_entries():
    from nu_nerf_amd import _lib
    names = {n for n, _, _ in _lib._signatures()}
    for must in ("nu_cc_init", "nu_cc_hook", "nu_cc_compress", "nu_cc_check", "nu_cc_labels", "nu_cc_compact", "nu_cc_face_stats"):
        assert must in names
    assert _lib.NU_CC_PARTS == 32
