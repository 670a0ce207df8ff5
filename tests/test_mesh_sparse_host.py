"""Block-sparse mesh extraction, the parts a host can check: the activation rule keeps every block a dense grid
requires on analytic 1-Lipschitz fields, the canonical mesh comparison, and the command's switches."""
import numpy as np
import pytest

import mesh_sparse_oracle as O


def _probe_values(field, probe):
    return field(probe.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("res", [41, 64])
@pytest.mark.parametrize("name", sorted(O.FIELDS))
def test_rule_keeps_every_required_block(name, res):
    B = 4
    X, Y, Z = O.axes(res)
    flags, probe, radius = O.regions(X, Y, Z, B)
    need, crossed = O.required_blocks(O.dense_field(O.FIELDS[name], X, Y, Z), B)
    assert crossed > 500 and need.sum() > 20
    active = O.active_rule(flags, radius, _probe_values(O.FIELDS[name], probe), 1.0)
    assert not (need & ~active).any(), int((need & ~active).sum())
    assert active.sum() < 0.8 * (flags > 0).sum()                      # the rule culls: it does not pass by keeping everything
    assert not (need & (flags == 0)).any()                                # a block that is never probed is never needed
    if name == 'clipped':
        assert (need & (flags == 2)).any()                                # the rim rule is exercised


@pytest.mark.parametrize("iso", [0.3, 0.45, -0.2])
def test_rule_follows_the_level(iso):
    """The level set at iso, not the zero set: 0.3 (radius 0.8) lies wholly outside the band around zero, 0.45 touches rim regions."""
    X, Y, Z = O.axes(64)
    flags, probe, radius = O.regions(X, Y, Z, 4)
    need, crossed = O.required_blocks(O.dense_field(O.FIELDS['sphere'], X, Y, Z), 4, iso)
    assert crossed > 500
    f = _probe_values(O.FIELDS['sphere'], probe)
    active = O.active_rule(flags, radius, f, 1.0, iso=iso)
    assert not (need & ~active).any() and active.sum() < 0.8 * (flags > 0).sum()
    if iso > 0:
        assert (need & ~O.active_rule(flags, radius, f, 1.0)).any()      # the band around zero does not hold it
    if iso == 0.45:
        assert (need & (flags == 2)).any()


@pytest.mark.parametrize("iso", [0.1, -0.1])
@pytest.mark.parametrize("name", sorted(O.PAIRS))
def test_composite_rule_follows_the_level(name, iso):
    X, Y, Z = O.axes(64)
    flags, probe, radius = O.regions(X, Y, Z, 4)
    need, crossed = O.required_blocks(O.dense_composite(O.PAIRS[name], X, Y, Z), 4, iso)
    assert crossed > 500
    s, g = (_probe_values(f, probe) for f in O.PAIRS[name])
    active = O.active_rule(flags, radius, s, 1.0, g, iso)
    assert not (need & ~active).any() and active.sum() < 0.8 * (flags > 0).sum()


def test_rule_misses_blocks_under_a_bound_that_is_too_small():
    X, Y, Z = O.axes(41)
    flags, probe, radius = O.regions(X, Y, Z, 4)
    need, _ = O.required_blocks(O.dense_field(O.FIELDS['sphere'], X, Y, Z), 4)
    active = O.active_rule(flags, radius, _probe_values(O.FIELDS['sphere'], probe), 0.05)
    assert (need & ~active).sum() > 0


def test_infinite_bound_activates_every_probed_block():
    X, Y, Z = O.axes(41)
    flags, probe, radius = O.regions(X, Y, Z, 4)
    active = O.active_rule(flags, radius, np.full(flags.shape, 1e30, np.float32), float('inf'))
    assert np.array_equal(active, flags > 0)
    ins = O.inside_mask(X, Y, Z)
    pi, pj, pk = np.nonzero(ins)
    assert (flags[pi // 4, pj // 4, pk // 4] > 0).all()                   # every inside point lies in a probed block


@pytest.mark.parametrize("res", [41, 64])
@pytest.mark.parametrize("name", sorted(O.PAIRS))
def test_composite_rule_keeps_every_required_block(name, res):
    B = 4
    X, Y, Z = O.axes(res)
    flags, probe, radius = O.regions(X, Y, Z, B)
    need, crossed = O.required_blocks(O.dense_composite(O.PAIRS[name], X, Y, Z), B)
    assert crossed > 500
    s, g = (_probe_values(f, probe) for f in O.PAIRS[name])
    active = O.active_rule(flags, radius, s, 1.0, g)
    assert not (need & ~active).any(), int((need & ~active).sum())
    assert active.sum() < 0.8 * (flags > 0).sum()


def test_region_geometry():
    X, Y, Z = O.axes(41)
    flags, probe, radius = O.regions(X, Y, Z, 4)
    assert flags.shape == (11, 11, 11) and flags[0, 0, 0] == 0 and flags[5, 5, 5] == 1 and (flags == 2).any()
    assert (np.linalg.norm(probe.astype(np.float64), axis=-1) <= 0.999 + 1e-6).all()
    h = 2.0 / 40
    assert abs(radius[5, 5, 5] - 0.5 * np.sqrt(3) * 5 * h) < 1e-5             # an interior region spans B + 1 cells per axis
    assert abs(radius[10, 5, 5] - 0.5 * np.sqrt(2 * 25 + 1) * h) < 1e-5       # the last block holds one point: its region two


def test_canonical_form():
    rng = np.random.default_rng(3)
    V = rng.normal(size=(50, 3)).astype(np.float32)
    V[7] = V[3]                                                            # two vertices on one position
    F = rng.integers(0, 50, size=(80, 3))
    perm = rng.permutation(50)
    inv = np.empty(50, np.int64)
    inv[perm] = np.arange(50)
    F2 = inv[F][rng.permutation(80)]
    F2 = np.stack([np.roll(f, k) for f, k in zip(F2, rng.integers(0, 3, size=80))])
    assert O.same_mesh((V, F), (V[perm], F2))
    flipped = F2.copy()
    flipped[5] = flipped[5][::-1]
    assert len(set(F2[5].tolist())) == 3 and not O.same_mesh((V, F), (V[perm], flipped))
    moved = V[perm].copy()
    moved[0, 0] = np.nextafter(moved[0, 0], np.float32(10))
    assert not O.same_mesh((V, F), (moved, F2))
    assert not O.same_mesh((V, F), (V[perm], F2[:-1]))


def test_cli_switches():
    from nu_nerf_amd.extract_mesh import parse_args
    plain = vars(parse_args(["--cfg", "x.yaml"]))
    assert plain['sparse'] is False and plain['block'] == 8 and plain['lipschitz'] == 2.0
    # every switch the command had keeps its default
    assert plain['resolution'] == 1024 and plain['ckpt'] is None and plain['out'] is None and plain['stage2'] is False
    assert plain['remesh'] is False and plain['fix'] is False and plain['decimate'] is None and plain['slab_points'] is None
    a = parse_args(["--cfg", "x.yaml", "--sparse", "--block", "4", "--lipschitz", "1.5", "--stage2", "--fix"])
    assert a.sparse and a.block == 4 and a.lipschitz == 1.5 and a.stage2 and a.fix
    rest = {k: v for k, v in vars(a).items() if k not in ('sparse', 'block', 'lipschitz', 'stage2', 'fix')}
    assert rest == {k: v for k, v in plain.items() if k in rest}
    for bad in (["--block", "5"], ["--lipschitz", "0"], ["--lipschitz", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(["--cfg", "x.yaml", "--sparse"] + bad)
    for stray in (["--block", "4"], ["--lipschitz", "2.0"]):             # not ignored without a word
        with pytest.raises(SystemExit):
            parse_args(["--cfg", "x.yaml"] + stray)


def test_api_is_reexported_and_checks_its_arguments():
    from nu_nerf_amd import mesh, mesh_sparse
    for name in ('SparseGrid', 'sparse_sdf_grid', 'marching_cubes_sparse', 'extract_mesh_sparse', 'stage2_inner_sparse',
                 'extract_stage2_mesh_sparse'):
        assert getattr(mesh, name) is getattr(mesh_sparse, name)
    with pytest.raises(AttributeError):
        mesh.no_such_name
    with pytest.raises(ValueError, match="block must be one of"):
        mesh_sparse._check_block(5)
    with pytest.raises(ValueError, match="int32 block ids"):
        mesh_sparse._block_dims((8192, 8192, 8192), 4)
    from nu_nerf_amd import _lib
    sig = {n: a for n, _, a in _lib._signatures()}
    for name in ('nu_smc_workspace_bytes', 'nu_smc_regions', 'nu_smc_activate', 'nu_smc_block_rows', 'nu_smc_finish', 'nu_smc_count',
                 'nu_smc_scan', 'nu_smc_write_vertices', 'nu_smc_write_triangles'):
        assert name in sig
