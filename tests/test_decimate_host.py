"""Quadric-error decimation, host side (no GPU): the port in tests/decimate_oracle.py on its own -- the quadric against plane
distances computed directly, the placement solve and its fallbacks, the key and budget rules, full runs on a cube and an open grid
-- plus the C ABI surface and the CLI's names and arguments."""
import functools
import os
import re

import numpy as np
import pytest

import decimate_oracle as D
from test_mesh_host import directed_edge_defects
from test_remesh_host import perturbed_icosphere, euler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_cube(n=8):
    """The unit cube with n x n quads per side (12 n^2 faces), outward, vertices at multiples of 1 / n (exact in fp32 for n = 8)."""
    ids, V, F = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(V)
            V.append([c / n for c in p])
        return ids[p]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]          # counter-clockwise seen from +axis
                    if side == 0:
                        q.reverse()
                    F += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def open_grid(n=16):
    """n x n quads in the plane z = 0 over [0, 1]^2 (2 n^2 faces), with a boundary."""
    V = np.array([[i / n, j / n, 0.0] for j in range(n + 1) for i in range(n + 1)], np.float32)
    F = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            F += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return V, np.asarray(F, np.int32)


def volume(V, F):
    W = V.astype(np.float64)
    return float(np.einsum('ij,ij->i', W[F[:, 0]], np.cross(W[F[:, 1]], W[F[:, 2]])).sum() / 6.0)


def on_cube_surface(V):
    """Every vertex exactly on the unit cube's surface: inside [0, 1]^3 with a coordinate that is exactly 0 or 1."""
    return bool(((V >= 0) & (V <= 1)).all() and ((V == 0) | (V == 1)).any(axis=1).all())


def boundary_vertices(V, F):
    T = D.Tables(V, F)
    return set(V[v].tobytes() for v in np.nonzero(T.vbound)[0])


@functools.lru_cache(maxsize=None)
def oracle_runs():
    """The oracle's full runs, computed once per process (test_decimate_gpu compares the device's results with them):
    name -> (V, F, stats)."""
    out = {}
    for name, (V, F), target in (("cube100", unit_cube(), 100), ("cube12", unit_cube(), 12), ("grid64", open_grid(), 64)):
        stats = {}
        Vd, Fd = D.decimate(V, F, target, stats=stats)
        out[name] = (Vd, Fd, stats)
    return out


@pytest.fixture(scope="module")
def runs():
    return oracle_runs()


def test_header_declares_the_decimation_entries():
    text = open(os.path.join(ROOT, "include", "nu_nerf.h")).read()
    for name in ("nu_dm_quadrics", "nu_dm_eval", "nu_dm_points", "nu_dm_keys", "nu_dm_claim", "nu_dm_apply"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_quadric_cost_is_the_weighted_plane_distance():
    V, F = perturbed_icosphere()
    M = D.Mesh(V, F)
    Q = D.quadrics(M)
    rng = np.random.default_rng(0)
    for v in rng.integers(0, len(V), 20):
        for x in rng.uniform(-1, 1, (5, 3)):
            direct = sum(w * (pl[0] * x[0] + pl[1] * x[1] + pl[2] * x[2] + pl[3]) ** 2 for w, pl in D.plane_terms(M, int(v)))
            got = D.cost_at(Q[v].tolist(), tuple(x.tolist()))
            assert abs(got - direct) <= 1e-12 * abs(direct), (v, got, direct)


def test_accepted_solves_satisfy_the_normal_equations():
    V, F = perturbed_icosphere()
    M = D.Mesh(V, F)
    Q = D.quadrics(M)
    solved = 0
    for e in range(M.nh):
        q = M.T.quad(e)
        if q is None:
            continue
        s = (Q[q[0]] + Q[q[1]]).tolist()
        x, how = D.placement(s, M.P[q[0]], M.P[q[1]])
        if how != 'solve':
            continue
        solved += 1
        A = np.array([[s[0], s[1], s[2]], [s[1], s[4], s[5]], [s[2], s[5], s[7]]])
        b = np.array([s[3], s[6], s[8]])
        scale = np.abs(A).max() * max(np.abs(x).max(), 1.0)
        assert np.abs(A @ np.array(x) + b).max() <= 1e-10 * scale
    assert solved > 100


def test_rank_deficient_quadrics_take_the_fallback():
    def quadric(planes):
        q = [0.0] * 10
        for pl in planes:
            for k, (i, j) in enumerate(D.PAIRS):
                q[k] += pl[i] * pl[j]
        return q
    pa, pb = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    rank1 = quadric([(0.0, 0.0, 1.0, 0.0)])                              # the plane z = 0: every point of the edge costs 0
    assert D.solve(rank1)[0] is None
    assert D.placement(rank1, pa, pb) == (pa, 'a')                        # a three-way tie goes to a
    rank2 = quadric([(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -1.0)])       # z = 0 and x = 1: b lies on both
    assert D.solve(rank2)[0] is None
    assert D.placement(rank2, pa, pb) == (pb, 'b')
    rank2m = quadric([(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -0.5)])      # z = 0 and x = 1/2: the midpoint
    assert D.placement(rank2m, pa, pb) == ((0.5, 0.0, 0.0), 'm')
    full = quadric([(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -0.25), (0.0, 1.0, 0.0, 0.0)])
    assert D.placement(full, pa, pb) == ((0.25, 0.0, 0.0), 'solve')
    far = quadric([(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -5.0), (0.0, 1.0, 0.0, 0.0)])      # minimiser far from the edge: refused
    assert D.placement(far, pa, pb)[1] == 'b'


def test_mix32_is_injective_and_keys_are_unique():
    n = 1 << 20
    h = np.arange(n, dtype=np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    assert len(np.unique(h)) == n
    assert [int(x) for x in h[:1000]] == [D.mix32(i) for i in range(1000)]
    V, F = unit_cube()
    M = D.Mesh(V, F)
    cost, pos, npts = D.evaluate(M, D.quadrics(M), 0.01)
    ckey = D.keys(cost, npts, D.cost_floor(V))
    live = ckey[ckey != D.NO_KEY]
    assert len(live) == int((npts > 0).sum()) > 500 and len(np.unique(live)) == len(live)
    assert (live >> 32).max() < (1 << 20)
    # flat faces: equal costs, so the order within the cube's faces is the hash's, not the edge table's
    flat = np.nonzero((npts > 0) & (cost == 0))[0]
    assert len(flat) > 100 and not np.array_equal(np.argsort(ckey[flat]), np.arange(len(flat)))


def test_budget_rule_never_admits_more_than_k():
    V, F = perturbed_icosphere()
    M = D.Mesh(V, F)
    cost, pos, npts = D.evaluate(M, D.quadrics(M), 0.01)
    ckey = D.keys(cost, npts, D.cost_floor(V))
    ncand = int((npts > 0).sum())
    for need in (1, 2, 7, ncand - 1, ncand, ncand + 5):
        thr = D.threshold(ckey, ncand, need)
        admitted = int(((ckey != D.NO_KEY) & (ckey <= thr)).sum())
        assert admitted == min(need, ncand)
        assert int(D.winners(M, ckey, thr).sum()) <= admitted
    thr = D.threshold(np.full(12, D.NO_KEY, np.int64), 0, 3)            # no candidate: nobody competes
    assert thr == D.NO_KEY


def test_winners_read_nothing_another_winner_writes():
    """The hold set is a, b, c, d, the write set the whole ring.  A winner moves `keep`, rewrites the faces of `rem` and lowers the
    valences of c and d; it reads the positions and faces of the ring and the valences of c and d.  So two winners must have no end
    in each other's ring and no opposite vertex in common -- on every round of a run, not just the first."""
    V, F = perturbed_icosphere()
    floor, checked = D.cost_floor(V), 0
    Vc, Fc = D.compact(V, F)
    for _ in range(6):
        r = D.one_round(Vc, Fc, len(Fc), floor, 0.01)           # no budget cut: the most winners the rule allows
        M, won = r['M'], [int(e) for e in np.nonzero(r['win'])[0]]
        quads = [M.T.quad(e) for e in won]
        rings = [set(D.ring(M, q[0], q[1])) for q in quads]
        assert len(won) >= 2
        for i in range(len(won)):
            for j in range(len(won)):
                if i != j:
                    assert not {quads[j][0], quads[j][1]} & rings[i]
                    assert not {quads[j][2], quads[j][3]} & {quads[i][2], quads[i][3]}
                    checked += 1
        Vc, Fc = D.compact(r['V'], r['F'])
        assert directed_edge_defects(Fc) == 0 and euler(Vc, Fc) == 2
        assert int(np.bincount(Fc.reshape(-1)).min()) >= 3
    assert checked > 100


def test_four_held_vertices_need_fewer_rounds_than_the_ring(runs):
    """The same cube run with the hold-everything rule of the remeshing collapse: as valid, but more rounds."""
    stats = {}
    V, F = D.decimate(*unit_cube(), 100, stats=stats, hold='ring')
    print("cube 768 -> 100: rounds with the ring held", stats['rounds'], "with a, b, c, d held", runs["cube100"][2]['rounds'])
    assert stats['converged'] and directed_edge_defects(F) == 0 and on_cube_surface(V) and volume(V, F) == 1.0
    assert stats['rounds'] > runs["cube100"][2]['rounds']


def test_extract_mesh_refuses_a_budget_below_four_when_parsing():
    from nu_nerf_amd.extract_mesh import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--cfg", "x.yaml", "--decimate", "3"])


@pytest.mark.parametrize("name,target", [("cube100", 100), ("cube12", 12)])
def test_oracle_cube_stays_a_unit_cube(runs, name, target):
    V, F, stats = runs[name]
    print(name, stats['rounds'], stats['faces_out'], stats['per_round'])
    assert stats['converged'] and stats['faces_in'] == 768
    assert target <= len(F) == stats['faces_out'] <= int(np.ceil(1.02 * target))
    assert directed_edge_defects(F) == 0 and euler(V, F) == 2 and len(np.unique(F)) == len(V)
    assert on_cube_surface(V)
    assert volume(V, F) == 1.0


def test_oracle_open_grid_keeps_its_plane_and_boundary(runs):
    V0, F0 = open_grid()
    V, F, stats = runs["grid64"]
    print("grid", stats['rounds'], stats['faces_out'])
    assert (V[:, 2] == 0).all()
    assert boundary_vertices(V, F) == boundary_vertices(V0, F0) and len(boundary_vertices(V0, F0)) == 64
    assert stats['converged'] is False and 64 < len(F) < len(F0)


def test_cli_names_and_arguments():
    from nu_nerf_amd import decimate as M
    a = M.parse_args(["m.ply", "--faces", "5000"])
    assert a.input == "m.ply" and a.faces == 5000 and a.max_surf_dist_pct is None and a.out is None
    a = M.parse_args(["m.ply", "--faces", "10", "--max-surf-dist-pct", "0.5", "--out", "o.ply"])
    assert a.max_surf_dist_pct == 0.5 and a.out == "o.ply"
    with pytest.raises(SystemExit):
        M.parse_args(["m.ply"])
    assert M.decimated_path(os.path.join("d", "golden-1234.ply")) == os.path.join("d", "golden-1234_decimated.ply")
    assert M.cost_floor((0, 0, 0), (1, 2, 2)) == 1e-12 * 81.0 and M.NO_KEY == D.NO_KEY
    from nu_nerf_amd.extract_mesh import parse_args
    assert parse_args(["--cfg", "x.yaml", "--decimate", "2000"]).decimate == 2000 and parse_args(["--cfg", "x.yaml"]).decimate is None
    from nu_nerf_amd.bake_textures import parse_args as bake_args
    assert bake_args(["--decimate", "300"] + BAKE_REQUIRED).decimate == 300 and bake_args(BAKE_REQUIRED).decimate is None
    import inspect
    from nu_nerf_amd import mesh
    assert list(inspect.signature(mesh.decimate).parameters) == ["V", "F", "target_faces", "max_surf_dist", "min_quality", "max_rounds",
                                                                  "tolerance", "stats"]


BAKE_REQUIRED = ["--cfg", "c.yaml"]
