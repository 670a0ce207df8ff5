"""Mesh extraction, host side (no GPU): the PLY writer round trip through stage2.read_ply, the CLI's argument parser, the
marching-cubes tables of csrc/mc_tables.h, and an independent numpy marching cubes (the GPU tests compare the HIP kernels to it)."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cube corners (dx, dy, dz) and edges (corner pairs), as documented in mc_tables.h
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def parse_tables():
    """(edge_table [256], tri_table [256] lists of edge ids) parsed from csrc/mc_tables.h."""
    text = open(os.path.join(ROOT, "nu_nerf_amd", "csrc", "mc_tables.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    et = re.search(r"nu_mc_edge_table\[256\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    edge_table = [int(t, 16) for t in re.findall(r"0x[0-9a-fA-F]+", et)]
    tt = re.search(r"nu_mc_tri_table\[256\]\[16\]\s*=\s*\{(.*)\};", text, re.S).group(1)
    rows = re.findall(r"\{([^{}]*)\}", tt)
    tri_table = [[int(t) for t in r.split(",") if int(t) >= 0] for r in rows]
    return edge_table, tri_table


def numpy_marching_cubes(u, iso):
    """Reference marching cubes: cells in C order, table slots in order; a vertex per straddling grid edge, keyed by
    (owner point, axis) and numbered in key order; t = (iso - u_a) / (u_b - u_a) in fp32.  Returns (V [Nv,3] f32, F [Nf,3] i32)."""
    _, tri = parse_tables()
    u = np.asarray(u, np.float32)
    nx, ny, nz = u.shape
    inside = u < np.float32(iso)
    ci = np.zeros((nx - 1, ny - 1, nz - 1), np.int32)
    for b, (dx, dy, dz) in enumerate(CORNERS):
        ci |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int32) << b
    keys = []
    for (i, j, k) in zip(*np.nonzero((ci != 0) & (ci != 255))):        # np.nonzero walks C order
        row = tri[ci[i, j, k]]
        for e in row:
            a, b = EDGES[e]
            pa = np.array(CORNERS[a]) + (i, j, k)
            pb = np.array(CORNERS[b]) + (i, j, k)
            lo = np.minimum(pa, pb)
            axis = int(np.argmax(np.abs(pb - pa)))
            keys.append(((lo[0] * ny + lo[1]) * nz + lo[2]) * 3 + axis)
    keys = np.asarray(keys, np.int64)
    uniq = np.unique(keys)
    F = np.searchsorted(uniq, keys).astype(np.int32).reshape(-1, 3)
    V = np.zeros((len(uniq), 3), np.float32)
    for n, key in enumerate(uniq):
        p, axis = divmod(int(key), 3)
        i, r = divmod(p, ny * nz)
        j, k = divmod(r, nz)
        q = [i, j, k]
        q2 = list(q)
        q2[axis] += 1
        ua, ub = u[tuple(q)], u[tuple(q2)]
        t = (np.float32(iso) - ua) / (ub - ua)
        v = np.array(q, np.float32)
        v[axis] = np.float32(v[axis] + t)
        V[n] = v
    return V, F


def directed_edge_defects(F):
    """Number of directed edges that do not appear exactly once with their reverse exactly once (0: closed, oriented 2-manifold)."""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    n = int(F.max()) + 1
    key = e[:, 0] * n + e[:, 1]
    rev = e[:, 1] * n + e[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    bad = int((cnt != 1).sum())
    bad += int((~np.isin(rev, uk)).sum())
    return bad


def test_tables_are_the_256_case_tables():
    edge_table, tri = parse_tables()
    assert len(edge_table) == 256 and len(tri) == 256
    assert edge_table[:4] == [0x000, 0x109, 0x203, 0x30a] and tri[1] == [0, 8, 3] and tri[0] == [] and tri[255] == []
    for c in range(256):
        strad = {e for e, (a, b) in enumerate(EDGES) if ((c >> a) & 1) != ((c >> b) & 1)}
        assert edge_table[c] == sum(1 << e for e in strad), c
        assert len(tri[c]) % 3 == 0 and len(tri[c]) <= 15
        assert set(tri[c]) == strad, c                       # every straddling edge carries a vertex, no other edge does


def test_numpy_marching_cubes_closed_on_random_fields():
    """The tables tile: on random fields with an outside border the mesh is a closed, consistently oriented 2-manifold."""
    rng = np.random.default_rng(3)
    for _ in range(3):
        u = rng.normal(size=(9, 8, 7)).astype(np.float32)
        u[[0, -1]] = 1.0
        u[:, [0, -1]] = 1.0
        u[:, :, [0, -1]] = 1.0
        V, F = numpy_marching_cubes(u, 0.0)
        assert len(F) > 100 and directed_edge_defects(F) == 0


def test_write_ply_read_ply_round_trip_is_exact(tmp_path):
    from nu_nerf_amd.mesh import write_ply
    from nu_nerf_amd.stage2 import read_ply
    rng = np.random.default_rng(0)
    V = rng.normal(size=(1001, 3)).astype(np.float32)
    V[0] = [np.float32(1e-38), -0.0, np.float32(3.4e38)]
    F = rng.integers(0, 1001, size=(2000, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, V, F)
    V2, F2 = read_ply(p)
    assert V2.dtype == np.float32 and F2.dtype == np.int32
    assert V2.tobytes() == V.tobytes() and np.array_equal(F2, F)
    write_ply(p, V[:0], F[:0])                               # empty mesh
    V3, F3 = read_ply(p)
    assert V3.shape == (0, 3) and F3.shape == (0, 3)


def test_extract_mesh_cli_help_parses():
    r = subprocess.run([sys.executable, "-m", "nu_nerf_amd.extract_mesh", "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--cfg", "--resolution", "--ckpt", "--out", "--stage2"):
        assert flag in r.stdout
    from nu_nerf_amd.extract_mesh import parse_args
    a = parse_args(["--cfg", "x.yaml"])
    assert a.resolution == 1024 and a.ckpt is None and a.out is None and not a.stage2
