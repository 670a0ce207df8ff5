"""mesh.read_ply (the inverse of write_ply) on files the tests write themselves, the refusals, the command lines' arguments, and the
closest-point oracle against its float64 counterpart -- no GPU needed."""
import struct

import numpy as np
import pytest

from closest_point_oracle import brute_force_closest, closest_on_triangles, exact_d2, exact_min_d2


def _mesh():
    from nu_nerf_amd.lbvh import icosphere
    return icosphere(1, 0.5)


def _header(fmt, nv, nf, vprops, flist="uchar int"):
    h = f"ply\nformat {fmt} 1.0\ncomment written by a test\nelement vertex {nv}\n"
    h += "".join(f"property {t} {n}\n" for t, n in vprops)
    h += f"element face {nf}\nproperty list {flist} vertex_indices\nend_header\n"
    return h.encode('ascii')


def test_round_trip_with_write_ply(tmp_path):
    from nu_nerf_amd.mesh import read_ply, write_ply
    V, F = _mesh()
    write_ply(tmp_path / "m.ply", V, F)
    V2, F2 = read_ply(tmp_path / "m.ply")
    assert V2.dtype == np.float32 and F2.dtype == np.int32
    assert np.array_equal(V2.view(np.uint32), V.view(np.uint32)) and np.array_equal(F2, F)
    write_ply(tmp_path / "e.ply", V, np.zeros((0, 3), np.int32))
    V3, F3 = read_ply(tmp_path / "e.ply")
    assert np.array_equal(V3, V) and F3.shape == (0, 3)


def test_ascii(tmp_path):
    from nu_nerf_amd.mesh import read_ply
    V, F = _mesh()
    body = "".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in V.astype(np.float64).tolist())
    body += "".join(f"3 {a} {b} {c}\n" for a, b, c in F.tolist())
    (tmp_path / "a.ply").write_bytes(_header("ascii", len(V), len(F), [("float", "x"), ("float", "y"), ("float", "z")]) + body.encode())
    V2, F2 = read_ply(tmp_path / "a.ply")
    assert np.array_equal(V2, V) and np.array_equal(F2, F)


@pytest.mark.parametrize("flist", ["uchar int", "int int", "uint uint", "uchar uint"])
def test_double_coordinates_extra_properties_and_list_types(tmp_path, flist):
    from nu_nerf_amd.mesh import read_ply
    V, F = _mesh()
    ct, it = flist.split()
    code = {'uchar': 'u1', 'int': '<i4', 'uint': '<u4'}
    vdt = np.dtype([('x', '<f8'), ('y', '<f8'), ('z', '<f8'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'), ('red', 'u1'),
                    ('green', 'u1'), ('blue', 'u1')])
    vert = np.zeros(len(V), vdt)
    for k, c in enumerate('xyz'):
        vert[c] = V[:, k].astype(np.float64) + 1e-12               # rounds back to the float32 value
    vert['nx'], vert['red'] = 1.0, 200
    fdt = np.dtype([('n', code[ct]), ('i', code[it], (3,)), ('flag', 'u1')])
    face = np.zeros(len(F), fdt)
    face['n'], face['i'], face['flag'] = 3, F, 7
    hdr = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(V)}\nproperty double x\nproperty double y\nproperty double z\n"
           "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
           f"element face {len(F)}\nproperty list {ct} {it} vertex_indices\nproperty uchar flag\n"
           "element edge 2\nproperty int vertex1\nproperty int vertex2\nend_header\n").encode()
    edges = np.array([[0, 1], [1, 2]], '<i4')
    (tmp_path / "d.ply").write_bytes(hdr + vert.tobytes() + face.tobytes() + edges.tobytes())
    V2, F2 = read_ply(tmp_path / "d.ply")
    assert np.array_equal(V2, (V.astype(np.float64) + 1e-12).astype(np.float32)) and np.array_equal(F2, F)


def _binary(tmp_path, V, F, counts=None, fmt="binary_little_endian", name="b.ply"):
    counts = [3] * len(F) if counts is None else counts
    end = '>' if fmt == "binary_big_endian" else '<'
    out = _header(fmt, len(V), len(F), [("float", "x"), ("float", "y"), ("float", "z")])
    out += np.asarray(V, end + 'f4').tobytes()
    for n, f in zip(counts, F):
        out += struct.pack(end + 'B' + 'i' * n, n, *[int(x) for x in list(f) + [0] * (n - 3)][:n])
    (tmp_path / name).write_bytes(out)
    return tmp_path / name


def test_refusals(tmp_path):
    from nu_nerf_amd.mesh import read_ply
    V, F = _mesh()
    with pytest.raises(ValueError, match="triangles"):
        read_ply(_binary(tmp_path, V, F, counts=[3] * 5 + [4] + [3] * (len(F) - 6)))
    with pytest.raises(ValueError, match="triangles"):
        read_ply(_binary(tmp_path, V, F, counts=[4] * len(F)))
    with pytest.raises(ValueError, match="big-endian"):
        read_ply(_binary(tmp_path, V, F, fmt="binary_big_endian"))
    bad = F.copy()
    bad[7, 1] = len(V)
    with pytest.raises(ValueError, match="out of range"):
        read_ply(_binary(tmp_path, V, bad))
    bad[7, 1] = -1
    with pytest.raises(ValueError, match="out of range"):
        read_ply(_binary(tmp_path, V, bad))
    body = "".join(f"{x} {y} {z}\n" for x, y, z in V.tolist()) + "".join(f"4 {a} {b} {c} {a}\n" for a, b, c in F.tolist())
    (tmp_path / "q.ply").write_bytes(_header("ascii", len(V), len(F), [("float", "x"), ("float", "y"), ("float", "z")]) + body.encode())
    with pytest.raises(ValueError, match="triangles"):
        read_ply(tmp_path / "q.ply")
    (tmp_path / "n.ply").write_bytes(b"solid not a ply\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply(tmp_path / "n.ply")
    full = _binary(tmp_path, V, F).read_bytes()
    (tmp_path / "t.ply").write_bytes(full[:-10])
    with pytest.raises(ValueError, match="truncated"):
        read_ply(tmp_path / "t.ply")


def test_command_line_arguments():
    from nu_nerf_amd import postprocess_mesh, mesh_distance
    a = postprocess_mesh.parse_args(["--inner", "s2.ply", "--outer", "s1.ply"])
    assert a.min_dist == 0.055 and a.out is None
    b = mesh_distance.parse_args(["a.ply", "b.ply", "--samples", "10", "--seed", "3"])
    assert (b.a, b.b, b.samples, b.seed) == ("a.ply", "b.ply", 10, 3)
    assert mesh_distance.parse_args(["a.ply", "b.ply"]).samples == 1_000_000


def test_oracle_regions_against_float64():
    """The fp32 oracle's regions agree with the independent float64 formulation, and its pruned search with the full sweep."""
    V, F = _mesh()
    g = np.random.default_rng(2)
    P = np.concatenate([g.uniform(-1, 1, (3000, 3)), V[g.integers(0, len(V), 500)]]).astype(np.float32)
    d2, idx, q = brute_force_closest(V, F, P)
    m = exact_min_d2(V, F, P)
    tol = 1e-6 * np.maximum(1.0, np.sum(P.astype(np.float64) ** 2, 1))
    assert (np.abs(d2 - m) <= tol).all() and (exact_d2(V, F, P, idx) - m <= tol).all()
    T = V[F]
    full, _ = closest_on_triangles(P[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
    assert np.array_equal(np.argmin(full, 1), idx) and np.array_equal(full[np.arange(len(P)), idx], d2)
    # a zero-area triangle is its edges: a point triangle gives the point, a segment the clamped segment
    a = np.array([[0.25, 0.5, 0.0]], np.float32)
    dd, qq = closest_on_triangles(np.array([[1.0, 1.0, 1.0]], np.float32), a, a, a)
    assert np.array_equal(qq, a) and np.isfinite(dd).all()
    b = np.array([[1.25, 0.5, 0.0]], np.float32)
    dd, qq = closest_on_triangles(np.array([[0.75, 2.0, 0.0]], np.float32), a, b, b)
    assert np.array_equal(qq, [[0.75, 0.5, 0.0]]) and dd[0] == np.float32(2.25)
