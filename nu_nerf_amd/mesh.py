"""Mesh extraction from a trained SDF on the GPU: the link between stage 1 and stage 2 (extract_mesh_stage1.py / _stage2.py, which
run PyMCubes on a host grid: network/field.py:1286-1317).

  sdf_grid          dense device SDF grid through a Stage1Engine (slab compaction -> MFMA SDF forward -> scatter); never on the host
  marching_cubes    HIP marching cubes (csrc/mcubes.hip): V [Nv,3] in index space, F [Nf,3] int32, canonical order, deterministic
  extract_geometry  field.py:1310-1317 with any query_func, the grid kept on the device
  extract_mesh      the fast path: sdf_grid of a renderer's SDF + marching cubes, world coordinates
  write_ply         binary little-endian PLY that stage2.read_ply reads back unchanged
  read_ply          its inverse for any triangle PLY (ascii / binary little-endian, float / double, extra properties)
  remove_faces_near postprocess_stage2_mesh.py: drop the inner faces that lie on the outer shell (LBVH closest points)
  sample_surface    area-weighted deterministic surface samples on the device
  mesh_distance     Chamfer / Hausdorff distances of two meshes from surface samples and LBVH closest points
  remesh_isotropic  isotropic explicit remeshing (split / collapse / flip / relax on the device: remesh.py, csrc/remesh.hip)
  decimate          quadric-error edge-collapse decimation to a face budget (decimate.py, csrc/decimate.hip)
  connected_components / component_stats / remove_floaters   component labelling, statistics and floater removal (components.py,
                    csrc/components.hip)
  SparseGrid / sparse_sdf_grid / marching_cubes_sparse / extract_mesh_sparse / stage2_inner_sparse   block-sparse extraction: the SDF
                    evaluated only near the surface (mesh_sparse.py, csrc/mcubes_sparse.hip)

Conventions (DESIGN.md "Mesh extraction"): a grid point is INSIDE when u < threshold; triangles wind so that their right-handed
normal points inside, which is where the reference's raw PyMCubes output of an sdf (positive outside) points before the face flip of
extract_mesh_stage1.py:40 -- after np.fliplr the normals point outward.  Every entry runs on the caller's current stream and syncs
the host once (the sizes of the outputs), plus once per sdf_grid (the row counts of its slabs).
"""
import numpy as np
import torch

from . import _lib as L
from .engine import addr

# grid points per slab of sdf_grid: the no-grad layered SDF forward holds ~3.3 KB of activations per evaluated row, so 2^19 points
# keep a slab under ~1.8 GB even when every point is inside the unit sphere
SLAB_POINTS = 1 << 19
_BRICK = 256


def _lib():
    return L.load()


def _workspace(lib, dev, nx, ny, nz):
    nbytes = lib.nu_mc_workspace_bytes(nx, ny, nz)
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev), nbytes


def _as_device_grid(u):
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
    if not torch.is_tensor(u) or u.dim() != 3:
        raise ValueError("marching_cubes: u must be a 3-d grid u[nx][ny][nz]")
    L.require_cuda(u)
    if u.dtype != torch.float32:
        raise ValueError("marching_cubes: u must be float32")
    if min(u.shape) < 2:
        raise ValueError(f"marching_cubes: every grid dimension must be >= 2, got {tuple(u.shape)}")
    return u.contiguous()


def _mc_device(u, threshold):
    """V [Nv,3] float32 (index space) and F [Nf,3] int32 on u's device."""
    lib = _lib()
    dev = u.device
    nx, ny, nz = (int(s) for s in u.shape)
    iso = float(threshold)
    with torch.cuda.device(dev):
        S = L.stream(dev.index)
        ws, nbytes = _workspace(lib, dev, nx, ny, nz)
        tot = torch.empty(2, dtype=torch.int64, device=dev)
        lib.nu_mc_count(addr(u), nx, ny, nz, iso, addr(ws), nbytes, S)
        lib.nu_mc_scan(nx, ny, nz, addr(ws), nbytes, addr(tot), S)
        nv, nf = (int(x) for x in tot.cpu())                  # the one host sync: sizes of the outputs
        if nv >= 2 ** 31:
            raise ValueError(f"marching_cubes: {nv} vertices do not fit int32 face indices")
        V = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        F = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nv == 0:
            return V, F
        first_vid = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)   # written at the owners only (read at the owners only)
        lib.nu_mc_write_vertices(addr(u), nx, ny, nz, iso, addr(ws), nbytes, addr(V), addr(first_vid), S)
        lib.nu_mc_write_triangles(addr(u), nx, ny, nz, iso, addr(ws), nbytes, addr(first_vid), addr(F), S)
    return V, F


def marching_cubes(u, threshold):
    """Marching cubes of the grid u[nx][ny][nz] (C order, the layout of the reference's numpy grid) at `threshold`.
    Returns (V float32 [Nv,3] in index space, F int32 [Nf,3]): device tensors for a device tensor, numpy arrays for a numpy array.
    Vertices are ordered by (owner grid point, axis), triangles by (cell, table slot); two runs give the same bits."""
    host = isinstance(u, np.ndarray)
    V, F = _mc_device(_as_device_grid(u), threshold)
    if host:
        return V.cpu().numpy(), F.cpu().numpy()
    return V, F


def _linspaces(bound_min, bound_max, res):
    """The three CPU torch.linspace vectors of extract_fields (field.py:1288-1290): every grid coordinate bit-equal to the reference."""
    return [torch.linspace(float(bound_min[a]), float(bound_max[a]), res) for a in range(3)]


@torch.no_grad()
def sdf_grid(engine, bmin, bmax, res, outside_val=1.0, slab_points=None, stats=None):
    """Dense SDF grid u[res][res][res] (device, fp32) of `engine`'s SDF network on the extract_fields grid: the points with
    NOT |x| >= 1 (torch.norm's arithmetic) go through Engine.sdf_forward(keep=False, want_feat=False) -- the fused kernel up to 40 000
    rows, the layered GEMMs above, bit-identical -- and every other point gets `outside_val` without being evaluated.
    The grid is cut into slabs of `slab_points` consecutive points (C order; a multiple of 256): per slab a HIP kernel compacts its
    inside points into x rows, the SDF forward runs on them, and a second kernel scatters the results (a row's bits do not depend on
    the batch it is evaluated in: scripts/debug_rowwise_independence.py).  stats: a dict that receives 'points' (rows evaluated)
    and 'slabs'."""
    lib = _lib()
    dev = engine.dev
    res = int(res)
    if res < 2:
        raise ValueError("sdf_grid: res must be >= 2")
    slab = int(slab_points or SLAB_POINTS)
    slab = max(_BRICK, slab // _BRICK * _BRICK)
    npts = res ** 3
    with torch.cuda.device(dev):
        S = L.stream(dev.index)
        X, Y, Z = (v.to(dev) for v in _linspaces(bmin, bmax, res))
        engine.pack()
        ws, nbytes = _workspace(lib, dev, res, res, res)
        nslab = (npts + slab - 1) // slab
        rows_at = torch.empty(nslab + 1, dtype=torch.int64, device=dev)
        lib.nu_grid_inside_count(addr(X), addr(Y), addr(Z), res, res, res, slab, addr(ws), nbytes, addr(rows_at), S)
        rows_at = rows_at.cpu().tolist()                           # the one host sync: row counts of every slab
        if stats is not None:
            stats.update(points=rows_at[-1], slabs=nslab)
        u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
        for s in range(nslab):
            p0 = s * slab
            n = min(slab, npts - p0)
            P = rows_at[s + 1] - rows_at[s]
            sdf = None
            if P > 0:
                rows = engine.empty(P, 3)
                lib.nu_grid_compact(addr(X), addr(Y), addr(Z), res, res, res, p0, n, addr(ws), nbytes, addr(rows), S)
                sdf = engine.sdf_forward(addr(rows), 3, P, keep=False, want_feat=False)['sdf']
            lib.nu_grid_scatter(addr(X), addr(Y), addr(Z), res, res, res, p0, n, addr(ws),
                                nbytes, addr(sdf), float(outside_val), addr(u), S)
    return u


def _to_world(V, res, bmin, bmax):
    """field.py:1314-1316: v / (res - 1) (bmax - bmin) + bmin (in float64, as numpy does it there), stored as float32."""
    bmin = np.asarray([float(b) for b in bmin], np.float32)
    bmax = np.asarray([float(b) for b in bmax], np.float32)
    Vn = V.cpu().numpy() if torch.is_tensor(V) else V
    W = Vn.astype(np.float64) / (res - 1.0) * (bmax - bmin)[None, :] + bmin[None, :]
    return W.astype(np.float32)


@torch.no_grad()
def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, outside_val=1.0):
    """field.py:1310-1317 without a host grid: query_func runs on the point blocks of extract_fields (64^3 per call, same order and
    coordinates), its values (outside the unit sphere: outside_val) fill a device grid, and marching cubes runs on the device.
    Returns (vertices float32 [Nv,3] in world coordinates, triangles int32 [Nf,3]) as numpy arrays."""
    res = int(resolution)
    N = 64
    dev = bound_min.device if torch.is_tensor(bound_min) and bound_min.is_cuda else torch.device('cuda', torch.cuda.current_device())
    X, Y, Z = (v.split(N) for v in _linspaces(bound_min, bound_max, res))
    u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).to(dev)
                val = query_func(pts).detach().reshape(-1).to(torch.float32).clone()
                val[torch.norm(pts, dim=-1) >= 1.0] = outside_val
                u[xi * N: xi * N + len(xs), yi * N: yi * N + len(ys), zi * N: zi * N + len(zs)] = val.reshape(len(xs), len(ys), len(zs))
    V, F = _mc_device(u, threshold)
    return _to_world(V, res, bound_min, bound_max), F.cpu().numpy()


BOX_MIN, BOX_MAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


@torch.no_grad()
def extract_mesh(renderer, resolution, threshold=0.0, slab_points=None):
    """extract_mesh_stage1.py without its face flip: the renderer's SDF (positive outside) on the [-1,1]^3 grid through sdf_grid,
    marching cubes at `threshold`.  Returns (vertices float32 [Nv,3] world, triangles int32 [Nf,3]) as numpy arrays."""
    u = sdf_grid(renderer.engine(), BOX_MIN, BOX_MAX, resolution, slab_points=slab_points)
    V, F = _mc_device(u, threshold)
    return _to_world(V, resolution, BOX_MIN, BOX_MAX), F.cpu().numpy()


@torch.no_grad()
def stage2_inner_grid(stage2_renderer, resolution, slab_points=None):
    """The composite field of extract_mesh_stage2.py:42-43 on the [-1,1]^3 grid: the inner sdf where the stage-1 sdf is < 0, 1
    elsewhere -- two sdf_grid calls (the stage-1 engine and the inner engine of Stage2Renderer.nets()) and one select, on the device."""
    s1 = sdf_grid(stage2_renderer.stage1_network.engine(), BOX_MIN, BOX_MAX, resolution, slab_points=slab_points)
    inner = sdf_grid(stage2_renderer.nets()[1].eng, BOX_MIN, BOX_MAX, resolution, slab_points=slab_points)
    return torch.where(s1 < 0, inner, torch.ones_like(inner))


def write_ply(path, V, F, colors=None):
    """Binary little-endian PLY: float x, y, z per vertex; uchar count + int vertex indices per face.  colors (optional, [Nv,3]):
    uchar red, green, blue per vertex behind the coordinates -- uint8 as given, floats as round(255 c) clipped to [0, 255]; without
    it the file is the plain mesh, byte for byte."""
    V = np.ascontiguousarray(V.cpu().numpy() if torch.is_tensor(V) else V, dtype='<f4').reshape(-1, 3)
    F = np.ascontiguousarray(F.cpu().numpy() if torch.is_tensor(F) else F).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError("write_ply: face index out of range")
    faces = np.empty(len(F), dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    faces['n'] = 3
    faces['i'] = F
    cprops = ""
    if colors is not None:
        C = np.asarray(colors.cpu().numpy() if torch.is_tensor(colors) else colors)
        if C.shape != (len(V), 3):
            raise ValueError(f"write_ply: colors must be [{len(V)}, 3], got {tuple(C.shape)}")
        if C.dtype != np.uint8:
            C = np.clip(np.rint(255.0 * C.astype(np.float64)), 0, 255).astype(np.uint8)
        verts = np.empty(len(V), dtype=np.dtype([('p', '<f4', (3,)), ('c', 'u1', (3,))]))
        verts['p'], verts['c'] = V, C
        V = verts
        cprops = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(V)}\nproperty float x\nproperty float y\nproperty float z\n{cprops}"
              f"element face {len(F)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(V.tobytes())
        fh.write(faces.tobytes())


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_type(name, path):
    if name not in _PLY_TYPES:
        raise ValueError(f"read_ply: {path}: unsupported property type {name!r}")
    return np.dtype('<' + _PLY_TYPES[name])


def _ply_header(data, path):
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError(f"read_ply: {path} is not a PLY file")
    body = data.index(b'\n', end) + 1
    fmt, elements = None, []                    # elements: [name, count, [(prop, type) or (prop, (count type, index type))]]
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property' and elements:
            if tok[1] == 'list':
                elements[-1][2].append((tok[4], (_ply_type(tok[2], path), _ply_type(tok[3], path))))
            else:
                elements[-1][2].append((tok[2], _ply_type(tok[1], path)))
    if fmt == 'binary_big_endian':
        raise ValueError(f"read_ply: {path}: big-endian PLY is not supported")
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f"read_ply: {path}: unknown format {fmt!r}")
    return fmt, elements, body


def read_ply(path, colors=False):
    """Triangle mesh from a PLY file -> (V float32 [Nv,3], F int32 [Nf,3]); the inverse of write_ply.  Reads ascii and binary
    little-endian files with float or double coordinates; other vertex properties (normals, colours) and other elements without
    lists are skipped; the face list may count in uchar / int / uint and index in int / uint.  Refuses non-triangle faces,
    big-endian files and face indices outside the vertices.  colors=True: returns (V, F, C) with C uint8 [Nv,3] from the vertex
    properties red / green / blue, or None when the file has none."""
    path = str(path)
    with open(path, 'rb') as fh:
        data = fh.read()
    fmt, elements, off = _ply_header(data, path)
    V = F = C = None
    tokens = data[off:].decode('ascii', 'replace').split() if fmt == 'ascii' else None
    ti = 0
    for name, count, props in elements:
        lists = [p for p, t in props if isinstance(t, tuple)]
        if name == 'vertex' and lists:
            raise ValueError(f"read_ply: {path}: list properties on vertices are not supported")
        if name == 'face' and len(lists) != 1:
            raise ValueError(f"read_ply: {path}: a face element needs exactly one list property")
        if name not in ('vertex', 'face') and lists:
            raise ValueError(f"read_ply: {path}: element {name!r} with a list property is not supported")
        if fmt == 'ascii':
            if name == 'face':
                F = np.empty((count, 3), np.int64)
                for r in range(count):
                    for p, t in props:
                        if isinstance(t, tuple):
                            n = int(tokens[ti])
                            if n != 3:
                                raise ValueError(f"read_ply: {path}: face {r} has {n} vertices; only triangles are supported")
                            F[r] = [int(x) for x in tokens[ti + 1: ti + 4]]
                            ti += 4
                        else:
                            ti += 1
            else:
                width = len(props)
                vals = tokens[ti: ti + count * width]
                if len(vals) < count * width:
                    raise ValueError(f"read_ply: {path}: file is truncated")
                ti += count * width
                if name == 'vertex':
                    rows = np.asarray(vals, np.float64).reshape(count, width)
                    cols = [[p for p, _ in props].index(c) for c in 'xyz']
                    V = rows[:, cols].astype(np.float32)
                    names = [p for p, _ in props]
                    if all(c in names for c in ('red', 'green', 'blue')):
                        C = rows[:, [names.index(c) for c in ('red', 'green', 'blue')]].astype(np.uint8)
            continue
        fields = []
        for p, t in props:
            fields += [('n', t[0]), ('i', t[1], (3,))] if isinstance(t, tuple) else [(p, t)]
        dt = np.dtype(fields)
        fit = min(count, max(0, (len(data) - off) // dt.itemsize))
        rec = np.frombuffer(data, dtype=dt, count=fit, offset=off)
        if name == 'face':
            bad = np.nonzero(rec['n'] != 3)[0]     # records up to the first non-triangle are laid out as assumed
            if len(bad):
                raise ValueError(f"read_ply: {path}: face {int(bad[0])} has {int(rec['n'][bad[0]])} vertices; only triangles are "
                                 "supported")
        if fit < count:
            raise ValueError(f"read_ply: {path}: file is truncated")
        off += count * dt.itemsize
        if name == 'vertex':
            V = np.stack([rec['x'], rec['y'], rec['z']], 1).astype(np.float32)
            if all(c in rec.dtype.names for c in ('red', 'green', 'blue')):
                C = np.stack([rec['red'], rec['green'], rec['blue']], 1).astype(np.uint8)
        elif name == 'face':
            F = rec['i'].astype(np.int64)
    if V is None:
        raise ValueError(f"read_ply: {path}: no vertex element")
    if F is None:
        F = np.zeros((0, 3), np.int64)
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError(f"read_ply: {path}: face index out of range (vertices: {len(V)})")
    if colors:
        return np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32), C
    return np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _as_device_mesh(V, F, dev):
    V = V if torch.is_tensor(V) else torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32))
    F = F if torch.is_tensor(F) else torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32))
    return V.to(device=dev, dtype=torch.float32).contiguous(), F.to(device=dev, dtype=torch.int32).contiguous()


def remove_faces_near(V_in, F_in, V_out, F_out, min_dist=0.055):
    """postprocess_stage2_mesh.py: keep the faces of the inner mesh (V_in, F_in) whose three vertices all lie farther than min_dist
    from the outer mesh (V_out, F_out) -- faces on the outer shell, where the stage-2 field's torch.where seam makes a surface, go.
    Each inner vertex's distance is np.linalg.norm(v - closest) in float64 from the fp32 closest point on the outer mesh (the
    reference's Open3D compute_closest_points, here LBVH.closest_points).  Returns numpy (V float32, F int32): faces in their
    order, the vertices no kept face references dropped and the rest in their order, reindexed.  (The reference's trimesh
    update_faces + PLY export keeps every vertex; the kept triangles are the same.)"""
    from .lbvh import LBVH
    Vi = np.ascontiguousarray(V_in.cpu().numpy() if torch.is_tensor(V_in) else V_in, dtype=np.float32).reshape(-1, 3)
    Fi = np.asarray(F_in.cpu().numpy() if torch.is_tensor(F_in) else F_in, dtype=np.int64).reshape(-1, 3)
    dev = _device()
    bvh = LBVH(*_as_device_mesh(V_out, F_out, dev))
    _, _, q = bvh.closest_points(torch.from_numpy(Vi).to(dev))
    dist = np.linalg.norm(Vi.astype(np.float64) - q.cpu().numpy().astype(np.float64), axis=-1)
    keep = (dist > min_dist)[Fi].all(axis=1)
    F = Fi[keep]
    used = np.zeros(len(Vi), bool)
    used[F.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return Vi[used], remap[F].astype(np.int32).reshape(-1, 3)


def sample_surface(V, F, n, seed=0):
    """n points [n,3] float32 on the device, uniform over the mesh's area: a face by the inverse CDF of the cumulative face areas
    (float64, torch.searchsorted), a point in it by the square-root barycentric map; the uniforms come from a CPU generator
    seeded with `seed`, so a seed gives the same points on every run.  Zero-area faces are never drawn."""
    V, F = _as_device_mesh(V, F, V.device if torch.is_tensor(V) and V.is_cuda else _device())
    n = int(n)
    if len(F) == 0:
        raise ValueError("sample_surface: the mesh has no triangles")
    tri = V.double()[F.long()]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    cdf = torch.cumsum(0.5 * torch.linalg.norm(torch.cross(b - a, c - a, dim=1), dim=1), 0)
    total = cdf[-1]
    if not float(total) > 0:
        raise ValueError("sample_surface: the mesh has no area")
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(n, 3, dtype=torch.float64, generator=g).to(V.device)
    fi = torch.searchsorted(cdf, u[:, 0] * total, right=True).clamp_(max=len(F) - 1)
    r1, r2 = torch.sqrt(u[:, 1:2]), u[:, 2:3]
    p = a[fi] * (1.0 - r1) + b[fi] * (r1 * (1.0 - r2)) + c[fi] * (r1 * r2)
    return p.to(torch.float32)


def mesh_distance(A, B, n_samples=1_000_000, seed=0):
    """Distances between the meshes A = (V, F) and B from n_samples surface samples of each (sample_surface, the same seed for
    both, so swapping A and B swaps the directions exactly) and closest points on the other mesh (LBVH.closest_points):
    a_to_b_mean, b_to_a_mean, chamfer (their mean), a_to_b_max, b_to_a_max, hausdorff (the larger maximum)."""
    from .lbvh import LBVH
    dev = _device()
    (VA, FA), (VB, FB) = _as_device_mesh(*A, dev), _as_device_mesh(*B, dev)
    bvh_a, bvh_b = LBVH(VA, FA), LBVH(VB, FB)
    d_ab = bvh_b.closest_points(sample_surface(VA, FA, n_samples, seed))[0].double().sqrt()
    d_ba = bvh_a.closest_points(sample_surface(VB, FB, n_samples, seed))[0].double().sqrt()
    ab_mean, ba_mean, ab_max, ba_max = (float(x) for x in torch.stack([d_ab.mean(), d_ba.mean(), d_ab.max(), d_ba.max()]).cpu())
    return dict(a_to_b_mean=ab_mean, b_to_a_mean=ba_mean, chamfer=(ab_mean + ba_mean) / 2, a_to_b_max=ab_max, b_to_a_max=ba_max,
                hausdorff=max(ab_max, ba_max))


def remesh_isotropic(V, F, target_len=None, max_surf_dist=None, iterations=3, stats=None):
    """Isotropic explicit remeshing on the GPU (the reference's pymeshlab step before stage 2): see remesh.remesh_isotropic."""
    from .remesh import remesh_isotropic as _remesh
    return _remesh(V, F, target_len=target_len, max_surf_dist=max_surf_dist, iterations=iterations, stats=stats)


def decimate(V, F, target_faces, max_surf_dist=None, min_quality=0.1, max_rounds=256, tolerance=0.02, stats=None):
    """Quadric-error decimation to about target_faces faces on the GPU (never fewer): see decimate.decimate."""
    from .decimate import decimate as _decimate
    return _decimate(V, F, target_faces, max_surf_dist=max_surf_dist, min_quality=min_quality, max_rounds=max_rounds,
                     tolerance=tolerance, stats=stats)


def connected_components(V, F, connectivity='vertex', stats=None):
    """Component labels of the mesh's faces and vertices on the GPU: see components.connected_components."""
    from .components import connected_components as _cc
    return _cc(V, F, connectivity=connectivity, stats=stats)


def component_stats(V, F, face_label, C):
    """Per-component counts, Euler characteristic, AABB, area and signed volume on the GPU: see components.component_stats."""
    from .components import component_stats as _stats
    return _stats(V, F, face_label, C)


def remove_floaters(V, F, keep=1, min_area_frac=None, min_faces=None, drop_cavities=False, connectivity='vertex', stats=None):
    """The mesh without its floaters (and, with drop_cavities, its bubbles) on the GPU: see components.remove_floaters."""
    from .components import remove_floaters as _remove
    return _remove(V, F, keep=keep, min_area_frac=min_area_frac, min_faces=min_faces, drop_cavities=drop_cavities,
                   connectivity=connectivity, stats=stats)


# block-sparse extraction (mesh_sparse.py, csrc/mcubes_sparse.hip): re-exported here, loaded on first use (mesh_sparse imports this module)
_SPARSE = ('SparseGrid', 'sparse_sdf_grid', 'marching_cubes_sparse', 'extract_mesh_sparse', 'stage2_inner_sparse',
           'extract_stage2_mesh_sparse')


def __getattr__(name):
    if name in _SPARSE:
        from . import mesh_sparse
        return getattr(mesh_sparse, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
