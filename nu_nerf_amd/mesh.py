"""Mesh extraction from a trained SDF on the GPU: the link between stage 1 and stage 2 (extract_mesh_stage1.py / _stage2.py, which
run PyMCubes on a host grid: network/field.py:1286-1317).

  sdf_grid          dense device SDF grid through a Stage1Engine (slab compaction -> MFMA SDF forward -> scatter); never on the host
  marching_cubes    HIP marching cubes (csrc/mcubes.hip): V [Nv,3] in index space, F [Nf,3] int32, canonical order, deterministic
  extract_geometry  field.py:1310-1317 with any query_func, the grid kept on the device
  extract_mesh      the fast path: sdf_grid of a renderer's SDF + marching cubes, world coordinates
  write_ply         binary little-endian PLY that stage2.read_ply reads back unchanged

Conventions (DESIGN.md "Mesh extraction"): a grid point is INSIDE when u < threshold; triangles wind so that their right-handed
normal points inside, which is where the reference's raw PyMCubes output of an sdf (positive outside) points before the face flip of
extract_mesh_stage1.py:40 -- after np.fliplr the normals point outward.  Every entry runs on the caller's current stream and syncs
the host once (the sizes of the outputs), plus once per sdf_grid (the row counts of its slabs).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .engine import addr

c_p, c_ll, c_f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float

# grid points per slab of sdf_grid: the no-grad layered SDF forward holds ~3.3 KB of activations per evaluated row, so 2^19 points
# keep a slab under ~1.8 GB even when every point is inside the unit sphere
SLAB_POINTS = 1 << 19
_BRICK = 256


def _lib():
    lib = L.load()
    lib.nu_mc_workspace_bytes.restype = c_ll
    return lib


def _workspace(lib, dev, nx, ny, nz):
    nbytes = int(lib.nu_mc_workspace_bytes(nx, ny, nz))
    if nbytes < 0:
        raise L.NuNerfLibraryError(f"nu_mc_workspace_bytes({nx}, {ny}, {nz}) failed with code {nbytes}")
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
    iso = c_f(float(threshold))
    with torch.cuda.device(dev):
        S = L.stream(dev.index)
        ws, nbytes = _workspace(lib, dev, nx, ny, nz)
        tot = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(lib.nu_mc_count(c_p(addr(u)), nx, ny, nz, iso, c_p(addr(ws)), c_ll(nbytes), S), "nu_mc_count")
        L.check(lib.nu_mc_scan(nx, ny, nz, c_p(addr(ws)), c_ll(nbytes), c_p(addr(tot)), S), "nu_mc_scan")
        nv, nf = (int(x) for x in tot.cpu())                  # the one host sync: sizes of the outputs
        if nv >= 2 ** 31:
            raise ValueError(f"marching_cubes: {nv} vertices do not fit int32 face indices")
        V = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        F = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nv == 0:
            return V, F
        first_vid = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)   # written at the owners only (read at the owners only)
        L.check(lib.nu_mc_write_vertices(c_p(addr(u)), nx, ny, nz, iso, c_p(addr(ws)), c_ll(nbytes), c_p(addr(V)),
                                         c_p(addr(first_vid)), S), "nu_mc_write_vertices")
        L.check(lib.nu_mc_write_triangles(c_p(addr(u)), nx, ny, nz, iso, c_p(addr(ws)), c_ll(nbytes), c_p(addr(first_vid)),
                                          c_p(addr(F)), S), "nu_mc_write_triangles")
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
        L.check(lib.nu_grid_inside_count(c_p(addr(X)), c_p(addr(Y)), c_p(addr(Z)), res, res, res, c_ll(slab), c_p(addr(ws)),
                                         c_ll(nbytes), c_p(addr(rows_at)), S), "nu_grid_inside_count")
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
                L.check(lib.nu_grid_compact(c_p(addr(X)), c_p(addr(Y)), c_p(addr(Z)), res, res, res, c_ll(p0), c_ll(n), c_p(addr(ws)),
                                            c_ll(nbytes), c_p(addr(rows)), S), "nu_grid_compact")
                sdf = engine.sdf_forward(addr(rows), 3, P, keep=False, want_feat=False)['sdf']
            L.check(lib.nu_grid_scatter(c_p(addr(X)), c_p(addr(Y)), c_p(addr(Z)), res, res, res, c_ll(p0), c_ll(n), c_p(addr(ws)),
                                        c_ll(nbytes), c_p(addr(sdf)), c_f(float(outside_val)), c_p(addr(u)), S), "nu_grid_scatter")
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


def write_ply(path, V, F):
    """Binary little-endian PLY: float x, y, z per vertex; uchar count + int vertex indices per face."""
    V = np.ascontiguousarray(V.cpu().numpy() if torch.is_tensor(V) else V, dtype='<f4').reshape(-1, 3)
    F = np.ascontiguousarray(F.cpu().numpy() if torch.is_tensor(F) else F).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError("write_ply: face index out of range")
    faces = np.empty(len(F), dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    faces['n'] = 3
    faces['i'] = F
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(V)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(F)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(V.tobytes())
        fh.write(faces.tobytes())
