"""Per-vertex curvature of the trained surface, from the SDF's Hessian.

The non-zero-thickness stage 2 (stage2_thick.py) refracts through a wall of two concentric spheres whose radius is the per-vertex
Gaussian curvature of the stage-1 mesh (DiffRender.py:331,360: PyMesh's, clipped to [-10, 10]; here lbvh.vertex_normals_and_curvature,
the angle defect over the vertex area).  On the meshes marching cubes produces that discrete curvature is poor: vertices
inside a flat facet get none, vertices on a crease all of it.  The surface those meshes sample is the zero set of a smooth function,
the SDF network f, which has an exact curvature everywhere.  With g = grad f and H = Hessian f:

    mean      k_m = (|g|^2 tr H - g^T H g) / (2 |g|^3)
    Gaussian  K   = g^T adj(H) g / |g|^4
    normal    n   = g / |g|

Sign: n points where f grows (outward for an SDF that is positive outside); k_m is the mean of the principal curvatures and is
POSITIVE for a convex body (f = |x| - r: k_m = 1 / r, K = 1 / r^2).  Where |g|^2 < 1e-12 the three are 0.

The whole evaluation is ONE launch of csrc/sdf_jet.hip (nu_sdf_jet_fwd) for any vertex count: the second-order jet of the network in
forward mode, no workspace, fp32 in every `mlp_dtype` (the kernel reads the fp32 packed tables pack() always writes).  Results are not
clipped; lbvh.Scene(curvature=...) clips when it takes them.  'outer' is the stage-1 SDF, 'inner' a stage-2 model's inner SDF, as in
materials.py.  This is the project's own quantity: the reference has no counterpart, and PyMesh's curvature stays unpinned.
"""
import math

import numpy as np
import torch

from .materials import _check_points, bake_engine, mesh_vertices

PERCENTILES = (5, 50, 95)


@torch.no_grad()
def bake_curvature(renderer, points, *, which=None, hessian=False):
    """Curvature of the SDF's level sets at `points` ([V, >= 3] float32 device tensor, contiguous; the first three columns are x) ->
    dict of device tensors 'sdf' [V], 'normal' [V,3], 'gradient' [V,3], 'mean' [V], 'gaussian' [V,1] (the shape of
    Scene.gaussian_curvatures), plus 'hessian' [V,6] = (xx, yy, zz, xy, xz, yz) on request.  One kernel launch for any V.  which: see
    materials.bake_engine."""
    eng = bake_engine(renderer, which)
    points = _check_points(points, eng.dev)
    V = points.shape[0]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)      # noqa: E731
    out = {'sdf': e(V), 'normal': e(V, 3), 'gradient': e(V, 3), 'mean': e(V), 'gaussian': e(V, 1)}
    if hessian:
        out['hessian'] = e(V, 6)
    if V == 0:
        return out
    eng.pack()
    eng.sdf_jet(points.data_ptr(), points.shape[1], V, out['sdf'], out['gradient'], out.get('hessian'), out['mean'], out['gaussian'],
                out['normal'])
    return out


@torch.no_grad()
def bake_normals(renderer, points, *, which=None):
    """Value, gradient and unit normal of the SDF at `points` ([V, >= 3] float32 device tensor, contiguous) -> dict of device tensors
    'sdf' [V], 'gradient' [V,3], 'normal' [V,3] = gradient / |gradient| (it points where f grows; 0 where |gradient|^2 < 1e-12): the
    three bake_curvature returns under these names, bit for bit, from ONE launch of the first-order kernel (csrc/sdf_grad.hip,
    nu_sdf_grad_fwd) for any V -- four rows per point instead of ten, the tool for the texels of an atlas (texture.bake_textures(...,
    normals='sdf')).  which: see materials.bake_engine."""
    eng = bake_engine(renderer, which)
    points = _check_points(points, eng.dev)
    V = points.shape[0]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)      # noqa: E731
    out = {'sdf': e(V), 'gradient': e(V, 3), 'normal': e(V, 3)}
    if V == 0:
        return out
    eng.pack()
    eng.sdf_grad(points.data_ptr(), points.shape[1], V, out['sdf'], out['gradient'], out['normal'])
    return out


def predict_curvature(renderer, mesh=None, which=None):
    """{'gaussian' [V,1], 'mean' [V], 'normal' [V,3]} as float32 numpy arrays in the vertex order of the mesh (materials.mesh_vertices:
    None = data/meshes/{name}-300000.ply, a PLY path, or a (V, F) pair)."""
    V = mesh_vertices(renderer, mesh)
    dev = next(renderer.parameters()).device
    out = bake_curvature(renderer, torch.from_numpy(V).to(dev), which=which)
    return {k: out[k].cpu().numpy() for k in ('gaussian', 'mean', 'normal')}


# ---- mesh statistics of a per-vertex curvature (host, float64) -------------------------------------------------------------------------
def vertex_areas(V, F):
    """A_v [V] float64: a third of the area of the incident faces."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    tri = V[F]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    out = np.zeros(len(V))
    np.add.at(out, F.reshape(-1), np.repeat(area / 3.0, 3))
    return out


def euler_characteristic(n_verts, F):
    """V - E + F of a triangle mesh (edges counted once whatever their face count)."""
    F = np.asarray(F, np.int64)
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(F)


def gauss_bonnet_ratio(K, V, F):
    """sum_v K(v) A_v / (2 pi chi): 1 for the exact curvature of a closed surface in the limit of a fine mesh.  None when chi = 0."""
    chi = euler_characteristic(len(V), F)
    if chi == 0:
        return None
    return float(np.sum(np.asarray(K, np.float64).reshape(-1) * vertex_areas(V, F)) / (2.0 * math.pi * chi))


def curvature_stats(K):
    """{'p5', 'p50', 'p95', 'outside_pm10'} of a per-vertex curvature: percentiles and the share of vertices the +-10 clip changes."""
    K = np.asarray(K, np.float64).reshape(-1)
    if K.size == 0:
        return {**{f'p{p}': None for p in PERCENTILES}, 'outside_pm10': None}
    out = {f'p{p}': float(np.percentile(K, p)) for p in PERCENTILES}
    out['outside_pm10'] = float(np.mean(np.abs(K) > 10.0))
    return out
