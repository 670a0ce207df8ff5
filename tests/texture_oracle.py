"""numpy oracle of the texture atlas (include/nu_nerf.h): the ownership map, the per-texel barycentrics in a chosen
precision with the kernel's operation order, the fp32 surface points and normals of nu_atlas_texels operation for operation, a
float64 atlas of a per-face-corner attribute, and the float64 bilinear lookup that also reports which texels took part."""
import numpy as np


def owner_map(lay):
    """(face int32 [T,T] (-1: nobody), s, t int64 [T,T]: cell-local coordinates in the owning face's frame) from the header's rules."""
    T, c, cols, nf = lay['size'], lay['cell'], lay['cols'], lay['n_faces']
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    cx, cy = x // c, y // c
    i, j = x - cx * c, y - cy * c
    h = (i + j >= c).astype(np.int64)
    f = 2 * (cy * cols + cx) + h
    owned = (cx < cols) & (cy < cols) & (i + j != c - 1) & (f < nf)
    s = np.where(h == 1, c - 1 - i, i)
    t = np.where(h == 1, c - 1 - j, j)
    return np.where(owned, f, -1).astype(np.int32), s, t


def barycentrics(lay, dtype):
    """(face [T,T], b [T,T,3] of `dtype`): b1 = (s - pad) / L, b2 = (t - pad) / L, b0 = (1 - b1) - b2, each operation rounded to dtype."""
    face, s, t = owner_map(lay)
    L = dtype(lay['L'])
    b1 = (s - lay['pad']).astype(dtype) / L
    b2 = (t - lay['pad']).astype(dtype) / L
    b0 = (dtype(1) - b1) - b2
    return face, np.stack([b0, b1, b2], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def texels_f32(V, F, lay, VN=None):
    """(face int32 [T,T], points float32 [T,T,3], normals float32 [T,T,3] or None) as nu_atlas_texels computes them: every operation a
    separately rounded fp32 one, in its order; zeros on unowned texels."""
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int64)
    face, b = barycentrics(lay, np.float32)
    own = face >= 0
    fo = face[own]
    b0, b1, b2 = (b[own][:, k:k + 1] for k in range(3))
    v0, v1, v2 = (V[F[fo, k]] for k in range(3))
    points = np.zeros(face.shape + (3,), np.float32)
    points[own] = (b0 * v0 + b1 * v1) + b2 * v2
    assert points.dtype == np.float32
    if VN is None:
        return face, points, None
    VN = np.asarray(VN, np.float32)
    with np.errstate(all='ignore'):
        n = (b0 * VN[F[fo, 0]] + b1 * VN[F[fo, 1]]) + b2 * VN[F[fo, 2]]
        ln = np.sqrt(_dot(n, n))
        ok = (ln > 0) & (ln < np.float32(1e30))
        ng = _cross(v1 - v0, v2 - v0)
        lg = np.sqrt(_dot(ng, ng))
        okg = (lg > 0) & (lg < np.float32(1e30))
        geo = np.where(okg[:, None], ng / lg[:, None], np.float32(0))
        res = np.where(ok[:, None], n / ln[:, None], geo).astype(np.float32)
    normals = np.zeros(face.shape + (3,), np.float32)
    normals[own] = res
    return face, points, normals


def atlas_f64(lay, corner_values, sentinel=0.0):
    """float64 [T,T,C]: every owned texel holds sum_k b_k corner_values[f, k] (corner_values [Nf,3,C]) at its extrapolated barycentrics,
    every other texel `sentinel`."""
    face, b = barycentrics(lay, np.float64)
    cv = np.asarray(corner_values, np.float64)
    out = np.full(face.shape + (cv.shape[2],), float(sentinel), np.float64)
    own = face >= 0
    out[own] = np.einsum('nk,nkc->nc', b[own], cv[face[own]])
    return out


def lookup_f64(lay, atlas, face, u, v):
    """(values float64 [N,C], taps int64 [N,4,2] = (x, y) of the four taps, weights float64 [N,4]): the header's bilinear lookup in
    float64 with bilinear weights; a tap of weight 0 contributes exactly 0 whatever it holds."""
    c, pad, L, cols = lay['cell'], lay['pad'], lay['L'], lay['cols']
    face = np.asarray(face, np.int64)
    u = np.clip(np.asarray(u, np.float64), 0.0, 1.0)
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0 - u)
    s = pad + u * L
    t = np.minimum(pad + v * L, (2 * pad + L) - s)
    i0, j0 = np.floor(s).astype(np.int64), np.floor(t).astype(np.int64)
    fs, ft = s - i0, t - j0
    k, h = face >> 1, face & 1
    ox, oy = (k % cols) * c, (k // cols) * c
    taps, weights = [], []
    for di, dj, w in ((0, 0, (1 - fs) * (1 - ft)), (1, 0, fs * (1 - ft)), (0, 1, (1 - fs) * ft), (1, 1, fs * ft)):
        i, j = np.minimum(i0 + di, c - 1), np.minimum(j0 + dj, c - 1)
        taps.append(np.stack([ox + np.where(h == 1, c - 1 - i, i), oy + np.where(h == 1, c - 1 - j, j)], -1))
        weights.append(w)
    taps, weights = np.stack(taps, 1), np.stack(weights, 1)
    vals = atlas[taps[..., 1], taps[..., 0]]                                   # [N,4,C]
    contrib = np.where(weights[..., None] != 0, weights[..., None] * vals, 0.0)
    return contrib.sum(1), taps, weights


def triangle_points(n_faces, n_random, seed, n_edge=5):
    """(face [N], u [N], v [N]) float64: for the faces of an atlas, n_random uniform points of the triangle spread over the faces, plus
    for EVERY face its three corners and n_edge points on each of its three edges."""
    g = np.random.Generator(np.random.PCG64(seed))
    f = g.integers(0, n_faces, n_random)
    a, b = g.random(n_random), g.random(n_random)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    e = (np.arange(n_edge) + 0.5) / n_edge
    z = np.zeros(n_edge)
    cu = np.concatenate([[0.0, 1.0, 0.0], e, z, e])
    cv = np.concatenate([[0.0, 0.0, 1.0], z, e, 1.0 - e])
    allf = np.repeat(np.arange(n_faces), len(cu))
    return (np.concatenate([f, allf]), np.concatenate([a, np.tile(cu, n_faces)]), np.concatenate([b, np.tile(cv, n_faces)]))


def uv_area_checks(lay, uv):
    """Property 1 on the UV set atlas_uv returned: every triangle inside [0,1]^2 and inside its own half cell (the half cells tile
    without overlap, so the triangles are disjoint).  Returns the number of faces checked."""
    T, c, cols, pad, L = lay['size'], lay['cell'], lay['cols'], lay['pad'], lay['L']
    xy = np.asarray(uv, np.float64) * T - 0.5                                  # back to texel coordinates
    assert (np.asarray(uv) >= 0).all() and (np.asarray(uv) <= 1).all()
    f = np.arange(lay['n_faces'])
    k, h = f >> 1, f & 1
    origin = np.stack([(k % cols) * c, (k // cols) * c], -1)
    local = xy - origin[:, None, :]
    frame = np.where(h[:, None, None] == 1, (c - 1) - local, local)           # the face's own frame
    want = np.asarray([[pad, pad], [pad + L, pad], [pad, pad + L]], np.float64)
    assert np.abs(frame - want[None]).max() < 1e-3                             # float32 uv of a <= 32768 atlas
    assert (frame >= 0).all() and (frame.sum(-1) <= c - 2 + 1e-3).all()        # strictly on its side of the diagonal i + j = c - 1
    return len(f)
