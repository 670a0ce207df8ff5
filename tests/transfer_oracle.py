"""float64 / integer restatement of the visibility transfer: the sample sequence as integers, the rays, the transfer row of a
point from given verdicts, the barycentric mix at a hit point, the shadowed split-sum colour, and the closed forms the tests pin."""
import numpy as np

import relight_oracle as RO
import splitsum_oracle as SO

ROW = 16
_M32 = np.uint64(0xFFFFFFFF)
SH_BAND = np.asarray([1.0, 2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0, 0.25, 0.25, 0.25, 0.25, 0.25])


# ---- integer part --------------------------------------------------------------------------------------------------------------------
def sample_bits(ids, seed, S):
    """(b1, b2) int64 [n,S]: the two 24-bit integers of every sample of the points that hash as `ids` [n]."""
    ids = np.asarray(ids, np.int64).reshape(-1, 1)
    j = np.arange(S, dtype=np.uint64).reshape(1, -1)
    x1 = (j << np.uint64(32)) // np.uint64(S)
    x2 = RO.bitrev32(j)
    a = RO.fmix32((ids.astype(np.uint64) & _M32) + np.uint64(0x9E3779B9))
    a = RO.fmix32(a ^ np.uint64(int(seed) & 0xFFFFFFFF))
    h1 = RO.fmix32(a + np.uint64(1))
    h2 = RO.fmix32(h1 ^ np.uint64(0x68E31DA4))
    return (((x1 + h1) & _M32) >> np.uint64(8)).astype(np.int64), (((x2 + h2) & _M32) >> np.uint64(8)).astype(np.int64)


# ---- rays ----------------------------------------------------------------------------------------------------------------------------
def rays(points, normals, b1, b2, eps):
    """(origins [n,S,3], directions [n,S,3]) float64 from the integers b1, b2 [n,S]."""
    p, n = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    u1, u2 = b1 * 2.0 ** -24, b2 * 2.0 ** -24
    t, b = RO.frame(n)
    phi = 2.0 * np.pi * u1
    ct, st = np.sqrt(1.0 - u2), np.sqrt(u2)
    d = (st * np.cos(phi))[..., None] * t[:, None] + (st * np.sin(phi))[..., None] * b[:, None] + ct[..., None] * n[:, None]
    o = np.broadcast_to((p + eps * n)[:, None], d.shape)
    return o, d


def sh9(d):
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def unoccluded(normals):
    """(1, 2/3, 1/4)_l Y_k(n): the transfer of a point that sees its whole hemisphere."""
    return sh9(normals) * SH_BAND


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def transfer_rows(dirs, vis, normals):
    """Rows float64 [n,16] from directions [n,S,3], verdicts vis [n,S] (1 = unoccluded) and the points' normals [n,3]."""
    d, v = np.asarray(dirs, np.float64), np.asarray(vis, np.float64)
    S = d.shape[1]
    out = np.zeros((d.shape[0], ROW))
    out[:, 0:9] = (v[..., None] * sh9(d)).sum(1) / S
    out[:, 9] = v.sum(1) / S
    b = (v[..., None] * d).sum(1)
    ln = np.linalg.norm(b, axis=1, keepdims=True)
    out[:, 10:13] = np.where(ln < 1e-12, np.asarray(normals, np.float64), b / np.maximum(ln, 1e-300))
    return out


# ---- occluders in closed form and by brute force -----------------------------------------------------------------------------------------
def sphere_occludes(o, d, centre, radius, tmax=np.inf):
    """bool [...]: the ray (o, d) meets the sphere at some 0 < t < tmax (origins outside the sphere)."""
    oc = np.asarray(o, np.float64) - np.asarray(centre, np.float64)
    a = np.sum(d * d, -1)
    b = np.sum(oc * d, -1)
    c = np.sum(oc * oc, -1) - radius * radius
    disc = b * b - a * c
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
    return (disc > 0) & (t > 0) & (t < tmax)


def any_hit(tri, o, d, tmax=1e16):
    """bool [N]: ray i meets one of the triangles tri [K,3,3] at 0 < t < tmax (Moeller-Trumbore, float64, every pair)."""
    v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    dd, oo = d[:, None], o[:, None]
    pv = np.cross(dd, e2)
    det = np.sum(e1 * pv, -1)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / det
        tv = oo - v0
        u = np.sum(tv * pv, -1) * inv
        qv = np.cross(tv, e1)
        v = np.sum(dd * qv, -1) * inv
        t = np.sum(e2 * qv, -1) * inv
        return ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < tmax)).any(1)


def convex_self_occlusion(V, F, vertex, o, d):
    """Share of the rays (o [S,3], d [S,3]) leaving `vertex` of a closed CONVEX mesh that the mesh itself stops, by brute force: a ray
    from outside enters a convex body through a face whose plane the origin lies strictly above, so only those faces are swept."""
    V = np.asarray(V, np.float64)
    tri = V[np.asarray(F, np.int64)]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    front = np.sum((o[0][None] - tri[:, 0]) * fn, 1) > 0
    return float(any_hit(tri[front], o, d).mean()) if front.any() else 0.0


# ---- the shadowed resolve ----------------------------------------------------------------------------------------------------------------
def barycentric_uv(x, v0, v1, v2):
    """(u, v) [N] of x = v0 + u (v1 - v0) + v (v2 - v0) by least squares; 0, 0 for a face without area (the device's formula)."""
    e1, e2, t = v1 - v0, v2 - v0, x - v0
    d11, d12, d22 = np.sum(e1 * e1, 1), np.sum(e1 * e2, 1), np.sum(e2 * e2, 1)
    t1, t2 = np.sum(t * e1, 1), np.sum(t * e2, 1)
    den = d11 * d22 - d12 * d12
    ok = den > 0
    safe = np.where(ok, den, 1.0)
    return np.where(ok, (d22 * t1 - d12 * t2) / safe, 0.0), np.where(ok, (d11 * t2 - d12 * t1) / safe, 0.0)


def transfer_at(V, F, transfer, face, x):
    """The 13 live columns [N,13] at hit points x [N,3] of faces `face` [N]: r0 + u (r1 - r0) + v (r2 - r0), bent normal renormalised."""
    V, T = np.asarray(V, np.float64), np.asarray(transfer, np.float64)
    f = np.asarray(F, np.int64)[np.asarray(face, np.int64)]
    u, v = barycentric_uv(np.asarray(x, np.float64), V[f[:, 0]], V[f[:, 1]], V[f[:, 2]])
    r0, r1, r2 = T[f[:, 0], :13], T[f[:, 1], :13], T[f[:, 2], :13]
    row = r0 + u[:, None] * (r1 - r0) + v[:, None] * (r2 - r0)
    ln = np.linalg.norm(row[:, 10:13], axis=1, keepdims=True)
    row[:, 10:13] = np.where(ln > 0, row[:, 10:13] / np.maximum(ln, 1e-300), r0[:, 10:13])
    return row


def spec_occlusion(nov, ao, rho):
    return np.clip((np.clip(nov, 0.0, 1.0) + ao) ** (2.0 ** (-16.0 * rho - 1.0)) - 1.0 + ao, 0.0, 1.0)


def resolve_occluded(rows, face, V, F, transfer, env_sh, mode, pyramid, levels, diffuse, lut):
    """rgb [N,3] of the G-buffer rows [N,20] of hit pixels with face ids `face`: mode 'ao' or 'sh' (env_sh [9,3])."""
    g = np.asarray(rows, np.float64)
    n, a, m, rho, v = g[:, 7:10], g[:, 10:13], g[:, 13:14], g[:, 14], g[:, 15:18]
    nov = np.sum(n * v, 1)
    r = 2.0 * nov[:, None] * n - v
    ab = RO.fg_lookup(np.asarray(lut, np.float64), nov, rho)
    f0 = 0.04 * (1.0 - m) + m * a
    sp = (f0 * ab[:, :1] + ab[:, 1:]) * SO.pyramid_lookup(pyramid, levels, r, rho)
    tr = transfer_at(V, F, transfer, face, g[:, 1:4])
    ao = tr[:, 9]
    so = spec_occlusion(nov, ao, rho)[:, None]
    if mode == 'ao':
        return ao[:, None] * ((1.0 - m) * a * RO.env_lookup(diffuse, n)) + so * sp
    return (1.0 - m) * a * np.maximum(tr[:, :9] @ np.asarray(env_sh, np.float64), 0.0) + so * sp
