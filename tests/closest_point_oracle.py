"""Brute-force closest point on a triangle mesh in numpy float32, operation for operation the routine of nu_closest_tri
(nu_nerf_amd/csrc/lbvh.hip): numpy rounds every array operation once and never fuses a multiply-add, which is what the kernel's
`#pragma clang fp contract(off)` gives.  Ties in d2 go to the lowest face id.  `exact_d2` is an independent float64
reference by a different formulation (plane projection, else the clamped edges) to catch a region bug the two might share."""
import numpy as np

MISS_INDEX = 10000000


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dist2(p, q):
    e = p - q
    return _dot(e, e)


def _seg(p, a, b):
    ab, ap = b - a, p - a
    t = _dot(ap, ab)
    den = _dot(ab, ab)
    s = t / den
    q = a + ab * s[..., None]
    q = np.where((t >= den)[..., None], b, q)
    return np.where((t <= 0)[..., None], a, q)


def _edges(p, a, b, c):
    q = _seg(p, a, b)
    best = _dist2(p, q)
    for u, v in ((b, c), (c, a)):
        q1 = _seg(p, u, v)
        d = _dist2(p, q1)
        m = d < best
        best = np.where(m, d, best)
        q = np.where(m[..., None], q1, q)
    return q


def closest_on_triangles(p, a, b, c):
    """p [..., 3] against triangles a, b, c [..., 3] (broadcast), float32 -> (d2 [...], q [..., 3])."""
    f32 = np.float32
    zero = f32(0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ab, ac = b - a, c - a
        n = _cross(ab, ac)
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        den_ab, den_ac, den_bc = d1 - d3, d2 - d6, e43 + e56
        v_ab = np.where(den_ab > 0, d1 / den_ab, zero)
        w_ac = np.where(den_ac > 0, d2 / den_ac, zero)
        w_bc = np.where(den_bc > 0, e43 / den_bc, zero)
        s = (va + vb) + vc
        denom = f32(1) / s
        v, w = vb * denom, vc * denom
        face = (a + ab * v[..., None]) + ac * w[..., None]
        edges = _edges(p, a, b, c)
        conds = [_dot(n, n) == 0,
                 (d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (e43 >= 0) & (e56 >= 0),
                 ~((va >= 0) & (vb >= 0) & (vc >= 0) & (s > 0))]
        choices = [edges, a, b, a + ab * v_ab[..., None], c, a + ac * w_ac[..., None], b + (c - b) * w_bc[..., None], edges]
        shape = np.broadcast_shapes(p.shape, a.shape, b.shape, c.shape)
        q = face
        for cond, ch in zip(reversed(conds), reversed(choices)):      # the first region that applies wins
            q = np.where(cond[..., None], np.broadcast_to(ch, shape), q)
        return _dist2(p, q), q


def candidate_pairs(V, F, P, chunk_elems=1 << 22):
    """(query, face) pairs that can hold a query's closest face, by a float64 bound that shares nothing with the kernel's boxes:
    the distance to a face is at least |p - centroid| - (its circumradius about the centroid) and the closest one is at most
    the distance to the nearest vertex; a face is dropped only when its lower bound exceeds that by a margin (1e-4 + 1e-4 of the
    distance) far above fp32 rounding, so it can be neither the fp32 minimum nor tied with it."""
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    T = V[F]
    cen = T.mean(1)
    rad = np.sqrt(((T - cen[:, None, :]) ** 2).sum(-1)).max(1)
    used = np.unique(F)
    qs, fs = [], []
    step = max(1, chunk_elems // max(len(F), len(used)))
    for i in range(0, len(P), step):
        p = P[i:i + step]
        ub = np.sqrt(((p[:, None, :] - V[None, used]) ** 2).sum(-1).min(1))
        lb = np.sqrt(((p[:, None, :] - cen[None]) ** 2).sum(-1)) - rad[None]
        q, f = np.nonzero(lb <= (ub * (1 + 1e-4) + 1e-4)[:, None])
        qs.append(q + i)
        fs.append(f)
    return np.concatenate(qs), np.concatenate(fs)


def brute_force_closest(V, F, P, max_d2=np.inf):
    """-> (d2 f32 [N], idx i32 [N], closest f32 [N,3]) with the miss triple (inf, 10000000, 0) where no face has d2 <= max_d2."""
    V = np.asarray(V, np.float32)
    F = np.asarray(F, np.int64)
    P = np.asarray(P, np.float32).reshape(-1, 3)
    qi, fj = candidate_pairs(V, F, P)
    T = V[F[fj]]
    d2, q = closest_on_triangles(P[qi], T[:, 0], T[:, 1], T[:, 2])
    d2 = np.where(d2 <= np.float32(max_d2), d2, np.float32(np.inf))
    order = np.lexsort((fj, d2, qi))                            # per query: smallest d2, then the lowest face id
    first = order[np.unique(qi[order], return_index=True)[1]]
    assert np.array_equal(qi[first], np.arange(len(P)))
    best = d2[first]
    hit = np.isfinite(best)
    return (np.where(hit, best, np.float32(np.inf)).astype(np.float32), np.where(hit, fj[first], MISS_INDEX).astype(np.int32),
            np.where(hit[:, None], q[first], np.float32(0)).astype(np.float32))


def exact_d2(V, F, P, faces):
    """float64 squared distance from P[i] to face faces[i]: the projection onto the triangle's plane when it falls inside
    (barycentric signs from cross products with the normal), else the minimum over the three clamped segments."""
    V = np.asarray(V, np.float64)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    T = V[np.asarray(F, np.int64)[np.asarray(faces, np.int64)]]
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    n = np.cross(b - a, c - a)
    nn = np.sum(n * n, -1)

    def seg(u, v):
        d = v - u
        dd = np.sum(d * d, -1)
        t = np.clip(np.sum((P - u) * d, -1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        e = P - (u + d * t[:, None])
        return np.sum(e * e, -1)

    with np.errstate(divide='ignore', invalid='ignore'):
        h = np.sum((P - a) * n, -1) / nn
        x = P - n * h[:, None]
        wa = np.sum(np.cross(c - b, x - b) * n, -1)
        wb = np.sum(np.cross(a - c, x - c) * n, -1)
        wc = np.sum(np.cross(b - a, x - a) * n, -1)
    inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
    return np.where(inside, h * h * nn, np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a)))


def exact_min_d2(V, F, P):
    """float64 min over the faces of exact_d2 for every point [N]."""
    qi, fj = candidate_pairs(V, F, P)
    d = exact_d2(V, F, np.asarray(P, np.float64).reshape(-1, 3)[qi], fj)
    out = np.full(len(np.asarray(P).reshape(-1, 3)), np.inf)
    np.minimum.at(out, qi, d)
    return out
