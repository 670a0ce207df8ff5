"""Numpy ports of the remeshing passes of nu_nerf_amd/csrc/remesh.hip, operation for operation in fp32 (numpy rounds every
operation once and never fuses a multiply-add, which is what the kernels' `#pragma clang fp contract(off)` gives).  Sequential
loops: meant for meshes of a few thousand faces.  The surface-distance check uses closest_point_oracle.brute_force_closest."""
import numpy as np

from closest_point_oracle import brute_force_closest, MISS_INDEX

f32 = np.float32
SENTINEL = np.int64(0x7fffffffffffffff)
MAX_RING = 32


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def dist2(a, b):
    e = a - b
    return dot(e, e)


def normal(a, b, c):
    return cross(b - a, c - a)


def face_points(a, b, c):
    return np.stack([((a + b) + c) / f32(3), (a + b) * f32(0.5), (b + c) * f32(0.5), (c + a) * f32(0.5)])


class Tables:
    def __init__(self, V, F):
        self.V, self.F = np.asarray(V, f32), np.asarray(F, np.int32)
        F = self.F.astype(np.int64)
        nf, nv = len(F), len(V)
        a, b = F, np.roll(F, -1, axis=1)
        keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
        keys[F[:, 0] < 0] = SENTINEL
        keys = keys.reshape(-1)
        perm = np.argsort(keys, kind='stable')
        sk = keys[perm]
        nh = 3 * nf
        self.E = np.tile(np.array([-1, -1, 0, 1], np.int64), (nh, 1))
        self.he_edge = np.full(nh, -1, np.int64)
        self.vlock = np.zeros(nv, bool)
        self.vbound = np.zeros(nv, bool)
        i = 0
        while i < nh:
            j = i
            while j < nh and sk[j] == sk[i]:
                j += 1
            if sk[i] != SENTINEL:
                n = j - i
                self.he_edge[perm[i:j]] = i
                h0, h1 = perm[i], perm[i + 1] if n >= 2 else -1
                lock = n != 2 or self.F.reshape(-1)[h0] == self.F.reshape(-1)[h1]
                self.E[i] = [h0, h1, n, int(lock)]
                va, vb = int(sk[i] >> 32), int(sk[i] & 0xffffffff)
                if lock:
                    self.vlock[[va, vb]] = True
                if n == 1:
                    self.vbound[[va, vb]] = True
            i = j
        flat = self.F.reshape(-1)
        cperm = np.argsort(flat, kind='stable')
        self.vc_off = np.searchsorted(flat[cperm], np.arange(nv + 1), 'left')
        self.vc_corner = cperm

    def faces_of(self, v):
        return [int(c) // 3 for c in self.vc_corner[self.vc_off[v]:self.vc_off[v + 1]]]

    def deg(self, v):
        return int(self.vc_off[v + 1] - self.vc_off[v])

    def adjacent(self, v, x):
        return any(x in self.F[g] for g in self.faces_of(v))

    def quad(self, e):
        h0, h1, n, lock = (int(x) for x in self.E[e])
        if n != 2 or lock:
            return None
        f0, s0, f1, s1 = h0 // 3, h0 % 3, h1 // 3, h1 % 3
        F = self.F
        return (int(F[f0, s0]), int(F[f0, (s0 + 1) % 3]), int(F[f0, (s0 + 2) % 3]), int(F[f1, (s1 + 2) % 3]), f0, f1)


def split(V, F, max_len2):
    T = Tables(V, F)
    V, F = T.V, T.F
    nh = 3 * len(F)
    eflag = np.zeros(nh, np.int64)
    for e in range(nh):
        h0, _, n, lock = T.E[e]
        if n > 0 and not lock:
            f, s = h0 // 3, h0 % 3
            eflag[e] = dist2(V[F[f, s]], V[F[f, (s + 1) % 3]]) > f32(max_len2)
    voff = np.cumsum(eflag) - eflag
    newV = [V]
    for e in np.nonzero(eflag)[0]:
        f, s = T.E[e, 0] // 3, T.E[e, 0] % 3
        newV.append(((V[F[f, s]] + V[F[f, (s + 1) % 3]]) * f32(0.5))[None])
    nv = len(V)
    out = []
    for f in range(len(F)):
        v = [int(x) for x in F[f]]
        es = [T.he_edge[3 * f + s] for s in range(3)]
        mid = [nv + int(voff[e]) if eflag[e] else -1 for e in es]
        mask = sum(int(eflag[e]) << s for s, e in enumerate(es))
        n = bin(mask).count('1')
        if n == 0:
            out.append(v)
        elif n == 1:
            r = [1, 2, 4].index(mask)
            a, b, c, m = v[r], v[(r + 1) % 3], v[(r + 2) % 3], mid[r]
            out += [[a, m, c], [m, b, c]]
        elif n == 2:
            r = [1, 2, 4].index(~mask & 7)
            a, b, c, mbc, mca = v[r], v[(r + 1) % 3], v[(r + 2) % 3], mid[(r + 1) % 3], mid[(r + 2) % 3]
            out += [[a, b, mbc], [a, mbc, mca], [mbc, c, mca]]
        else:
            out += [[v[0], mid[0], mid[2]], [mid[0], v[1], mid[1]], [mid[2], mid[1], v[2]], [mid[0], mid[1], mid[2]]]
    return np.concatenate(newV).astype(f32), np.asarray(out, np.int32).reshape(-1, 3)


def collapse_eval(T, e, min_len2, max_len2):
    """-> (query points [n, 3], (keep, p)) of a collapse candidate, or None."""
    q = T.quad(e)
    if q is None or q[2] == q[3]:
        return None
    a, b, c, d, _, _ = q
    V, F = T.V, T.F
    la, lb = T.vlock[a], T.vlock[b]
    if la and lb:
        return None
    if not dist2(V[a], V[b]) < f32(min_len2):
        return None
    if T.deg(c) <= 3 or T.deg(d) <= 3:
        return None
    p = V[a] if la else V[b] if lb else (V[a] + V[b]) * f32(0.5)
    for g in T.faces_of(a):
        for x in F[g]:
            if x in (a, b, c, d):
                continue
            if T.adjacent(b, x):
                return None
    pts = []
    for v, o in ((a, b), (b, a)):
        for g in T.faces_of(v):
            if o in F[g]:
                continue
            x = [V[u] for u in F[g]]
            y = [p if u == v else V[u] for u in F[g]]
            for u, xt in zip(F[g], x):
                if u != v and dist2(p, xt) > f32(max_len2):
                    return None
            no, nn = normal(*x), normal(*y)
            if not dot(nn, nn) > 0:
                return None
            if dot(no, no) > 0 and not dot(no, nn) > 0:
                return None
            if len(pts) >= MAX_RING:
                return None
            pts.append(face_points(*y))
    keep = b if lb else a
    return np.concatenate(pts), (keep, p)


def flip_eval(T, e, cos2):
    """-> (query points [8, 3], gain) of a flip candidate, or None."""
    q = T.quad(e)
    if q is None or q[2] == q[3]:
        return None
    a, b, c, d, _, _ = q
    before = after = 0
    for i, (v, dv) in enumerate(((a, -1), (b, -1), (c, 1), (d, 1))):
        val = T.deg(v) + int(T.vbound[v])
        tgt = 4 if T.vbound[v] else 6
        if i < 2 and val <= 3:
            return None
        before += abs(val - tgt)
        after += abs(val + dv - tgt)
    if after >= before or T.adjacent(c, d):
        return None
    V = T.V
    ns = [normal(V[a], V[b], V[c]), normal(V[b], V[a], V[d])]
    ms = [normal(V[a], V[d], V[c]), normal(V[d], V[b], V[c])]
    for m in ms:
        mm = dot(m, m)
        if not mm > 0:
            return None
        for n in ns:
            nn = dot(n, n)
            if not nn > 0:
                continue
            dn = dot(m, n)
            if not dn > 0 or dn * dn < f32(cos2) * (mm * nn):
                return None
    return np.concatenate([face_points(V[a], V[d], V[c]), face_points(V[d], V[b], V[c])]), before - after


def round_winners(kind, V, F, V0, F0, params, max_d2):
    """-> (T, {edge id: eval result}) of the winners of one round: candidates whose points all lie within max_d2 of (V0, F0),
    claimed with their keys over their vertex sets (a min, so no order)."""
    T = Tables(V, F)
    cands = {}
    for e in range(3 * len(T.F)):
        r = collapse_eval(T, e, *params) if kind == 'collapse' else flip_eval(T, e, *params)
        if r is not None:
            cands[e] = r
    if cands:
        allp = np.concatenate([r[0] for r in cands.values()])
        idx = brute_force_closest(V0, F0, allp, max_d2)[1]
    claim = {}
    keys, rings, i = {}, {}, 0
    for e, r in cands.items():
        n = len(r[0])
        ok = bool((idx[i:i + n] != MISS_INDEX).all())
        i += n
        if not ok:
            continue
        a, b, c, d, _, _ = T.quad(e)
        if kind == 'collapse':
            hi = int(np.float32(dist2(T.V[a], T.V[b])).view(np.int32))
            ring = [int(u) for v in (a, b) for g in T.faces_of(v) for u in T.F[g]]
        else:
            hi = 16 - r[1]
            ring = [a, b, c, d]
        keys[e] = (hi << 32) | e
        rings[e] = ring
        for u in ring:
            claim[u] = min(claim.get(u, 1 << 64), keys[e])
    win = {e: cands[e] for e in keys if all(claim[u] == keys[e] for u in rings[e])}
    return T, win


def collapse_apply(T, win):
    V, F = T.V.copy(), T.F.copy()
    for e, (_, (keep, p)) in win.items():
        a, b = T.quad(e)[:2]
        rem = a if keep == b else b
        V[keep] = p
        for g in T.faces_of(rem):
            if keep in F[g]:
                F[g] = -1
            else:
                F[g][F[g] == rem] = keep
    return V, F


def flip_apply(T, win):
    F = T.F.copy()
    for e in win:
        a, b, c, d, f0, f1 = T.quad(e)
        F[f0] = [a, d, c]
        F[f1] = [d, b, c]
    return F


def relax(V, F):
    T = Tables(V, F)
    V = T.V
    out = V.copy()
    for v in range(len(V)):
        if T.vlock[v] or T.deg(v) == 0:
            continue
        p = V[v]
        sc, N, sw = np.zeros(3, f32), np.zeros(3, f32), f32(0)
        for g in T.faces_of(v):
            x, y, z = V[T.F[g, 0]], V[T.F[g, 1]], V[T.F[g, 2]]
            n = normal(x, y, z)
            w = np.sqrt(dot(n, n))
            sc = sc + (((x + y) + z) / f32(3)) * w
            N = N + n
            sw = f32(sw + w)
        if not sw > 0:
            continue
        dv = sc / sw - p
        nn = dot(N, N)
        if nn > 0:
            t = dot(N, dv) / nn
            dv = dv - N * t
        out[v] = p + dv
    return out


def project(V, F, V0, F0):
    T = Tables(V, F)
    q = brute_force_closest(V0, F0, T.V)[2]
    return np.where(T.vlock[:, None], T.V, q).astype(f32)
