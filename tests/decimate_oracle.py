"""Numpy / plain-Python port of the decimation round of nu_nerf_amd/csrc/decimate.hip and of the driver's loop
(nu_nerf_amd/decimate.py), operation for operation in float64: Python floats round every operation once and never fuse a
multiply-add, which is what the kernels' `#pragma clang fp contract(off)` gives; math.sqrt and / are correctly rounded.  Sequential
loops: meant for meshes of a few thousand faces.  No surface bound (the kernels' bound is checked through mesh_distance).
winners(hold='ring') is the hold-everything rule of the remeshing collapse, kept to count the rounds the narrower hold set saves."""
import math

import numpy as np

from remesh_oracle import Tables, MAX_RING

NO_KEY = 0x7fffffffffffffff
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]          # the ten unique entries, in storage order


def mix32(h):
    h &= 0xffffffff
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xffffffff
    h ^= h >> 16
    return h


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def dist2(a, b):
    e = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    return dot(e, e)


def normal(a, b, c):
    u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    w = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


class Mesh:
    """The tables of (V, F) with plain-Python copies: P (float64 positions), faces, the CSR as lists."""

    def __init__(self, V, F):
        self.T = Tables(V, F)
        self.P = [tuple(r) for r in self.T.V.astype(np.float64).tolist()]
        self.F = self.T.F.tolist()
        off, cor = self.T.vc_off.tolist(), self.T.vc_corner.tolist()
        self.faces_of = [[c // 3 for c in cor[off[v]:off[v + 1]]] for v in range(len(self.P))]
        self.vlock = self.T.vlock.tolist()
        self.nh = 3 * len(self.F)


def plane_terms(M, v):
    """[(w, (n^x, n^y, n^z, d))] of the faces of v with non-zero area, in corner order."""
    out = []
    for g in M.faces_of[v]:
        p0, p1, p2 = (M.P[u] for u in M.F[g])
        n = normal(p0, p1, p2)
        nn = dot(n, n)
        if not nn > 0.0:
            continue
        ln = math.sqrt(nn)
        pl = [n[0] / ln, n[1] / ln, n[2] / ln]
        pl.append(-dot(pl, p0))
        out.append((ln * 0.5, pl))
    return out


def quadrics(M):
    """Q [nv, 10] float64."""
    Q = np.zeros((len(M.P), 10))
    for v in range(len(M.P)):
        q = [0.0] * 10
        for w, pl in plane_terms(M, v):
            for k, (i, j) in enumerate(PAIRS):
                q[k] = q[k] + w * (pl[i] * pl[j])
        Q[v] = q
    return Q


def cost_at(s, x):
    a00, a01, a02, b0, a11, a12, b1, a22, b2, c = s
    ax0 = (a00 * x[0] + a01 * x[1]) + a02 * x[2]
    ax1 = (a01 * x[0] + a11 * x[1]) + a12 * x[2]
    ax2 = (a02 * x[0] + a12 * x[1]) + a22 * x[2]
    xax = (x[0] * ax0 + x[1] * ax1) + x[2] * ax2
    bx = (b0 * x[0] + b1 * x[1]) + b2 * x[2]
    return (xax + 2.0 * bx) + c


def solve(s):
    """(x, det, trace magnitude) of A x = -b by cofactors, or (None, det, tr) when |det| <= 1e-9 |tr|^3."""
    a00, a01, a02, b0, a11, a12, b1, a22, b2, _ = s
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    det = (a00 * c00 + a01 * c01) + a02 * c02
    tr = abs((a00 + a11) + a22)
    if not abs(det) > 1e-9 * ((tr * tr) * tr):
        return None, det, tr
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    r0, r1, r2 = -b0, -b1, -b2
    x = (((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det)
    return x, det, tr


def placement(s, pa, pb):
    """(x, 'solve' | 'a' | 'b' | 'm') for an edge with both ends free."""
    mid = tuple((pa[k] + pb[k]) * 0.5 for k in range(3))
    x = solve(s)[0]
    if x is not None and dist2(x, mid) <= dist2(pa, pb):
        return x, 'solve'
    best, x, how = cost_at(s, pa), pa, 'a'
    cb, cm = cost_at(s, pb), cost_at(s, mid)
    if cb < best:
        best, x, how = cb, pb, 'b'
    if cm < best:
        x, how = mid, 'm'
    return x, how


def eval_edge(M, Q, e, min_q2):
    """(npts, cost, pos fp32 [3]) of edge slot e, or None when it is rejected."""
    q = M.T.quad(e)
    if q is None or q[2] == q[3]:
        return None
    a, b, c, d, _, _ = q
    la, lb = M.vlock[a], M.vlock[b]
    if la and lb:
        return None
    if len(M.faces_of[c]) <= 3 or len(M.faces_of[d]) <= 3:
        return None
    s = [x + y for x, y in zip(Q[a].tolist(), Q[b].tolist())]
    pa, pb = M.P[a], M.P[b]
    x = pa if la else pb if lb else placement(s, pa, pb)[0]
    with np.errstate(over='ignore'):
        p = np.array(x, np.float64).astype(np.float32)
    xd = tuple(p.astype(np.float64).tolist())
    cst = cost_at(s, xd)
    if not math.isfinite(cst):
        return None
    cst = cst if cst > 0.0 else 0.0
    fb = M.faces_of[b]
    for g in M.faces_of[a]:
        for u in M.F[g]:
            if u in (a, b, c, d):
                continue
            if any(u in M.F[h] for h in fb):
                return None
    n = 0
    for v, o in ((a, b), (b, a)):
        for g in M.faces_of[v]:
            fg = M.F[g]
            if o in fg:
                continue
            xo = [M.P[u] for u in fg]
            y = [xd if u == v else M.P[u] for u in fg]
            no, nw = normal(*xo), normal(*y)
            nn_new, nn_old = dot(nw, nw), dot(no, no)
            if not nn_new > 0.0:
                return None
            if nn_old > 0.0 and not dot(no, nw) > 0.0:
                return None
            sn = (dist2(y[0], y[1]) + dist2(y[1], y[2])) + dist2(y[2], y[0])
            so = (dist2(xo[0], xo[1]) + dist2(xo[1], xo[2])) + dist2(xo[2], xo[0])
            if 12.0 * nn_new < min_q2 * (sn * sn) and nn_new * (so * so) < nn_old * (sn * sn):
                return None
            if n >= MAX_RING:
                return None
            n += 1
    if n == 0:
        return None
    return 7 * n, cst, p


def evaluate(M, Q, min_q2):
    """cost [nh] float64, pos [nh, 3] fp32, npts [nh] int32 (zeros at rejected slots)."""
    cost, pos, npts = np.zeros(M.nh), np.zeros((M.nh, 3), np.float32), np.zeros(M.nh, np.int32)
    for e in range(M.nh):
        r = eval_edge(M, Q, e, min_q2)
        if r is not None:
            npts[e], cost[e], pos[e] = r
    return cost, pos, npts


def cost_floor(V):
    V = np.asarray(V, np.float32)
    d = [float(V[:, k].max()) - float(V[:, k].min()) for k in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return 1e-12 * (d2 * d2)


def keys(cost, npts, floor):
    """[nh] int64: ((bits(float32(cost + floor)) >> 12) << 32) | mix32(e), NO_KEY at rejected slots."""
    out = np.full(len(cost), NO_KEY, np.int64)
    for e in np.nonzero(npts)[0]:
        hi = int(np.float32(float(cost[e]) + floor).view(np.uint32)) >> 12
        out[e] = (hi << 32) | mix32(int(e))
    return out


def threshold(ckey, ncand, need):
    """The k-th smallest key, k = min(candidates, need), at least 1."""
    k = max(min(int(ncand), int(need)), 1)
    return int(np.sort(ckey)[k - 1])


def ring(M, a, b):
    return [u for v in (a, b) for g in M.faces_of[v] for u in M.F[g]]


def winners(M, ckey, thr, hold='abcd'):
    """win [nh] int32: the competitors (key <= thr) write their key over their ring (every vertex of every face of a and b) and win
    when they hold the minimum at a, b, c and d -- or, with hold='ring', at every vertex of the ring."""
    comp = [int(e) for e in np.nonzero((ckey != NO_KEY) & (ckey <= thr))[0]]
    claim = {}
    for e in comp:
        a, b = M.T.quad(e)[:2]
        k = int(ckey[e])
        for u in ring(M, a, b):
            if claim.get(u, NO_KEY) > k:
                claim[u] = k
    win = np.zeros(M.nh, np.int32)
    for e in comp:
        q = M.T.quad(e)
        win[e] = all(claim[u] == int(ckey[e]) for u in (q[:4] if hold == 'abcd' else ring(M, q[0], q[1])))
    return win


def apply(M, win, pos):
    V, F = M.T.V.copy(), M.T.F.copy()
    for e in np.nonzero(win)[0]:
        a, b = M.T.quad(int(e))[:2]
        keep, rem = (b, a) if M.vlock[b] else (a, b)
        V[keep] = pos[e]
        for g in M.faces_of[rem]:
            if keep in F[g]:
                F[g] = -1
            else:
                F[g][F[g] == rem] = keep
    return V, F


def compact(V, F):
    Fk = F[F[:, 0] >= 0]
    used = np.zeros(len(V), bool)
    used[Fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.ascontiguousarray(V[used], np.float32), np.ascontiguousarray(remap[Fk], np.int32)


def one_round(V, F, need, floor, min_q2, hold='abcd'):
    """-> dict of everything a round computes on the compacted mesh (V, F)."""
    M = Mesh(V, F)
    Q = quadrics(M)
    cost, pos, npts = evaluate(M, Q, min_q2)
    ckey = keys(cost, npts, floor)
    ncand = int((npts > 0).sum())
    thr = threshold(ckey, ncand, need)
    win = winners(M, ckey, thr, hold)
    Vn, Fn = apply(M, win, pos)
    return dict(M=M, Q=Q, cost=cost, pos=pos, npts=npts, ckey=ckey, ncand=ncand, thr=thr, win=win, V=Vn, F=Fn)


def decimate(V, F, target, min_quality=0.1, max_rounds=256, tolerance=0.02, stats=None, hold='abcd'):
    floor = cost_floor(V)
    Vc, Fc = compact(np.asarray(V, np.float32), np.asarray(F, np.int32))
    nf = len(Fc)
    log = dict(rounds=0, faces_in=nf, converged=False, per_round=[], max_cost=0.0)
    if target < nf:
        while True:
            if nf <= target * (1.0 + tolerance) or nf - target < 2:
                log['converged'] = True
                break
            if log['rounds'] >= max_rounds:
                break
            r = one_round(Vc, Fc, (nf - target) // 2, floor, min_quality * min_quality, hold)
            nwin = int(r['win'].sum())
            log['per_round'].append((nf, r['ncand'], nwin))
            if nwin == 0:
                break
            log['max_cost'] = max(log['max_cost'], float(r['cost'][r['win'] > 0].max()))
            Vc, Fc = compact(r['V'], r['F'])
            nf = len(Fc)
            log['rounds'] += 1
    log['faces_out'] = len(Fc)
    if stats is not None:
        stats.update(log)
    return Vc, Fc
