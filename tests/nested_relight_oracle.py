"""Float64 numpy restatement of the nested-object transport, independent of nu_nerf_amd/csrc: the interface event, the
step that leaves the shell, the interior chain over a brute-force tracer, and the resolve sum fed the device's records.  Builds on
relight_oracle (sample sequence, weights, environment, G-buffer rows).  No GPU, no torch."""
import numpy as np

import relight_oracle as O

DARK, INNER, EXIT = 0, 1, 2
TIR_K2 = 0.999


def box(half=0.4):
    """Axis-aligned box [-half, half]^3 with per-face vertices: 24 vertices, 12 faces, outward winding (flat normals)."""
    V, F = [], []
    for ax in range(3):
        for sg in (-1.0, 1.0):
            u, v = (ax + 1) % 3, (ax + 2) % 3
            base = len(V)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[ax], p[u], p[v] = sg * half, a * half, b * half
                V.append(p)
            F += [(base, base + 1, base + 2), (base, base + 2, base + 3)] if sg > 0 else [(base, base + 2, base + 1), (base, base + 3, base + 2)]
    return np.array(V, np.float32), np.array(F, np.int32)


# ---- the interface event ---------------------------------------------------------------------------------------------------------------
def interface(d, ns, ior, entering):
    """d, ns [N,3] unit, ior [N], entering bool (scalar or [N]) -> dict: refr [N] bool, n (ns oriented against d), dn (refracted, or
    mirrored on total internal reflection), F (Schlick with the air-side cosine; 1 on total internal reflection; 0 throughout where
    ior = 1), k2 = eta^2 sin^2_i (the quantity the decision compares with 0.999), cos_i, cos_t."""
    d, ns, ior = np.asarray(d, np.float64), np.asarray(ns, np.float64), np.asarray(ior, np.float64)
    entering = np.broadcast_to(np.asarray(entering, bool), ior.shape)
    n = np.where((np.sum(ns * d, 1) > 0)[:, None], -ns, ns)
    cos_i = -np.sum(n * d, 1)
    sin2 = 1.0 - cos_i * cos_i
    eta = np.where(entering, 1.0 / ior, ior)
    k2 = eta * eta * sin2
    refr = ~(k2 > TIR_K2)
    cos_t = np.sqrt(np.maximum(1.0 - k2, 0.0))
    t = eta[:, None] * d + (eta * cos_i - cos_t)[:, None] * n
    with np.errstate(invalid='ignore', divide='ignore'):
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
    mirror = d + (2.0 * cos_i)[:, None] * n
    f0 = ((ior - 1.0) / (ior + 1.0)) ** 2
    c = np.where(entering, cos_i, cos_t)
    F = np.where(refr, f0 + (1.0 - f0) * np.maximum(1.0 - c, 0.0) ** 5, 1.0)
    F = np.where(f0 > 0, F, 0.0)
    return dict(refr=refr, n=n, dn=np.where(refr[:, None], t, mirror), F=F, k2=k2, cos_i=cos_i, cos_t=cos_t)


def surface(V, F, VN, o, d, face):
    """(x, n_g facing the viewer, n_s on its side, (w0, u, v)) at the hit of rays (o, d) with faces `face`."""
    rows = O.gbuffer_rows(V, F, VN, np.zeros((V.shape[0], 5)), o, d, face, np.zeros(len(face)), np.zeros(len(face)))
    f = F[face]
    u, v, _, _ = O.barycentrics(o, d, V[f[:, 0]], V[f[:, 1]], V[f[:, 2]])
    return rows[:, 1:4], rows[:, 4:7], rows[:, 7:10], np.stack([1.0 - u - v, u, v], 1)


def leave(V, F, VN, ior_v, o, d, face, eps):
    """The ray (o, d) meets `face` of the outer mesh from inside -> dict of interface() plus o2: the exit origin x - eps n_g where it
    refracts, the restart x + eps n_g where it is totally reflected (n_g faces the ray, i.e. points inside), and the index used."""
    x, ng, ns, bary = surface(V, F, VN, o, d, face)
    index = 1.0 + np.sum(bary * (ior_v[F[face]] - 1.0), 1)
    ev = interface(d, ns, index, False)
    ev['o2'] = np.where(ev['refr'][:, None], x - eps * ng, x + eps * ng)
    ev['ior'] = index
    return ev


def entry(rows):
    """The entry event of outer G-buffer rows (float64 [N,20], index of refraction minus 1 in [10]) -> interface() plus the reflection
    direction r, whether the reflection ray is traced, and the start of the interior chain."""
    d = -rows[:, 15:18]
    ev = interface(d, rows[:, 7:10], 1.0 + rows[:, 10], True)
    r = d + (2.0 * ev['cos_i'])[:, None] * ev['n']
    ev['r'] = np.where(ev['refr'][:, None], r, ev['dn'])
    ev['refl_traced'] = (ev['F'] > 0) & (np.sum(ev['n'] * ev['r'], 1) > 0) & (np.sum(rows[:, 4:7] * ev['r'], 1) > 0)
    return ev


# ---- the interior chain over the brute-force tracer -----------------------------------------------------------------------------------------
def chain(outer, inner, ior_v, rows, eps, K=4):
    """outer / inner = (V, F, VN) float64 / int64.  rows [N,20] outer G-buffer rows.  -> kind [N], T [N], exit direction [N,3], exit
    visibility [N], reflection (direction, F, visibility), inner (origin, direction, face) of inner pixels, and `margin` [N]: the
    smallest |eta^2 sin^2 - 0.999| met along the path."""
    N = rows.shape[0]
    Vo, Fo, VNo = outer
    Vi, Fi, _ = inner
    ev = entry(rows)
    margin = np.abs(ev['k2'] - TIR_K2)
    kind, T = np.zeros(N, np.int64), np.where(ev['refr'], 1.0 - ev['F'], 0.0)
    exit_d, exit_vis, refl_vis = np.zeros((N, 3)), np.zeros(N), np.zeros(N)
    in_o, in_d, in_f = np.zeros((N, 3)), np.zeros((N, 3)), np.full(N, O.MISS, np.int64)
    x0, ng0 = rows[:, 1:4], rows[:, 4:7]
    tr = np.flatnonzero(ev['refl_traced'])
    if len(tr):
        refl_vis[tr] = ~O.brute_trace(Vo, Fo, x0[tr] + eps * ng0[tr], ev['r'][tr])[0]
    live = np.flatnonzero(ev['refr'])
    o, d = (x0 - eps * ng0)[live], ev['dn'][live]
    for _ in range(K):
        if not len(live):
            break
        hi, fi, ti = O.brute_trace(Vi, Fi, o, d)
        ho, fo, to = O.brute_trace(Vo, Fo, o, d)
        ends = hi & (~ho | (ti <= to))
        idx = live[ends]
        kind[idx], in_o[idx], in_d[idx], in_f[idx] = INNER, o[ends], d[ends], fi[ends]
        leak = ~ends & ~ho
        idx = live[leak]
        kind[idx], exit_d[idx], exit_vis[idx] = EXIT, d[leak], 1.0
        at = ~ends & ho
        lv = leave(Vo, Fo, VNo, ior_v, o[at], d[at], fo[at], eps)
        idx = live[at]
        margin[idx] = np.minimum(margin[idx], np.abs(lv['k2'] - TIR_K2))
        out = lv['refr']
        T[idx[out]] *= 1.0 - lv['F'][out]
        kind[idx[out]], exit_d[idx[out]] = EXIT, lv['dn'][out]
        if out.any():
            exit_vis[idx[out]] = ~O.brute_trace(Vo, Fo, lv['o2'][out], lv['dn'][out])[0]
        live, o, d = idx[~out], lv['o2'][~out], lv['dn'][~out]
    T[kind == DARK] = 0.0
    return dict(kind=kind, T=T, exit_d=exit_d, exit_vis=exit_vis, refl_d=ev['r'], F=ev['F'], refl_vis=refl_vis, in_o=in_o, in_d=in_d,
                in_f=in_f, margin=margin)


# ---- resolve ---------------------------------------------------------------------------------------------------------------------------
def resolve(kind, chain_rec, irows, img, pixel, rec, S, seed, env):
    """Linear RGB [N,3] from the device's records: kind [N], chain_rec [N,12] (T, exit direction, exit visibility, reflection direction,
    F, reflection visibility), inner rows [N,20], rec [N,S,4] (exit direction, 1 - F_exit; zero = dark; rows of non-inner pixels
    ignored)."""
    N = len(kind)
    out = np.zeros((N, 3))
    s = np.arange(S)
    T = chain_rec[:, 0]
    for i in np.flatnonzero(kind == INNER):
        lit = rec[i, :, 3] != 0
        if not lit.any():
            continue
        lobe, b1, b2 = O.sample_bits(img[i], pixel[i], seed, S, s[lit])
        r = np.repeat(irows[i:i + 1], int(lit.sum()), 0)
        l, h, _ = O.sample_dirs(r, lobe, b1, b2)
        w = O.weights(r, lobe, l, h) * rec[i, lit, 3:4]
        out[i] = T[i] * np.sum(w * O.env_lookup(env, rec[i, lit, :3]), 0) * (2.0 / S)
    refl = (chain_rec[:, 8] > 0) & (chain_rec[:, 9] > 0)
    out[refl] += chain_rec[refl, 8:9] * O.env_lookup(env, chain_rec[refl, 5:8])
    ex = (kind == EXIT) & (chain_rec[:, 4] > 0)
    out[ex] += T[ex, None] * O.env_lookup(env, chain_rec[ex, 1:4])
    return out
