"""Float64 numpy restatement of the thin-shell transport, independent of nu_nerf_amd/csrc: the wall crossing with its
Fresnel factors and the distance of every decision from its branch point, the leaving step, the one-segment camera chain over the
brute-force tracer.  The crossing GEOMETRY is pinned against oracle/stage2_oracle.shell_refraction (cross_ref feeds it the logits of
the baked values); the resolve sum is nested_relight_oracle.resolve, unchanged.  No GPU."""
import numpy as np

import nested_relight_oracle as NO
import relight_oracle as O

DARK, INNER, EXIT = NO.DARK, NO.INNER, NO.EXIT
CAVITY = 1.0001
TIR = 0.999
CLAMP = 1e-4

# what the GPU and the host tests share
MARGIN, MARGIN_CAP = 1e-4, 0.02  # decisions within MARGIN of a branch point are left out of float64 comparisons, at most MARGIN_CAP of them
N_ROWS, N_FLAT = 4096, 64       # rows per direction of the crossing tests, and the flat rows (|curvature| < 1e-6, half of them 0) added
INNER_C = np.array([0.1, 0.0, 0.05], np.float32)
TORUS_INNER_C, TORUS_INNER_R = np.array([0.35, 0.0, 0.0], np.float32), 0.1
SCENES = {'ico2': (40, 40), 'ico3': (64, 64), 'torus': (64, 64), 'ico7': (32, 32)}


def logits(ior, thickness):
    """The pre-sigmoid values shell_refraction takes for a baked (index, thickness): index = sigmoid + 0.6, thickness = 0.01 sigmoid."""
    def logit(p):
        p = np.clip(np.asarray(p, np.float64), 1e-300, 1.0 - 1e-15)
        return np.log(p) - np.log1p(-p)
    return logit(np.asarray(ior, np.float64) - 0.6), logit(np.asarray(thickness, np.float64) / 0.01)


def cross_ref(d, n_out, x, ior, thickness, gk, inside):
    """oracle/stage2_oracle.shell_refraction in float64 on the logits of (ior, thickness) -> its dict as numpy arrays."""
    import torch
    from oracle.stage2_oracle import shell_refraction
    ior_raw, th_raw = logits(ior, thickness)
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float64)) for a in (d, n_out, x, ior_raw, gk, th_raw)]
    with torch.no_grad():
        out = shell_refraction(*t, bool(inside))
    return {k: v.numpy() for k, v in out.items()}


def schlick(n_in, n_out, c_in, c_out):
    """Schlick reflectance of a face between n_in (cosine c_in on that side) and n_out (c_out): the cosine of the lower-index side."""
    f0 = ((n_in - n_out) / (n_in + n_out)) ** 2
    m = np.clip(1.0 - np.where(n_in <= n_out, c_in, c_out), 0.0, 1.0)
    return np.where(f0 > 0, f0 + (1.0 - f0) * m ** 5, 0.0)


def _unit_eps(v):
    return v / (np.sqrt(np.sum(v * v, 1, keepdims=True)) + 1e-4)


def cross(d, n_out, x, ior, thickness, gk, inside, dtype=np.float64):
    """The crossing of M rows: d [M,3] unit, n_out [M,3] the OUTWARD shading normal, x [M,3], ior / thickness / gk [M].  -> dict:
    refracts, tir_ok [M] bool, normal, end, next_start, next_dir [M,3] (shell_refraction's names and conventions: rows that do not
    refract hold end = x and zeros), F_a, F_b [M] (the first / second face; !refracts: F_a = 1, or 0 when the first face is
    index-matched, F_b = 0), keep = (1 - F_a)(1 - F_b), margin1 [M] = the distance of the FIRST face's decisions from their branch
    points (the 0.999 test(s), the 1e-4 clamps of 1 - sin^2_t and -- leaving -- of the step-back discriminant) and margin [M] = that of
    every decision (adds the chord discriminant and the second face).  dtype=np.float32 runs the same operations in single precision
    (an estimate of the device's rounding; not a reference)."""
    f = dtype
    d, n_out, x = (np.asarray(a, f) for a in (d, n_out, x))
    n_g, th, gk = (np.asarray(a, f).reshape(-1, 1) for a in (ior, thickness, gk))
    one = f(1.0)
    nrm = n_out / np.maximum(np.sqrt(np.sum(n_out * n_out, 1, keepdims=True)), f(1e-12))
    if inside:
        nrm = -nrm
    r = one / n_g
    ro = (one / f(CAVITY)) / r
    if inside:
        r, ro = one / ro, one / r
    n_first_in, n_last_out = (f(CAVITY), one) if inside else (one, f(CAVITY))
    cos_i = -np.sum(nrm * d, 1, keepdims=True)
    sin2_i = one - cos_i * cos_i
    k2 = r * r * sin2_i
    refr = ~(k2 > f(TIR))
    tir = refr.copy()
    sin2_t = sin2_i * r * r
    with np.errstate(invalid='ignore', divide='ignore'):
        R = one / np.sqrt(np.maximum(np.abs(gk), f(1e-6)))
    R = np.where(np.isnan(R), f(0.1), R)
    cos_t = np.sqrt(np.maximum(one - sin2_t, f(CLAMP)))
    positive = (gk <= 0) if inside else (gk >= 0)
    margin1 = np.minimum(np.abs(k2 - f(TIR)), np.abs(one - sin2_t - f(CLAMP)))

    def chord(c):
        d2 = np.where(positive, c * c - R * th * f(2.0) + th * th, c * c + R * th * f(2.0) + th * th)
        return np.abs(c - np.sqrt(np.maximum(d2, f(CLAMP)))), np.abs(d2 - f(CLAMP))
    if not inside:
        d_in = _unit_eps(r * d + (r * cos_i - cos_t) * nrm)
        pm, nm = x, nrm
        F_a = schlick(n_first_in, n_g, cos_i, cos_t)
    else:
        length, m_d = chord(R * cos_i)
        center = np.where(positive, x - nrm * R, x + nrm * R)
        pm = x - length * d
        nm = _unit_eps(np.where(positive, pm - center, center - pm))
        cos_im = -np.sum(nm * d, 1, keepdims=True)
        xx = (one - cos_im * cos_im) * r * r
        tir &= ~(xx > f(TIR))
        cos_tm = np.sqrt(np.maximum(one - np.minimum(xx, f(TIR)), f(CLAMP)))
        d_in = _unit_eps(r * d + (r * cos_im - cos_tm) * nm)
        F_a = schlick(n_first_in, n_g, cos_im, cos_tm)
        margin1 = np.minimum(margin1, np.minimum(m_d, np.abs(xx - f(TIR))))
    length, m_d = chord(R * cos_t)
    center = np.where(positive, pm - nm * R, pm + nm * R)
    next_start = pm + d_in * (length + f(0.001))
    n_after = _unit_eps(np.where(positive, next_start - center, center - next_start))
    cos_i2 = -np.sum(n_after * d_in, 1, keepdims=True)
    x2 = (one - cos_i2 * cos_i2) * ro * ro
    tir &= ~(x2 > f(TIR))
    cos_t2 = np.sqrt(np.maximum(one - np.minimum(x2, f(TIR)), f(CLAMP)))
    next_dir = _unit_eps(ro * d_in + (ro * cos_i2 - cos_t2) * n_after)
    F_b = schlick(n_g, n_last_out, cos_i2, cos_t2)
    margin = np.minimum(margin1, np.minimum(m_d, np.abs(x2 - f(TIR))))
    f0_first = ((n_first_in - n_g) / (n_first_in + n_g)) ** 2
    F_a = np.where(refr, F_a, np.where(f0_first > 0, one, f(0.0)))
    F_b = np.where(refr, F_b, f(0.0))
    z = np.zeros_like(x)
    # a row that does not refract stops at the first test: nothing later is decided for it
    margin = np.where(refr, margin, np.abs(k2 - f(TIR)))
    margin1 = np.where(refr, margin1, np.abs(k2 - f(TIR)))
    return dict(refracts=refr[:, 0], tir_ok=(tir & refr)[:, 0], normal=nrm, end=np.where(refr, pm, x), next_start=np.where(refr, next_start, z),
                next_dir=np.where(refr, next_dir, z), F_a=F_a[:, 0], F_b=F_b[:, 0], keep=((one - F_a) * (one - F_b))[:, 0],
                margin1=margin1[:, 0], margin=margin[:, 0])


def random_rows(n, inside, seed, flat=64):
    """The rows of the crossing tests: random unit normals, d on the proper side (against the outward normal when entering, along it
    when leaving), points in the unit ball, index 0.7 .. 1.6, thickness 0.002 .. 0.01, curvature uniform in [-10, 10]; the last
    `flat` rows have |gk| < 1e-6, half of them gk = 0."""
    g = np.random.Generator(np.random.PCG64(seed))
    nrm = g.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.sum(d * nrm, 1)
    d = np.where(((s > 0) != bool(inside))[:, None], -d, d)
    x = g.uniform(-0.5, 0.5, (n, 3))
    ior, th, gk = g.uniform(0.7, 1.6, n), g.uniform(0.002, 0.01, n), g.uniform(-10.0, 10.0, n)
    gk[n - flat:] = g.uniform(-1e-6, 1e-6, flat)
    gk[n - flat // 2:] = 0.0
    return tuple(np.ascontiguousarray(a, np.float32) for a in (d, nrm, x, ior, th, gk))


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def torus(nu=32, nv=16, R=0.35, r=0.15):
    """Parametric torus about the z axis, nu x nv quads split into 2 nu nv triangles, outward winding."""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    V = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, e = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    F = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, e], -1).reshape(-1, 3)], 0)
    return V.astype(np.float32), F.astype(np.int32)


def meshes(name):
    """(V_o, F_o, ior [V_o], thickness [V_o], V_i, F_i, materials_i) of a test scene: index 0.7 .. 1.6 and thickness 0.002 .. 0.01 over
    the surface of an icosphere ('ico<subdivisions>', radius 0.5) or of the torus, around an 80-face inner sphere."""
    from nu_nerf_amd.lbvh import icosphere
    if name == 'torus':
        Vo, Fo = torus()
        Vi, Fi = icosphere(1, TORUS_INNER_R)
        Vi = Vi + TORUS_INNER_C
        th = 0.006 + 0.008 * Vo[:, 1]
    else:
        Vo, Fo = icosphere(int(name[3:]), 0.5)
        Vi, Fi = icosphere(1, 0.2)
        Vi = Vi + INNER_C
        th = 0.006 + 0.008 * Vo[:, 2]
    ior = 1.15 + 0.9 * Vo[:, 0]
    g = np.random.Generator(np.random.PCG64(5))
    return (Vo, Fo, ior.astype(np.float32), th.astype(np.float32), Vi.astype(np.float32), Fi,
            g.uniform(0.05, 0.95, (len(Vi), 5)).astype(np.float32))


def poses(name):
    """The one camera of a test scene: world -> camera [1,3,4]."""
    from nu_nerf_amd import relight as R
    return R.camera_in_mesh_frame(R.relighting_poses(3, 20.0, 30.0, 2.2))[1:2]


# ---- transport ---------------------------------------------------------------------------------------------------------------------------
def leave(V, F, VN, ior_v, th_v, gk_v, o, d, face, eps):
    """The cavity ray (o, d) meets `face` of the outer mesh -> cross(inside=True) with the values interpolated at the hit (the index as
    1 + sum w (n - 1)) plus o2 = next_start pushed eps along the outward geometric normal, out = refracts & tir_ok."""
    x, ng, ns, bary = NO.surface(V, F, VN, o, d, face)
    f = F[face]
    index = 1.0 + np.sum(bary * (ior_v[f] - 1.0), 1)
    th, gk = np.sum(bary * th_v[f], 1), np.sum(bary * gk_v[f], 1)
    ev = cross(d, -ns, x, index, th, gk, True)
    ev['o2'] = ev['next_start'] - eps * ng
    ev['out'] = ev['refracts'] & ev['tir_ok']
    ev['ior'], ev['th'], ev['gk'] = index, th, gk
    return ev


def entry(rows):
    """The entry crossing of outer G-buffer rows (float64 [N,20]; index - 1, thickness, curvature in [10], [11], [12]) -> cross() plus
    the reflection direction r off the first face, whether the reflection ray is traced, and enters = refracts & tir_ok."""
    d = -rows[:, 15:18]
    ev = cross(d, rows[:, 7:10], rows[:, 1:4], 1.0 + rows[:, 10], rows[:, 11], rows[:, 12], False)
    c = -np.sum(ev['normal'] * d, 1)
    ev['r'] = d + (2.0 * c)[:, None] * ev['normal']
    ev['refl_traced'] = (ev['F_a'] > 0) & (np.sum(ev['normal'] * ev['r'], 1) > 0) & (np.sum(rows[:, 4:7] * ev['r'], 1) > 0)
    ev['enters'] = ev['refracts'] & ev['tir_ok']
    return ev


def chain(outer, inner, ior_v, th_v, gk_v, rows, eps):
    """The one-segment camera chain over the brute-force tracer.  outer / inner = (V, F, VN) float64 / int64, rows [N,20] outer G-buffer
    rows.  -> kind, T, exit direction / visibility, reflection (direction, F, visibility), the cavity ray and the inner face of inner
    pixels, margin [N] = the smallest distance from a branch point met along the path."""
    N = rows.shape[0]
    Vo, Fo, VNo = outer
    Vi, Fi, _ = inner
    ev = entry(rows)
    margin = ev['margin'].copy()
    kind, T = np.zeros(N, np.int64), np.where(ev['enters'], ev['keep'], 0.0)
    exit_d, exit_vis, refl_vis = np.zeros((N, 3)), np.zeros(N), np.zeros(N)
    in_f = np.full(N, O.MISS, np.int64)
    x0, ng0 = rows[:, 1:4], rows[:, 4:7]
    tr = np.flatnonzero(ev['refl_traced'])
    if len(tr):
        refl_vis[tr] = ~O.brute_trace(Vo, Fo, x0[tr] + eps * ng0[tr], ev['r'][tr])[0]
    live = np.flatnonzero(ev['enters'])
    o, d = ev['next_start'][live], ev['next_dir'][live]
    if len(live):
        hi, fi, ti = O.brute_trace(Vi, Fi, o, d)
        ho, fo, to = O.brute_trace(Vo, Fo, o, d)
        ends = hi & (~ho | (ti <= to))
        kind[live[ends]], in_f[live[ends]] = INNER, fi[ends]
        leak = ~ends & ~ho
        kind[live[leak]], exit_d[live[leak]], exit_vis[live[leak]] = EXIT, d[leak], 1.0
        at = ~ends & ho
        lv = leave(Vo, Fo, VNo, ior_v, th_v, gk_v, o[at], d[at], fo[at], eps)
        idx = live[at]
        margin[idx] = np.minimum(margin[idx], lv['margin'])
        out = lv['out']
        T[idx[out]] *= lv['keep'][out]
        kind[idx[out]], exit_d[idx[out]] = EXIT, lv['next_dir'][out]
        if out.any():
            exit_vis[idx[out]] = ~O.brute_trace(Vo, Fo, lv['o2'][out], lv['next_dir'][out])[0]
    T[kind == DARK] = 0.0
    return dict(kind=kind, T=T, exit_d=exit_d, exit_vis=exit_vis, refl_d=ev['r'], F=ev['F_a'], refl_vis=refl_vis, cav_o=ev['next_start'],
                cav_d=ev['next_dir'], in_f=in_f, margin=margin)
