"""Float64 numpy restatement of the relighting model, independent of nu_nerf_amd/csrc: the integer sample sequence, the
sample directions and shadow rays, the lat-long environment lookup, the BRDF weights, the resolve sum, the G-buffer attributes and a
brute-force ray / triangle sweep.  No GPU, no torch."""
import numpy as np

ROW = 20
MISS = 10000000
ALPHA_MIN = 1e-3
NOV_MIN = 1e-4
_M32 = np.uint64(0xFFFFFFFF)


# ---- integer part --------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    h = np.asarray(h, np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def bitrev32(j):
    j = np.asarray(j, np.uint64)
    r = np.zeros_like(j)
    for b in range(32):
        r |= ((j >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return r


def sample_bits(img, pixel, seed, S, s):
    """(lobe, b1, b2) of sample s of S for pixel `pixel` of image `img` (arrays broadcast): the two 24-bit integers behind the uniforms."""
    img, pixel, s = (np.asarray(a, np.int64) for a in (img, pixel, s))
    M = S // 2
    lobe = (s >= M).astype(np.int64)
    j = (s - lobe * M).astype(np.uint64)
    x1 = (j << np.uint64(32)) // np.uint64(M)
    x2 = bitrev32(j)
    a = fmix32(img.astype(np.uint64) + np.uint64(0x9E3779B9))
    a = fmix32(a ^ pixel.astype(np.uint64))
    a = fmix32(a ^ np.uint64(int(seed) & 0xFFFFFFFF))
    h1 = fmix32(a + np.uint64(2) * lobe.astype(np.uint64) + np.uint64(1))
    h2 = fmix32(h1 ^ np.uint64(0x68E31DA4))
    b1 = ((x1 + h1) & _M32) >> np.uint64(8)
    b2 = ((x2 + h2) & _M32) >> np.uint64(8)
    return lobe, b1.astype(np.int64), b2.astype(np.int64)


# ---- directions ----------------------------------------------------------------------------------------------------------------------
def frame(n):
    sg = np.copysign(1.0, n[..., 2])
    a = -1.0 / (sg + n[..., 2])
    c = n[..., 0] * n[..., 1] * a
    t = np.stack([1.0 + sg * n[..., 0] ** 2 * a, sg * c, -sg * n[..., 0]], -1)
    b = np.stack([c, sg + n[..., 1] ** 2 * a, -n[..., 1]], -1)
    return t, b


def sample_dirs(rows, lobe, b1, b2):
    """rows [N,ROW] float64, lobe / b1 / b2 [N] -> l [N,3], h [N,3] (zero for the diffuse lobe), ok [N] (V.H > 0 or diffuse)."""
    u1, u2 = b1 * 2.0 ** -24, b2 * 2.0 ** -24
    ns, v = rows[:, 7:10], rows[:, 15:18]
    t, b = frame(ns)
    phi = 2.0 * np.pi * u1
    a = np.maximum(rows[:, 14] ** 2, ALPHA_MIN)
    den = np.where(lobe == 0, 1.0, (1.0 - u2) + a * a * u2)
    ct, st = np.sqrt((1.0 - u2) / den), np.sqrt(np.where(lobe == 0, u2, a * a * u2) / den)
    w = (st * np.cos(phi))[:, None] * t + (st * np.sin(phi))[:, None] * b + ct[:, None] * ns
    voh = np.sum(v * w, 1)
    spec = (lobe == 1)[:, None]
    l = np.where(spec, 2.0 * voh[:, None] * w - v, w)
    h = np.where(spec, w, 0.0)
    return l, h, (lobe == 0) | (voh > 0)


def shadow_rays(rows, lobe, b1, b2, eps):
    """(origin [N,3], direction [N,3], n_s . l, n_g . l, ok)"""
    l, _, ok = sample_dirs(rows, lobe, b1, b2)
    o = rows[:, 1:4] + eps * rows[:, 4:7]
    return o, l, np.sum(rows[:, 7:10] * l, 1), np.sum(rows[:, 4:7] * l, 1), ok


# ---- environment ---------------------------------------------------------------------------------------------------------------------
def env_lookup(env, d):
    """env [H,W,3], d [N,3] -> [N,3]: column (1/2 - atan2(y, x) / 2 pi) W, row atan2(hypot(x, y), z) / pi H, texel centres at
    half-integers, bilinear, u wraps, v clamps."""
    env = np.asarray(env, np.float64)
    H, W = env.shape[:2]
    fx = (0.5 - np.arctan2(d[:, 1], d[:, 0]) / (2.0 * np.pi)) * W - 0.5
    fy = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2]) / np.pi * H - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    ix0 = np.mod(x0.astype(np.int64), W)
    ix1 = np.mod(ix0 + 1, W)
    iy0 = np.clip(y0.astype(np.int64), 0, H - 1)
    iy1 = np.clip(y0.astype(np.int64) + 1, 0, H - 1)
    return (1 - ay) * ((1 - ax) * env[iy0, ix0] + ax * env[iy0, ix1]) + ay * ((1 - ax) * env[iy1, ix0] + ax * env[iy1, ix1])


# ---- shading -------------------------------------------------------------------------------------------------------------------------
def g1_smith(x, a2):
    return 2.0 * x / (x + np.sqrt(a2 + (1.0 - a2) * x * x))


def g1_schlick(x, a2):
    k = np.sqrt(a2) / 2.0
    return x / (x * (1.0 - k) + k)


def weights(rows, lobe, l, h, g1=g1_smith):
    """Estimator weight / pdf [N,3] of each sample (visibility and radiance not included)."""
    ns, v = rows[:, 7:10], rows[:, 15:18]
    albedo, metallic = rows[:, 10:13], rows[:, 13:14]
    a = np.maximum(rows[:, 14] ** 2, ALPHA_MIN)
    a2 = a * a
    nov = np.maximum(np.sum(ns * v, 1), NOV_MIN)
    nol, noh, voh = np.sum(ns * l, 1), np.sum(ns * h, 1), np.sum(v * h, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = g1(nol, a2) * g1(nov, a2) * voh / (nov * noh)
    fc = (1.0 - np.minimum(voh, 1.0)) ** 5
    f0 = 0.04 + (albedo - 0.04) * metallic
    spec = (f0 + (1.0 - f0) * fc[:, None]) * k[:, None]
    return np.where((lobe == 0)[:, None], (1.0 - metallic) * albedo, spec)


def resolve(rows, img, pixel, vis, S, seed, env, g1=g1_smith):
    """Linear RGB [n_pix,3]: rows [n_pix,ROW], img / pixel [n_pix], vis [n_pix,S] (the visibility bytes, 0 also for untraced samples)."""
    n = rows.shape[0]
    out = np.zeros((n, 3))
    s = np.arange(S)
    for i in range(n):
        lit = vis[i] != 0
        if not lit.any():
            continue
        lobe, b1, b2 = sample_bits(img[i], pixel[i], seed, S, s[lit])
        r = np.repeat(rows[i:i + 1], int(lit.sum()), 0)
        l, h, _ = sample_dirs(r, lobe, b1, b2)
        out[i] = np.sum(weights(r, lobe, l, h, g1) * env_lookup(env, l), 0) * (2.0 / S)
    return out


def linear_to_srgb(x):
    eps = np.finfo(np.float32).eps
    return np.where(x <= 0.0031308, 323 / 25 * x, (211 * np.maximum(x, eps) ** (5 / 12) - 11) / 200)


def to_srgb8(rgb):
    return np.floor(np.clip(linear_to_srgb(rgb), 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def barycentrics(o, d, v0, v1, v2):
    """Moeller-Trumbore (u, v, t, det) of rays [N] against triangles [N] (row by row)."""
    e1, e2 = v1 - v0, v2 - v0
    pv = np.cross(d, e2)
    det = np.sum(e1 * pv, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / det
        tv = o - v0
        u = np.sum(tv * pv, 1) * inv
        qv = np.cross(tv, e1)
        return u, np.sum(d * qv, 1) * inv, np.sum(e2 * qv, 1) * inv, det


def brute_trace(V, F, o, d, tmin=0.0, tmax=1e16):
    """(hit [N] bool, face [N], t [N]) of the closest hit of every ray against every triangle, float64."""
    N = o.shape[0]
    best_t, best_f = np.full(N, tmax), np.full(N, MISS, np.int64)
    tri = V[F]
    for f in range(F.shape[0]):
        u, v, t, det = barycentrics(o, d, *(np.broadcast_to(tri[f, k], (N, 3)) for k in range(3)))
        ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < best_t)
        best_t[ok], best_f[ok] = t[ok], f
    return best_f != MISS, best_f, best_t


def gbuffer_rows(V, F, VN, mat, o, d, face, img, pixel):
    """G-buffer rows [N,ROW] float64 of the rays (o, d) that hit `face` (all of them hits); the last two entries hold img / pixel as
    floats (compare them as integers elsewhere)."""
    f = F[face]
    v0, v1, v2 = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    u, v, t, _ = barycentrics(o, d, v0, v1, v2)
    w0 = 1.0 - u - v
    view = -d
    ng = np.cross(v1 - v0, v2 - v0)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    ng = np.where((np.sum(ng * view, 1) < 0)[:, None], -ng, ng)
    ns = w0[:, None] * VN[f[:, 0]] + u[:, None] * VN[f[:, 1]] + v[:, None] * VN[f[:, 2]]
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    ns = np.where((np.sum(ns * ng, 1) < 0)[:, None], -ns, ns)
    m = w0[:, None] * mat[f[:, 0]] + u[:, None] * mat[f[:, 1]] + v[:, None] * mat[f[:, 2]]
    rows = np.zeros((o.shape[0], ROW))
    rows[:, 0], rows[:, 1:4], rows[:, 4:7], rows[:, 7:10] = t, o + t[:, None] * d, ng, ns
    rows[:, 10:15], rows[:, 15:18], rows[:, 18], rows[:, 19] = m, view, img, pixel
    return rows


def pinhole_rays(K, pose, h, w):
    """Pixel-centre rays of a world -> camera pose [3,4] and K [3,3]: (o [h*w,3], d [h*w,3]) float64, row-major."""
    K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
    y, x = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    c = np.stack([x.ravel(), y.ravel(), np.ones(h * w)], 1)
    dd = (c @ np.linalg.inv(K).T) @ pose[:, :3]
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    o = np.broadcast_to(-pose[:, :3].T @ pose[:, 3], (h * w, 3)).copy()
    return o, dd


def vertex_normals(V, F):
    """Angle-weighted unit vertex normals, float64."""
    tri = V[F]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    vn = np.zeros_like(V)
    for k in range(3):
        a, b = tri[:, (k + 1) % 3] - tri[:, k], tri[:, (k + 2) % 3] - tri[:, k]
        cosang = np.sum(a * b, 1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        np.add.at(vn, F[:, k], np.arccos(np.clip(cosang, -1, 1))[:, None] * fn)
    return vn / np.linalg.norm(vn, axis=1, keepdims=True)


# ---- white furnace -------------------------------------------------------------------------------------------------------------------
def furnace_row(nov, albedo, metallic, roughness):
    """The G-buffer row of a point of an ideal sphere seen at N.V = nov (n_s = n_g = z)."""
    r = np.zeros(ROW)
    r[4:7] = r[7:10] = (0.0, 0.0, 1.0)
    r[10:13], r[13], r[14] = albedo, metallic, roughness
    r[15:18] = (np.sqrt(1.0 - nov * nov), 0.0, nov)
    return r


def furnace_estimate(nov, albedo, metallic, roughness, S, pixels, seed=0, g1=g1_smith):
    """[len(pixels),3]: the estimator under L = 1 with every traced sample unoccluded, one value per pixel id (= per sample shift)."""
    row = furnace_row(nov, albedo, metallic, roughness)
    out = []
    s = np.arange(S)
    for p in pixels:
        lobe, b1, b2 = sample_bits(0, p, seed, S, s)
        rows = np.repeat(row[None], S, 0)
        l, h, ok = sample_dirs(rows, lobe, b1, b2)
        lit = ok & (l[:, 2] > 0)
        out.append(np.sum(weights(rows, lobe, l, h, g1)[lit], 0) * (2.0 / S))
    return np.array(out)


def fg_lookup(lut, nov, roughness):
    """Bilinear, clamped lookup of the split-sum table lut [256(roughness),256(N.V),2] as the shading network does it."""
    H, W = lut.shape[:2]
    fx, fy = np.clip(nov, 0, 1) * W - 0.5, np.clip(roughness, 0, 1) * H - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    x0i, x1i = np.clip(x0.astype(int), 0, W - 1), np.clip(x0.astype(int) + 1, 0, W - 1)
    y0i, y1i = np.clip(y0.astype(int), 0, H - 1), np.clip(y0.astype(int) + 1, 0, H - 1)
    return (1 - ay) * ((1 - ax) * lut[y0i, x0i] + ax * lut[y0i, x1i]) + ay * ((1 - ax) * lut[y1i, x0i] + ax * lut[y1i, x1i])
