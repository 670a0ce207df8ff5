"""Float64 numpy restatement of the three formulas of split-sum relighting: the zonal kernel regression of
nu_env_prefilter, the pyramid lookup and the split-sum resolve.  Inputs are taken as the fp32 values the device reads; every operation
after that is float64.  The bilinear lat-long tap and the table lookup are relight_oracle's."""
import numpy as np

import relight_oracle as RO

ALPHA_MIN = 1e-3


def lobe_param(kind, rho):
    """The parameter the C entry receives (fp32): GGX alpha = max(rho^2, ALPHA_MIN), vMF kappa = 1 / rho."""
    if kind == 'cosine':
        return 0.0
    return float(np.float32(max(float(rho) ** 2, ALPHA_MIN) if kind == 'ggx' else 1.0 / float(rho)))


def lobe(kind, param, c):
    """f(c) of include/nu_nerf.h."""
    c = np.asarray(c, np.float64)
    if kind == 'cosine':
        return np.maximum(c, 0.0)
    if kind == 'ggx':
        a2 = np.float64(param) ** 2
        noh2 = (1.0 + c) * 0.5
        return np.maximum(c, 0.0) * a2 / (np.pi * (noh2 * (a2 - 1.0) + 1.0) ** 2)
    assert kind == 'vmf'
    return np.exp(np.float64(param) * (c - 1.0))


def as_lobes(lobes):
    """[(kind, roughness or None)] from the spellings environment.prefilter_dirs takes."""
    return [(x, None) if isinstance(x, str) else (x[0], x[1]) for x in lobes]


def prefilter(src_dir, src_rgb, dirs, lobes, chunk=4096):
    """out [L,N,3] = sum_j w_j f_l(c_ij) rgb_j / sum_j w_j f_l(c_ij), c_ij = dirs_i . src_dir_j."""
    sd, rgb, d = np.asarray(src_dir, np.float64), np.asarray(src_rgb, np.float64)[:, :3], np.asarray(dirs, np.float64)
    lobes = as_lobes(lobes)
    out = np.empty((len(lobes), d.shape[0], 3))
    for i0 in range(0, d.shape[0], chunk):
        c = d[i0:i0 + chunk] @ sd[:, :3].T
        for l, (kind, rho) in enumerate(lobes):
            g = lobe(kind, lobe_param(kind, rho), c) * sd[None, :, 3]
            out[l, i0:i0 + chunk] = (g @ rgb) / g.sum(1, keepdims=True)
    return out


def pyramid_lookup(pyramid, levels, dirs, rho):
    """L(d, rho): rho clamped to the levels' range, the largest i with levels[i] <= rho (i <= L - 2), linear mix of the two taps."""
    pyramid, levels = np.asarray(pyramid, np.float64), np.asarray(levels, np.float64)
    d, rho = np.asarray(dirs, np.float64), np.asarray(rho, np.float64)
    taps = np.stack([RO.env_lookup(p, d) for p in pyramid])
    if len(levels) == 1:
        return taps[0]
    r = np.clip(rho, levels[0], levels[-1])
    i = np.clip(np.searchsorted(levels, r, side='right') - 1, 0, len(levels) - 2)
    t = ((r - levels[i]) / (levels[i + 1] - levels[i]))[:, None]
    n = np.arange(d.shape[0])
    return (1.0 - t) * taps[i, n] + t * taps[i + 1, n]


def resolve(rows, pyramid, levels, diffuse, lut):
    """rgb [N,3] of G-buffer rows [N,20]: (1 - m) a Ld(n) + (F0 A + B) L(2 (n.v) n - v, rho), lut [256,256,2]."""
    g = np.asarray(rows, np.float64)
    n, a, m, rho, v = g[:, 7:10], g[:, 10:13], g[:, 13:14], g[:, 14], g[:, 15:18]
    nov = np.sum(n * v, 1)
    r = 2.0 * nov[:, None] * n - v
    ab = RO.fg_lookup(np.asarray(lut, np.float64), nov, rho)
    f0 = 0.04 * (1.0 - m) + m * a
    return (1.0 - m) * a * RO.env_lookup(diffuse, n) + (f0 * ab[:, :1] + ab[:, 1:]) * pyramid_lookup(pyramid, levels, r, rho)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def linear_map(h, w, a, dirs_of):
    """E(omega) = 1 + a . omega on the texel centres of an h x w lat-long map, the same in the three channels scaled (1, 1, 1)."""
    d = np.asarray(dirs_of(h, w), np.float64)
    return np.repeat((1.0 + d @ np.asarray(a, np.float64))[:, None], 3, 1).reshape(h, w, 3)


def cosine_of_linear(a, d):
    """The cosine-weighted mean of 1 + a . omega about d: 1 + (2/3) a . d."""
    return 1.0 + (2.0 / 3.0) * (np.asarray(d, np.float64) @ np.asarray(a, np.float64))


def vmf_of_linear(a, d, rho):
    """The vMF-weighted mean (kappa = 1 / rho) of 1 + a . omega about d: 1 + (coth kappa - 1 / kappa) a . d."""
    k = 1.0 / np.float64(rho)
    return 1.0 + (1.0 / np.tanh(k) - 1.0 / k) * (np.asarray(d, np.float64) @ np.asarray(a, np.float64))
