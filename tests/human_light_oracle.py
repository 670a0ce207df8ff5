"""float64 restatement of shader_config.human_light (network/field.py:411-445, :614-667, :773-774) for the tests, and the seeded
inputs that tests and scripts/gen_human_light_golden.py share (a fixture stores expected arrays only; inputs are rebuilt from the seed).

Everything is torch and follows the dtype of what it is given: float64 tensors give the oracle, float32 tensors the same formulas
in the reference's precision.  No GPU, no library.

  shade_dirs(n_raw, d)              n^, v^ = -d^, NoV, r = 2 (n^.v^) n^ - v^                       field.py:686-689
  plane(x, r, poses)                the intersection with the XY plane of the human frame          field.py:411-430
  encode(x, r, rho, poses)          mean / var / hit flag and the 24 IPE columns                   field.py:618-629, :433-444
  heads(raw, hit)                   h = exp(min(raw, 0)) hit, w = clamp(., 0, 1)                   field.py:630-634 (exp_max = 0.0)
  combine(...)                      AppShadingNetwork.forward's mix on raw heads, with the blend   field.py:662-665, :698-740
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SCALE = 0.3
PLANE_EPS = 1e-4
DISC = 1.5
REL_MARGIN = 1e-3          # rows this close (relative) to one of the three thresholds are left out of hit-flag comparisons


def shade_dirs(n_raw, d):
    nh = F.normalize(n_raw, dim=-1)
    vh = F.normalize(-d, dim=-1)
    nov = torch.sum(nh * vh, -1, keepdim=True)
    return nh, vh, nov, nov * nh * 2 - vh


def plane(x, r, poses):
    """-> (inter [P,3], dist [P], plane flag [P], r'_z [P] as computed); a row whose |r'_z| <= 1e-4 uses r'_z = 1e-4 as the reference does (its
    values never reach an output: the row cannot hit)."""
    R, t = poses[:, :, :3], poses[:, :, 3]
    xp = torch.einsum('pij,pj->pi', R, x) + t
    rp = torch.einsum('pij,pj->pi', R, r)
    rz_raw = rp[:, 2]
    ok = rz_raw.abs() > PLANE_EPS
    rz = torch.where(ok, rp[:, 2], torch.full_like(rp[:, 2], PLANE_EPS))
    dist = -xp[:, 2] / rz
    rp = torch.cat([rp[:, :2], rz[:, None]], -1)
    return xp + dist[:, None] * rp, dist, ok, rz_raw


def ipe(mean, var):
    """IPE(mean [P,2], [var, var], 0, 6): 24 columns, (k, c) with c fastest, then the same with sin(. + 0.5 pi)."""
    scales = (2.0 ** torch.arange(0, 6)).to(mean.dtype)
    sm = (mean[:, None, :] * scales[None, :, None]).reshape(mean.shape[0], -1)
    sv = (var[:, None, :].expand(-1, 1, 2) * (scales ** 2)[None, :, None]).reshape(mean.shape[0], -1)
    half_pi = torch.tensor(0.5 * np.pi, dtype=mean.dtype)
    return torch.exp(-0.5 * torch.cat([sv, sv], -1)) * torch.sin(torch.cat([sm, sm + half_pi], -1))


def encode(x, r, rho, poses):
    """x, r [P,3], rho [P,1], poses [P,3,4] -> dict(enc [P,24], hit [P] bool, dist [P], mean [P,2], near [P] bool).
    `near`: the row is within REL_MARGIN (relative; absolute for dist, whose threshold is 0) of a threshold it is compared with."""
    inter, dist, ok, rz = plane(x, r, poses)
    mean = inter[:, :2] * SCALE
    var = rho * (dist[:, None] * SCALE) ** 2
    mnorm = torch.norm(mean, dim=-1)
    hit = ok & (mnorm < DISC) & (dist > 0)
    hf = hit.to(mean.dtype)[:, None]
    mean_h, var_h = torch.where(hit[:, None], mean, torch.zeros_like(mean)), torch.where(hit[:, None], var, torch.zeros_like(var))
    near = ((rz.abs() - PLANE_EPS).abs() < REL_MARGIN * PLANE_EPS) | \
           (ok & (((mnorm - DISC).abs() < REL_MARGIN * DISC) | (dist.abs() < REL_MARGIN)))
    return {'enc': ipe(mean_h, var_h), 'hit': hit, 'dist': dist, 'mean': mean_h, 'near': near.detach(), 'hf': hf}


def non_hit_row(dtype=torch.float32):
    """IPE(0, 0): twelve zeros and twelve sin(0.5 pi) in the given precision."""
    one = torch.sin(torch.tensor(0.5 * np.pi, dtype=dtype))
    return torch.cat([torch.zeros(12, dtype=dtype), one.expand(12)])


def heads(raw, hit):
    out = torch.where(hit[:, None], torch.exp(torch.clamp(raw, max=0.0)), torch.zeros_like(raw))
    return out[:, :3], torch.clamp(out[:, 3:], 0.0, 1.0)


def linear_to_srgb(x):
    eps = torch.finfo(torch.float32).eps
    return torch.where(x <= 0.0031308, 323 / 25 * x, (211 * torch.clamp(x, min=eps) ** (5 / 12) - 11) / 200)


def lut_bilinear_clamp(lut, uv):
    """dr.texture(filter 'linear', boundary 'clamp') on lut [H,W,C]: texel centres at (i + 0.5) / N."""
    H, W, _ = lut.shape
    fx = torch.clamp(uv[:, 0] * W - 0.5, 0.0, W - 1.0)
    fy = torch.clamp(uv[:, 1] * H - 0.5, 0.0, H - 1.0)
    x0, y0 = torch.floor(fx).long(), torch.floor(fy).long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    tx, ty = (fx - x0.to(fx.dtype))[:, None], (fy - y0.to(fy.dtype))[:, None]
    top = lut[y0, x0] * (1 - tx) + lut[y0, x1] * tx
    bot = lut[y1, x0] * (1 - tx) + lut[y1, x1] * tx
    return top * (1 - ty) + bot * ty


def combine(mraw, ol, il, iw, rl, nov, lut, exp_max, hl=None, hit=None):
    """Raw heads -> (sRGB colour [P,3], h w [P,3] or None).  mraw [P,6] (metallic, roughness, albedo(3), transmission), ol [3P,3]
    (diffuse | specular at the roughness | mirror), il [2P,3], iw [P,1], rl [P,3], nov [P,1]; hl [P,4] + hit [P]: the human light."""
    P = mraw.shape[0]
    m = torch.sigmoid(mraw)
    met, rho, alb, T = m[:, 0:1], m[:, 1:2], m[:, 2:5], m[:, 5:6]
    e = lambda t: torch.exp(torch.clamp(t, max=exp_max))
    Ld, d1, d0 = e(ol[:P]), e(ol[P:2 * P]), e(ol[2 * P:])
    i1, i0, refr = e(il[:P]), e(il[P:]), e(rl)
    hw = None
    if hl is not None:
        h, w = heads(hl, hit)
        hw = h * w
        d1, d0 = hw + d1 * (1 - w), hw + d0 * (1 - w)
    oc = torch.clamp(iw * 0.5 + 0.5, 0.0, 1.0)
    light, light0 = i1 * oc + d1 * (1 - oc), i0 * oc + d0 * (1 - oc)
    t = torch.clamp(1 - nov, 0.0, 1.0)
    fres = torch.clamp(0.04 + 0.96 * t * t * t * t * t, 0.0, 1.0)
    fg = lut_bilinear_clamp(lut, torch.cat([torch.clamp(nov, 0.0, 1.0), torch.clamp(rho, 0.0, 1.0)], -1))
    spec = ((0.04 * (1 - met) + met * alb) * fg[:, 0:1] + fg[:, 1:2]) * light
    lin = ((1 - met) * alb * Ld + spec) * (1 - T) + (fres * light0 + (1 - fres) * refr) * T
    return linear_to_srgb(lin), hw


# ------------------------------------------------------------------------------------------------ seeded inputs
def camera_poses(n, seed, dist=3.0):
    """n world-to-camera poses [n,3,4] (float32) of cameras at `dist` from the origin looking at it, off the horizontal plane."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        az, el = 2 * math.pi * (i + 0.3 * g.random()) / n, 0.25 + 0.3 * g.random()
        c = dist * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])
        zc = -c / np.linalg.norm(c)
        xc = np.cross(zc, np.array([0.0, 0.0, 1.0]))
        xc /= np.linalg.norm(xc)
        yc = np.cross(zc, xc)
        R = np.stack([xc, yc, zc], 0)
        out.append(np.concatenate([R, (-R @ c)[:, None]], 1))
    return np.asarray(out, np.float32)


def human_poses(poses):
    """get_human_coordinate_poses (renderer.py:329-345, fixed_camera off) in float64 numpy -> float32 [n,3,4]."""
    poses = np.asarray(poses, np.float64)
    out = []
    for P in poses:
        c = -P[:, :3].T @ P[:, 3]
        c[2] = 0
        Y = np.array([0.0, 0.0, -1.0])
        Z = P[2, :3].copy()
        Z[2] = 0
        Z /= np.linalg.norm(Z)
        X = np.cross(Y, Z)
        R = np.stack([X, Y, Z], 0)
        out.append(np.concatenate([R, (-R @ c)[:, None]], 1))
    return np.asarray(out, np.float32)


def encode_inputs(P=1000, S=5, n_poses=3, seed=2027):
    """The rows of the kernel tests: uniform points in +-0.6, random unit reflections (realised through a raw normal n ~ r + v and a ray
    direction d = -v of random lengths, as the kernels receive them), three cameras at distance 3; rows 0..7 are hand-placed with
    r'_z = +-2e-5, +-5e-5 (not a plane intersection) and +-3e-4, +-2e-3 (one, far away).  idx [P] is a ray-major sample index with
    idx // S < n_poses; pt is the 8-float point record [x, unused, d, unused] with NaN in the unused slots.  g [P,24]: a cotangent."""
    g = np.random.Generator(np.random.PCG64(seed))
    hp = human_poses(camera_poses(n_poses, seed + 1))
    idx = g.integers(0, S * n_poses, P).astype(np.int32)
    x = g.uniform(-0.6, 0.6, (P, 3))
    r = g.standard_normal((P, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    for j, rz in enumerate((2e-5, -2e-5, 5e-5, -5e-5, 3e-4, -3e-4, 2e-3, -2e-3)):
        a = 0.7 * j + 0.2
        rp = np.array([math.cos(a), math.sin(a), rz])
        r[j] = hp[idx[j] // S][:, :3].astype(np.float64).T @ (rp / np.linalg.norm(rp))
    v = g.standard_normal((P, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = np.where((np.sum(v * r, 1, keepdims=True) < -0.9), -v, v)        # keep r + v away from zero
    n = (r + v) * g.uniform(0.5, 2.0, (P, 1))
    d = -v * g.uniform(0.5, 1.5, (P, 1))
    mraw = g.standard_normal((P, 8))
    hole = np.full((P, 1), np.nan)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {'n': f(n), 'pt': f(np.concatenate([x, hole, d, hole], 1)), 'mraw': f(mraw), 'idx': idx, 'poses': hp, 'S': S,
            'g': f(g.standard_normal((P, 24)))}


def encode_chain(I, dtype, n=None, logit=None):
    """The encoder's whole chain on the inputs of encode_inputs in `dtype`: raw normal and roughness logit (differentiable when
    given as leaves) -> encode() dict."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    n = t(I['n']) if n is None else n
    logit = t(I['mraw'][:, 1:2]) if logit is None else logit
    pt = t(I['pt'])
    _, _, _, r = shade_dirs(n, pt[:, 4:7])
    poses = t(I['poses'])[torch.from_numpy(I['idx'] // I['S']).long()]
    return encode(pt[:, :3], r, torch.sigmoid(logit), poses)


def shading_inputs(P=512, seed=3030, n_poses=3):
    """Inputs of the whole-shading tests: points in +-0.6, each seen from one of three cameras (view direction = towards that
    camera), normals scattered around the view direction so that most reflections head back to the photographer, features
    0.3 N(0,1), one human frame per point, a colour cotangent with weights in [0.5, 1.5].  The weights are positive on purpose: with
    sign-random ones the weight_g gradients of the one-row heads (a single number each, the sum over the rows of terms of both signs)
    lose two to three digits to cancellation -- the reference's own fp32 value of roughness_predictor.6.weight_g moves by 3.5e-5
    when its rows are merely permuted, against 4e-7 with positive weights -- and a comparison at 3e-4 would measure that."""
    g = np.random.Generator(np.random.PCG64(seed))
    cams = camera_poses(n_poses, seed + 1)
    hp = human_poses(cams)
    which = g.integers(0, n_poses, P)
    cen = np.stack([-c[:, :3].astype(np.float64).T @ c[:, 3].astype(np.float64) for c in cams], 0)
    x = g.uniform(-0.6, 0.6, (P, 3))
    v = cen[which] - x
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    n = (v + 0.7 * g.standard_normal((P, 3))) * g.uniform(0.5, 2.0, (P, 1))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {'points': f(x), 'normals': f(n), 'view_dirs': f(v), 'feats': f(0.3 * g.standard_normal((P, 256))), 'human_poses': hp[which],
            'gcol': f(0.5 + np.minimum(np.abs(g.standard_normal((P, 3))), 1.0))}


HEAD_OVERRIDE_BIAS = (-0.1, -1.8, -0.9, -0.7)
HEAD_OVERRIDE_GAIN = 6.0


def human_head_overrides(params, prefix='color_network.'):
    """The human-light head as the fixtures use it: with its initial bias log 0.01 the light is invisible (w = 0.01), so the head's
    bias is set to HEAD_OVERRIDE_BIAS (w around 0.5, h of order 1 and different per channel) and its weight_g scaled by
    HEAD_OVERRIDE_GAIN (so that h and w vary over the rows and some raw heads exceed the exp_max = 0 cap).  -> {key: array}."""
    kb, kg = prefix + 'human_light_predictor.6.bias', prefix + 'human_light_predictor.6.weight_g'
    return {kb: np.asarray(HEAD_OVERRIDE_BIAS, np.float32), kg: (params[kg] * HEAD_OVERRIDE_GAIN).astype(np.float32)}
