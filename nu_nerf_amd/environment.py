"""The illumination a trained model learned, read out for a caller's directions: the recovered environment as a lat-long map.

Reference: AppShadingNetwork.predict_specular_lights (network/field.py:636-667; AppShadingNetwork_SpecInner :1399-1430) with
reflective = d and no human light; the networks are outer_light / inner_light / inner_weight (:594-604):
  direct   = exp(min(outer_light([IDE(d, rho) | IDE(sph(x, d), rho) if sphere_direction]), exp_max))
  indirect = exp(min(inner_light([pos_enc(x) | IDE(d, rho)]), exp_max)) * occ                             (probe)
  occ      = clamp(0.5 inner_weight([pos_enc(x) | dir_enc(d)]) + 0.5, 0, 1)                               (probe)
  light    = indirect + direct (1 - occ)                                                                  (probe; else light = direct)
`direct` is the model's estimate of the capture environment; rho is the roughness the direction is queried with (the kappa_inv of the
integrated directional encoding: 0 is the mirror query, 1 the diffuse one).  With `sphere_direction` the outer light also sees where
the ray from x along d leaves the unit sphere, so the light depends on the point: a map is the environment as seen from ONE point
(default the origin).  The human light is left out on purpose: it belongs to a camera, not to the environment.

The whole evaluation is ONE launch of the fused kernel of csrc/light_bake.hip (nu_light_bake_fwd) for any row count; it is an fp32
evaluation in every `mlp_dtype`, like the material bake.  The map uses the lat-long convention of relight (csrc/relight.h
nu_relight_env: z up, row 0 = +z), so `relight --hdr env.hdr` re-renders the baked mesh under the illumination it was trained under.
"""
import numpy as np
import torch

from . import _lib as L
from .materials import _resolve_which, bake_engine


def light_engine(renderer, which=None):
    """The HIP engine whose light predictors are evaluated: `which` as materials.bake_engine resolves it, except that the default is
    'outer' for every renderer -- the environment is the outer light (of a stage-2 model: the stage-1 networks it carries)."""
    return bake_engine(renderer, _resolve_which(renderer, 'outer' if which is None else which))


def _bad(what, why):
    return L.NuNerfLibraryError(f"nu_light_bake_fwd failed with code -1 (NU_ERR_ARG): {what} {why}")


def _device_rows(t, dev, what, cols):
    """`t` as an fp32 contiguous device tensor [N, cols] (cols = 0: [N]); arrays are taken to the device, tensors are checked."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32)).to(dev)
    if not t.is_cuda:
        raise _bad(what, "are not on the GPU")
    if t.dtype != torch.float32:
        raise _bad(what, f"have dtype {t.dtype}, expected float32")
    if (t.dim() != 2 or t.shape[1] != cols) if cols else t.dim() != 1:
        raise _bad(what, f"have shape {tuple(t.shape)}, expected [N{', %d' % cols if cols else ''}]")
    if not t.is_contiguous():
        raise _bad(what, "are not contiguous")
    return t


@torch.no_grad()
def bake_light(renderer, dirs, roughness=0.0, points=None, *, which=None, probe=False, _enc=False, _raw=False):
    """The learned light arriving along `dirs` -> dict of device tensors: 'light' [N,3] and, with probe=True, 'direct' [N,3],
    'indirect' [N,3] (already multiplied by occ, as the reference returns it) and 'occ' [N].

    dirs [N,3] float32 on the device, contiguous.  They are used as given: unit length is the caller's business (the encodings are
    polynomials of d and are not renormalised).  roughness: a scalar or [N].  points: None (the origin), one point [3] for all rows
    or [N,3]; they matter with `sphere_direction` and for probe=True, which needs them.  which: see light_engine.  One kernel
    launch for any N.  _enc / _raw: the kernel's test outputs ('enc': the encoded input rows; 'raw' [N,8]: the heads before their
    activations -- direct 3, indirect 3, occlusion 1, 0)."""
    eng = light_engine(renderer, which)
    dirs = _device_rows(dirs, eng.dev, "dirs", 3)
    N = dirs.shape[0]
    if torch.is_tensor(roughness) and roughness.dim() or (not torch.is_tensor(roughness) and np.ndim(roughness)):
        kinv = _device_rows(roughness, eng.dev, "roughness values", 0)
        if kinv.shape[0] != N:
            raise _bad("roughness values", f"have shape {tuple(kinv.shape)}, expected [{N}]")
    else:
        kinv = torch.full((N,), float(roughness), dtype=torch.float32, device=eng.dev)
    x, x_stride = None, 0
    if points is not None:
        if not torch.is_tensor(points):
            points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32)).to(eng.dev)
        if points.dim() == 1:
            x = _device_rows(points.reshape(1, -1), eng.dev, "points", 3)
        else:
            x, x_stride = _device_rows(points, eng.dev, "points", 3), 3
            if x.shape[0] != N:
                raise _bad("points", f"have shape {tuple(x.shape)}, expected [{N}, 3] or [3]")
    if probe and x is None:
        raise _bad("points", "are needed by probe=True (the indirect light and the occlusion are functions of the point)")
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)      # noqa: E731
    out = {'light': e(N, 3)}
    if probe:
        out.update(direct=e(N, 3), indirect=e(N, 3), occ=e(N))
    if _enc:
        out['enc'] = e(N, eng.ld_ol + (224 if probe else 0))
    if _raw:
        out['raw'] = e(N, 8)
    if N == 0:
        return out
    eng.pack()
    eng.light_bake(dirs, kinv, N, x, x_stride, probe=probe, light=out['light'], direct=out.get('direct'), indirect=out.get('indirect'),
                   occ=out.get('occ'), enc=out.get('enc'), raw=out.get('raw'))
    return out


def latlong_dirs(h, w):
    """Texel-centre directions [h * w, 3] float32 (numpy, row-major) of an h x w lat-long map in relight's convention
    (csrc/relight.h nu_relight_env: z up, row 0 = +z): theta = (r + 1/2) pi / h, phi = 2 pi (1/2 - (c + 1/2) / w),
    d = (sin theta cos phi, sin theta sin phi, cos theta).  Computed in float64, then rounded."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"latlong_dirs: empty map {h} x {w}")
    theta = (np.arange(h, dtype=np.float64) + 0.5) * np.pi / h
    phi = 2.0 * np.pi * (0.5 - (np.arange(w, dtype=np.float64) + 0.5) / w)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.cos(phi)[None], st * np.sin(phi)[None], np.broadcast_to(ct, (h, w))], -1)
    return np.ascontiguousarray(d.reshape(h * w, 3), dtype=np.float32)


def project_sh(env):
    """Order-2 spherical-harmonic coefficients float64 [9,3] of a lat-long map [h,w,3] (transfer.sh_basis' order and
    constants): L_k = (4 pi / sum_j w_j) sum_j w_j Y_k(s_j) rgb_j over the texel centres s_j of latlong_dirs with w = sin theta.  On the
    host in float64: a 256 x 512 map is a 9 x 131 072 x 3 product."""
    from .transfer import sh_basis
    env = np.asarray(env, np.float64)
    if env.ndim != 3 or env.shape[2] != 3 or env.shape[0] < 1 or env.shape[1] < 1:
        raise ValueError(f"environment map must be [H,W,3], got {env.shape}")
    if not np.isfinite(env).all():
        raise ValueError("environment map has non-finite values")
    h, w = env.shape[:2]
    theta = (np.arange(h, dtype=np.float64) + 0.5) * np.pi / h
    phi = 2.0 * np.pi * (0.5 - (np.arange(w, dtype=np.float64) + 0.5) / w)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    dirs = np.stack([st * np.cos(phi)[None], st * np.sin(phi)[None], np.broadcast_to(ct, (h, w))], -1)      # latlong_dirs before rounding
    wgt = np.repeat(np.sin(theta), w)
    Y = sh_basis(dirs.reshape(h * w, 3))
    return (4.0 * np.pi / wgt.sum()) * ((Y * wgt[:, None]).T @ env.reshape(h * w, 3))


def environment_map(renderer, h=256, w=512, roughness=0.0, point=None, which=None, probe=False):
    """The learned illumination as a lat-long map, float32 numpy [h,w,3] (latlong_dirs' convention, linear radiance).  A sequence of
    roughness values gives the pyramid [L,h,w,3], still in one launch.  point: where the map is seen from (default the origin; it
    matters with `sphere_direction` and for probe=True, which returns the blended light instead of the direct one)."""
    eng = light_engine(renderer, which)
    levels = np.atleast_1d(np.asarray(roughness, dtype=np.float32))
    if levels.ndim != 1 or levels.size < 1:
        raise ValueError(f"roughness must be a scalar or a sequence, got shape {levels.shape}")
    nl = int(levels.size)
    d = latlong_dirs(h, w)
    dirs = torch.from_numpy(np.tile(d, (nl, 1))).to(eng.dev)
    kinv = torch.from_numpy(np.repeat(levels, h * w)).to(eng.dev)
    if point is None and probe:
        point = (0.0, 0.0, 0.0)
    if point is not None:
        point = np.asarray(point, dtype=np.float32).reshape(3)
    out = bake_light(renderer, dirs, kinv, point, which=which, probe=probe)['light'].cpu().numpy().reshape(nl, h, w, 3)
    return out if np.ndim(roughness) else out[0]


def write_hdr(path, img):
    """Radiance RGBE file (`#?RADIANCE`, FORMAT=32-bit_rle_rgbe, `-Y H +X W`) of a float [H,W,3] image, FLAT scanlines (no run-length
    coding: the format allows both, relight.read_hdr reads both).  A pixel is stored as (r, g, b, e) = (c / 2^(e - 136) rounded to
    nearest and held to 255, e) with 2^(e - 129) <= max channel < 2^(e - 128): the error is at most 2^-8 of the pixel's largest
    channel.  Negative values are stored as 0; a pixel below 2^-127 is (0, 0, 0, 0).  (A stored pixel that is not zero has a byte of at
    least 128, so no flat scanline can start with the (2, 2, W >> 8, W & 255) marker of a run-length one.)"""
    img = np.asarray(img, dtype=np.float64)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_hdr: image must be [H,W,3], got {img.shape}")
    if not np.isfinite(img).all():
        raise ValueError("write_hdr: image has non-finite values")
    img = np.maximum(img, 0.0)
    h, w = img.shape[:2]
    v = img.max(-1)
    _, e = np.frexp(v)                                   # v = m 2^e, m in [0.5, 1)
    live = (v > 0.0) & (e + 128 >= 1)
    if (e[live] + 128 > 255).any():
        raise ValueError("write_hdr: a value is too large for the RGBE exponent")
    e = np.where(live, e, 0)
    mant = np.minimum(np.rint(np.ldexp(img, (8 - e)[..., None])), 255.0)
    rgbe = np.zeros((h, w, 4), np.uint8)
    rgbe[..., :3] = np.where(live[..., None], mant, 0.0).astype(np.uint8)
    rgbe[..., 3] = np.where(live, e + 128, 0).astype(np.uint8)
    with open(path, 'wb') as fh:
        fh.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode())
        fh.write(rgbe.tobytes())
    return path


def predict_environment(renderer, h=256, w=512, roughness=0.0, point=None, which=None, probe=False):
    """What the renderer classes' predict_environment returns: environment_map."""
    return environment_map(renderer, h, w, roughness, point, which, probe)


# ---- prefiltering into the roughness pyramid of the split-sum model ----------------------------------------------------
LOBE_KINDS = {'cosine': L.NU_LOBE_COSINE, 'ggx': L.NU_LOBE_GGX, 'vmf': L.NU_LOBE_VMF}
ALPHA_MIN = 1e-3                # NU_RL_ALPHA_MIN of csrc/relight.h
DEFAULT_LEVELS = (0.0, 0.25, 0.5, 0.75, 1.0)


def _pf_bad(what, why):
    return L.NuNerfLibraryError(f"nu_env_prefilter failed with code -1 (NU_ERR_ARG): {what} {why}")


def lobe_param(kind, roughness):
    """The kernel's parameter of a lobe given by the roughness it serves: GGX alpha = max(rho^2, ALPHA_MIN); vMF kappa = 1 / rho (the
    kappa_inv of the integrated directional encoding); the cosine lobe has none (0)."""
    if kind not in LOBE_KINDS:
        raise ValueError(f"lobe kind must be one of {sorted(LOBE_KINDS)}, got {kind!r}")
    if kind == 'cosine':
        return 0.0
    rho = float(roughness)
    if kind == 'ggx':
        return max(rho * rho, ALPHA_MIN)
    if not rho > 0.0:
        raise ValueError(f"a vMF lobe needs a roughness > 0, got {roughness}")
    return 1.0 / rho


def lobe_falloff(kind, roughness, angle):
    """f(cos angle) / f(1) of the lobe in float64: its weight `angle` radians off axis relative to its peak."""
    c = np.cos(np.float64(angle))
    p = np.float64(lobe_param(kind, roughness))
    if kind == 'cosine':
        return max(c, 0.0)
    if kind == 'ggx':
        a2 = p * p
        return max(c, 0.0) * (a2 / (a2 + (1.0 - a2) * (1.0 - c) * 0.5)) ** 2
    return float(np.exp(p * (c - 1.0)))


def lobe_is_tapped(kind, roughness, src_height):
    """The tap rule: a level whose lobe is narrower than the source grid is served by the bilinear tap of the source instead of the
    regression -- its weight one source pitch (pi / src_height) off axis is below half its peak.  Roughness 0 always is (a sub-texel
    lobe over a texel-box map is the texel); the cosine lobe never is."""
    if kind == 'cosine':
        return False
    if float(roughness) <= 0.0:
        return True
    return bool(lobe_falloff(kind, roughness, np.pi / int(src_height)) < 0.5)


def source_table(env):
    """(src_dir [H*W,4], src_rgb [H*W,4]) float32 numpy of a lat-long map [H,W,3]: latlong_dirs' texel-centre directions with the
    quadrature weight w = sin theta (float64, then rounded; > 0 at every texel centre, the poles included), and the texels."""
    env = np.asarray(env)
    if env.ndim != 3 or env.shape[2] != 3 or env.shape[0] < 1 or env.shape[1] < 1:
        raise ValueError(f"environment map must be [H,W,3], got {env.shape}")
    if not np.isfinite(env).all():
        raise ValueError("environment map has non-finite values")
    h, w = env.shape[:2]
    theta = (np.arange(h, dtype=np.float64) + 0.5) * np.pi / h
    sd = np.empty((h * w, 4), np.float32)
    sd[:, :3] = latlong_dirs(h, w)
    sd[:, 3] = np.repeat(np.sin(theta), w)
    rgb = np.zeros((h * w, 4), np.float32)
    rgb[:, :3] = env.reshape(h * w, 3)
    return sd, rgb


def _lobes(lobes):
    out = []
    for item in lobes:
        kind, rho = (item, None) if isinstance(item, str) else item
        out.append((LOBE_KINDS[kind] if kind in LOBE_KINDS else -1, lobe_param(kind, rho)))
    if not 1 <= len(out) <= L.NU_ENV_MAX_LOBES:
        raise _pf_bad("lobes", f"must number 1..{L.NU_ENV_MAX_LOBES}, got {len(out)}")
    return out


def _pf_rows(t, dev, what, cols):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32)).to(dev)
    if not t.is_cuda:
        raise _pf_bad(what, "are not on the GPU")
    if t.dtype != torch.float32:
        raise _pf_bad(what, f"have dtype {t.dtype}, expected float32")
    if t.dim() != 2 or t.shape[1] != cols:
        raise _pf_bad(what, f"have shape {tuple(t.shape)}, expected [N, {cols}]")
    if not t.is_contiguous():
        raise _pf_bad(what, "are not contiguous")
    return t


@torch.no_grad()
def prefilter_dirs(env, dirs, lobes, device=None):
    """The raw entry (one nu_env_prefilter call): out [L,N,4] float32 on the device, rgb = the lobe-weighted mean of the source around each
    direction, alpha = 1.  env: a lat-long map [H,W,3] (source_table makes the point set) or a weighted point set (src_dir [M,4] = unit
    direction and weight, src_rgb [M,4]); dirs [N,3]; lobes: a sequence of 'cosine', ('ggx', roughness) or ('vmf', roughness), at most
    NU_ENV_MAX_LOBES.  Arrays are taken to the device; tensors must be float32, contiguous and on it.  A query's bits do not depend on
    the other queries or lobes of the call."""
    import ctypes
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if isinstance(env, (tuple, list)):
        sd, rgb = env
    else:
        sd, rgb = source_table(env.cpu().numpy() if torch.is_tensor(env) else env)
    sd, rgb, dirs = _pf_rows(sd, dev, "source directions", 4), _pf_rows(rgb, dev, "source values", 4), _pf_rows(dirs, dev, "dirs", 3)
    if rgb.shape[0] != sd.shape[0]:
        raise _pf_bad("source values", f"have shape {tuple(rgb.shape)}, expected [{sd.shape[0]}, 4]")
    table = _lobes(lobes)
    nl, N, M = len(table), int(dirs.shape[0]), int(sd.shape[0])
    out = torch.empty(nl, N, 4, dtype=torch.float32, device=dev)
    lib = L.load()
    need = lib.nu_env_prefilter_workspace_bytes(N, M, nl)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
    kinds = (ctypes.c_int * nl)(*[k for k, _ in table])
    params = (ctypes.c_float * nl)(*[p for _, p in table])
    lib.nu_env_prefilter(L.ptr(sd), L.ptr(rgb), M, L.ptr(dirs), N, kinds, params, nl, L.ptr(out), L.ptr(ws), need, L.stream())
    return out


@torch.no_grad()
def prefilter(env, roughness=DEFAULT_LEVELS, height=None, width=None, lobe='ggx', diffuse='cosine', device=None):
    """A lat-long map [H,W,3] prefiltered into the split-sum pyramid -> (pyramid [L,h,w,3], diffuse [h,w,3], info), float32 numpy in
    latlong_dirs' convention (h, w default to the source's).  Level l is the `lobe` ('ggx' or 'vmf') of roughness[l]; the diffuse map is
    the 'cosine' lobe (irradiance / pi) or, with diffuse='vmf', the vMF lobe of roughness 1 (the integrated directional encoding's own
    convention, as lobe='vmf').  Levels under the tap rule (lobe_is_tapped) are the bilinear tap of the source (relight.env_lookup);
    every other level and the diffuse map come from ONE nu_env_prefilter call.  info: 'tapped' (the indices of the tapped levels),
    'lobes' (what the call evaluated), 'pairs' (queries x source points x lobes of the call).  The work is that product: it grows with the
    square of the map's area when h, w follow the source (28 ms for 256 x 512 on an MI355X); a smaller query grid is enough
    for the rough levels of a large map."""
    from .relight import env_lookup, pack_env
    if lobe not in ('ggx', 'vmf') or diffuse not in ('cosine', 'vmf'):
        raise ValueError(f"lobe must be 'ggx' or 'vmf' and diffuse 'cosine' or 'vmf', got {lobe!r}, {diffuse!r}")
    env = np.ascontiguousarray(env.cpu().numpy() if torch.is_tensor(env) else env, dtype=np.float32)
    levels = [float(r) for r in np.atleast_1d(np.asarray(roughness, dtype=np.float64))]
    if not levels or any(r < 0.0 for r in levels):
        raise ValueError(f"roughness levels must be >= 0 and at least one, got {roughness}")
    sd, rgb = source_table(env)
    H, W = env.shape[:2]
    h, w = int(height or H), int(width or W)
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    dirs = torch.from_numpy(latlong_dirs(h, w)).to(dev)
    tapped = [i for i, r in enumerate(levels) if lobe_is_tapped(lobe, r, H)]
    lobes = [(lobe, r) for i, r in enumerate(levels) if i not in tapped] + ['cosine' if diffuse == 'cosine' else ('vmf', 1.0)]
    reg = prefilter_dirs((sd, rgb), dirs, lobes, dev)[..., :3].cpu().numpy().reshape(len(lobes), h, w, 3)
    pyramid = np.empty((len(levels), h, w, 3), np.float32)
    if tapped:
        tap = env_lookup(torch.from_numpy(pack_env(env)).to(dev), dirs).cpu().numpy().reshape(h, w, 3)
    k = 0
    for i in range(len(levels)):
        if i in tapped:
            pyramid[i] = tap
        else:
            pyramid[i] = reg[k]
            k += 1
    info = {'tapped': tapped, 'lobes': [x if isinstance(x, str) else [x[0], x[1]] for x in lobes], 'pairs': h * w * H * W * len(lobes),
            'source': [H, W], 'shape': [len(levels), h, w, 3]}
    return pyramid, np.ascontiguousarray(reg[-1]), info
