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
