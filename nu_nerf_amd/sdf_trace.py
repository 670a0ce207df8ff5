"""Sphere tracing of the trained SDF: the surface seen from a camera, without a mesh.

Reference: sphere_tracing() of network/tracing.py:103-164 -- entry into the bounding sphere, then x += d * clamp(sdf(x), -10, 10) until
|sdf| < 1e-5, the ray leaves the sphere, or 200 iterations have passed.  There it is a Python loop over whole-batch MLP calls whose
`break` waits for the slowest ray of the batch; here every ray is the function called on that ray ALONE (a ray's result does not depend
on its batch), and the whole march is ONE launch of csrc/sdf_trace.hip (nu_sdf_trace: persistent workgroups, 64 ray slots each, the
fused SDF forward around the step, finished slots refilled) for any ray count, with no workspace and no host read.  It is an fp32
evaluation in every `mlp_dtype` (the kernel reads the fp32 packed tables pack() always writes) and returns the bits of the composition
`sdf_forward(keep=False)` + separately rounded torch mul / add per iteration.  The exact per-ray arithmetic is stated at nu_sdf_trace in
include/nu_nerf.h.

trace_rays      rays -> {'pos' [R,3], 't' [R], 'sdf' [R] (the last evaluation), 'iters' [R] int32, 'hit' [R] uint8 (0 / 1)}
render_surface  a pinhole camera (mask_render.pinhole_rays: K, world -> camera pose) -> images of the traced surface: mask, depth,
                position, normal, and on request albedo / roughness / metallic (materials.bake_materials), mean / Gaussian curvature
                (curvature.bake_curvature) and the learned appearance (SHADING_AOVS: 'rgb' and the shading terms,
                surface_shade.shade_points), evaluated at the hit points only; and the learned NeRF++ background of every pixel's ray
                (BACKGROUND_AOVS: 'background', 'transmittance' and the composed 'frame', background.render_background).
'outer' is the stage-1 SDF, 'inner' a stage-2 model's inner SDF, as in materials.py.
"""
import torch

from . import _lib as L
from .materials import bake_engine

GEOMETRY_AOVS = ('mask', 'depth', 'position', 'normal')
MATERIAL_AOVS = ('albedo', 'roughness', 'metallic')
CURVATURE_AOVS = ('mean_curvature', 'gaussian_curvature')
AOVS = GEOMETRY_AOVS + MATERIAL_AOVS + CURVATURE_AOVS
# the learned appearance at the hit points (surface_shade.py): the colour and the reference's validation images (field.py:751-770)
SHADING_AOVS = ('rgb', 'diffuse_color', 'specular_color', 'diffuse_light', 'specular_light', 'occ_prob', 'indirect_light',
                'refraction_light', 'reflection_weight')
ALL_AOVS = AOVS + SHADING_AOVS
# the learned NeRF++ background of every pixel's ray (background.py) and the frame composed of it and 'rgb'
BACKGROUND_AOVS = ('background', 'transmittance', 'frame')
_CHANNELS = {'background': 3, 'frame': 3, 'position': 3, 'normal': 3, 'albedo': 3, 'rgb': 3, 'diffuse_color': 3, 'specular_color': 3, 'diffuse_light': 3,
             'specular_light': 3, 'indirect_light': 3, 'refraction_light': 3}
_SRGB_AOVS = ('diffuse_light', 'specular_light')       # the kernel returns these two linear; their pictures are clamp(linear_to_srgb(.))


def _fail(msg):
    raise L.NuNerfLibraryError(f"nu_sdf_trace failed with code -1 (NU_ERR_ARG): {msg}")


def _check_rays(x, what):
    """A [R, >= 3] float32 tensor whose rows are a fixed number of floats apart (a column slice of a wider matrix is fine) -> (x, ld)."""
    if not torch.is_tensor(x):
        _fail(f"{what} is not a tensor")
    if x.dtype != torch.float32:
        _fail(f"{what} has dtype {x.dtype}, expected float32")
    if x.dim() != 2 or x.shape[1] < 3:
        _fail(f"{what} has shape {tuple(x.shape)}, expected [R, >= 3]")
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < 3):
        _fail(f"{what} has strides {tuple(x.stride())}: rows must be contiguous and at least 3 floats apart")
    if x.shape[0] <= 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x, (int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]))


@torch.no_grad()
def trace_rays(renderer, rays_o, rays_d, *, which=None, mask=None, max_iter=200, threshold=1e-5, bound_radius=1.0, entry_forward=False):
    """Sphere-trace rays (rays_o, rays_d: [R, >= 3] float32 device tensors, the first three columns are origin / direction; mask: None or
    [R] bool / uint8, the rays to trace) against an SDF of `renderer` -> dict of device tensors 'pos' [R,3], 't' [R], 'sdf' [R] (the last
    evaluation), 'iters' [R] int32, 'hit' [R] uint8.  One kernel launch for any R.  bound_radius = 0 (or None): no bounding sphere.
    entry_forward: an origin inside the sphere starts at the origin (the reference steps back to the sphere's entry point).  A ray that is
    masked out, has a non-finite origin or misses the sphere: pos = origin, t = 0, iters = 0, hit = 0.  which: see materials.bake_engine."""
    rays_o, o_ld = _check_rays(rays_o, 'rays_o')
    rays_d, d_ld = _check_rays(rays_d, 'rays_d')
    R = rays_o.shape[0]
    if rays_d.shape[0] != R:
        _fail(f"{R} origins but {rays_d.shape[0]} directions")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
        _fail(f"max_iter = {max_iter!r}, expected an integer >= 1")
    if not float(threshold) > 0.0:
        _fail(f"threshold = {threshold!r}, expected > 0")
    bound_radius = 0.0 if bound_radius is None else float(bound_radius)
    if not bound_radius >= 0.0:
        _fail(f"bound_radius = {bound_radius!r}, expected >= 0 (0: no bounding sphere)")
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (R,)):
        _fail(f"mask must be a bool / uint8 tensor of shape [{R}]")
    eng = bake_engine(renderer, which)
    for what, x in (('rays_o', rays_o), ('rays_d', rays_d), ('mask', mask)):
        if x is not None and (not x.is_cuda or x.device != eng.dev):
            _fail(f"{what} is not on the engine's GPU")
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
    out = {'pos': torch.empty(R, 3, dtype=torch.float32, device=eng.dev), 't': torch.empty(R, dtype=torch.float32, device=eng.dev),
           'sdf': torch.empty(R, dtype=torch.float32, device=eng.dev), 'iters': torch.empty(R, dtype=torch.int32, device=eng.dev),
           'hit': torch.empty(R, dtype=torch.uint8, device=eng.dev)}
    if R == 0:
        return out
    eng.pack()
    eng.sdf_trace(rays_o.data_ptr(), o_ld, rays_d.data_ptr(), d_ld, R, fg=mask, max_iter=int(max_iter), threshold=float(threshold),
                  bound_radius=bound_radius, flags=L.NU_TRACE_ENTRY_FORWARD if entry_forward else 0, pos=out['pos'], t=out['t'],
                  sdf=out['sdf'], iters=out['iters'], hit=out['hit'])
    return out


def _check_aovs(aovs):
    aovs = (aovs,) if isinstance(aovs, str) else tuple(aovs)
    bad = [a for a in aovs if a not in ALL_AOVS + BACKGROUND_AOVS]
    if bad or not aovs:
        raise ValueError(f"aovs={aovs!r}: expected one or more of {ALL_AOVS + BACKGROUND_AOVS}")
    return aovs


@torch.no_grad()
def render_surface(renderer, K, pose, h, w, *, which=None, aovs=('depth', 'normal', 'mask'), chunk=None, white_background=None,
                   **trace_kw):
    """Images of the SDF's surface from one pinhole camera (K [3,3], pose [3,4] world -> camera, pixel centres, unit directions: the rays
    of mask_render.pinhole_rays): one trace (entry_forward=True: a camera inside the bounding sphere looks forward), then the jet and the
    material bake at the hit points only.  -> dict of device tensors, one per name in `aovs`:
      'mask' [h,w] uint8 (255 = hit)        'depth' [h,w] (t along the unit ray, 0 where missed)      'position', 'normal' [h,w,3]
      'albedo' [h,w,3], 'roughness', 'metallic' [h,w]      'mean_curvature', 'gaussian_curvature' [h,w]      (all 0 where missed)
    and the learned appearance at the hit points (SHADING_AOVS; surface_shade.shade_points with view direction = -ray direction, one
    fused shading kernel per pass), clamped to [0, 1] as the reference's validation pictures are:
      'rgb' [h,w,3]      'diffuse_color', 'specular_color', 'indirect_light', 'refraction_light' [h,w,3]
      'diffuse_light', 'specular_light' [h,w,3] (sRGB of the diffuse query's light / of the roughness-0 specular light)
      'occ_prob', 'reflection_weight' [h,w]
    and the learned NeRF++ background (BACKGROUND_AOVS; background.render_background on EVERY pixel's ray at background.default_nodes,
    stopped at the hit's t on hit pixels, one fused kernel per pass):
      'background' [h,w,3] (the composite of the outer samples in front of the surface)      'transmittance' [h,w] (what they let through)
      'frame' [h,w,3] = clamp(background + transmittance rgb, 0, 1) on hit pixels, clamp(background + (white ? transmittance : 0), 0, 1)
              on missed ones; white_background: None = cfg['is_nerf'] (the reference's color + (1 - acc) of NeRF-synthetic data)
    Only this one surface is shaded: no human light, no refraction through a stage-2 shell; the surface is opaque to the background.
    chunk: rays per pass (None: the whole image at once); the result does not depend on it.  trace_kw: max_iter, threshold, bound_radius
    of trace_rays."""
    from .curvature import bake_curvature
    from .mask_render import pinhole_rays
    from .materials import bake_materials
    aovs = _check_aovs(aovs)
    if 'entry_forward' in trace_kw or 'mask' in trace_kw:
        raise TypeError("render_surface: entry_forward and mask are not options of a camera render")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"h, w = {h}, {w}: expected >= 1")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    eng = bake_engine(renderer, which)
    dev = eng.dev
    K = torch.as_tensor(K, dtype=torch.float32).reshape(3, 3)
    pose = torch.as_tensor(pose, dtype=torch.float32).reshape(1, 3, 4)
    rays = pinhole_rays(K, pose, h, w, dev)                            # [h w, 6]
    n = h * w
    step = n if chunk is None else int(chunk)
    want_curv = 'normal' in aovs or any(a in aovs for a in CURVATURE_AOVS)
    want_mat = any(a in aovs for a in MATERIAL_AOVS)
    shading = tuple(a for a in aovs if a in SHADING_AOVS)
    want_bg = any(a in aovs for a in BACKGROUND_AOVS)
    white = bool(renderer.cfg.get('is_nerf', False)) if white_background is None else bool(white_background)
    flat = {a: torch.zeros((n, _CHANNELS[a]) if a in _CHANNELS else (n,), dtype=torch.uint8 if a == 'mask' else torch.float32, device=dev)
            for a in aovs}
    for i in range(0, n, step):
        part = rays[i:i + step]
        tr = trace_rays(renderer, part[:, :3], part[:, 3:], which=which, entry_forward=True, **trace_kw)
        idx = tr['hit'].nonzero().reshape(-1)
        pts = tr['pos'][idx].contiguous()
        dst = idx + i
        if 'mask' in flat:
            flat['mask'][i:i + step] = tr['hit'] * 255
        if 'depth' in flat:
            flat['depth'][dst] = tr['t'][idx]
        if 'position' in flat:
            flat['position'][dst] = pts
        if want_curv:
            curv = bake_curvature(renderer, pts, which=which)
            for a, k in (('normal', 'normal'), ('mean_curvature', 'mean'), ('gaussian_curvature', 'gaussian')):
                if a in flat:
                    flat[a][dst] = curv[k].reshape(flat[a][dst].shape)
        if want_mat:
            mat = bake_materials(renderer, pts, which=which)
            for a in MATERIAL_AOVS:
                if a in flat:
                    flat[a][dst] = mat[a].reshape(flat[a][dst].shape)
        if shading or 'frame' in aovs:
            from . import torch_glue as G
            from .surface_shade import shade_points
            sh = shade_points(renderer, pts, -part[idx, 3:6], which=which, terms=tuple(a for a in shading if a != 'rgb'))
            for a in shading:
                v = sh[a]
                flat[a][dst] = torch.clamp(G.linear_to_srgb(v) if a in _SRGB_AOVS else v, 0.0, 1.0)
        if want_bg:
            from .background import render_background
            t_stop = torch.where(tr['hit'] != 0, tr['t'], torch.full_like(tr['t'], float('inf')))
            bg = render_background(renderer, part[:, :3], part[:, 3:], t_stop=t_stop)
            if 'background' in flat:
                flat['background'][i:i + step] = bg['color']
            if 'transmittance' in flat:
                flat['transmittance'][i:i + step] = bg['transmittance']
            if 'frame' in flat:
                behind = bg['transmittance'][:, None].repeat(1, 3) if white else torch.zeros_like(bg['color'])
                behind[idx] = bg['transmittance'][idx][:, None] * torch.clamp(sh['rgb'], 0.0, 1.0)
                flat['frame'][i:i + step] = torch.clamp(bg['color'] + behind, 0.0, 1.0)
    return {a: v.reshape((h, w, 3) if a in _CHANNELS else (h, w)) for a, v in flat.items()}
