"""The appearance a trained model learned, at explicit surface points, without a mesh and without the volume render.

Reference: AppShadingNetwork.forward in its stage-1 form (network/field.py:684-777; AppShadingNetwork_SpecInner, the inner network of
the non-zero-thickness stage-2 model, is the same form): diffuse + specular under the learned light with occlusion, indirect light and
the transmission / refraction mix,
  colour = srgb((diffuse + specular) (1 - T) + (F light0 + (1 - F) refraction) T)
and the validation images of field.py:751-770.  In training this is the layered path shading_glue.shade (one encode kernel, four
predictor stacks, one combine kernel, with every encoded row and 21 hidden buffers in HBM); here the whole evaluation of a point set is
ONE launch of the fused kernel of csrc/surface_shade.hip (nu_surface_shade_fwd) after the fused SDF gradient (normals) and the fused
material bake (raw material heads): three launches for any point count, no workspace.  It is an fp32 evaluation in every `mlp_dtype`,
like the other bake kernels.

Not modelled: the human light (a model trained with shader_config.human_light is shaded with human_weight = 0, as predict_environment
does), the NeRF++ background, and refraction through a stage-2 shell -- ONE surface is shaded; the nested object seen through its shell
stays the job of relight --inner or render_eval.
"""
import torch

from . import _lib as L
from .materials import _resolve_which, bake_engine

# the kernel's outputs besides the colour (include/nu_nerf.h nu_surface_shade_fwd): name -> channels
TERMS = {'diffuse_color': 3, 'specular_color': 3, 'diffuse_light': 3, 'specular_light': 3, 'indirect_light': 3, 'refraction_light': 3,
         'occ_prob': 1, 'reflection_weight': 1}


def _bad(what, why):
    return L.NuNerfLibraryError(f"nu_surface_shade_fwd failed with code -1 (NU_ERR_ARG): {what} {why}")


def _rows(t, dev, what, n=None):
    """`t` as an fp32 device tensor [P, >= 3] whose rows are a fixed number of floats apart (a column slice of a wider matrix is fine)
    -> (tensor, leading dimension)."""
    if not torch.is_tensor(t):
        raise _bad(what, "are not a tensor")
    if not t.is_cuda or t.device != dev:
        raise _bad(what, "are not on the engine's GPU")
    if t.dtype != torch.float32:
        raise _bad(what, f"have dtype {t.dtype}, expected float32")
    if t.dim() != 2 or t.shape[1] < 3:
        raise _bad(what, f"have shape {tuple(t.shape)}, expected [P, >= 3]")
    if n is not None and t.shape[0] != n:
        raise _bad(what, f"have {t.shape[0]} rows, expected {n}")
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < 3):
        raise _bad(what, f"have strides {tuple(t.stride())}: rows must be contiguous and at least 3 floats apart")
    if t.shape[0] <= 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))


def shade_engine(renderer, which=None):
    """The HIP engine whose SDF, material and light networks shade the points: `which` as materials.bake_engine resolves it (stage 1, or
    'outer' / 'inner' of a stage-2 renderer -- the inner networks of both stage-2 models are the stage-1 form).  The same engine holds
    all three: it is what environment.light_engine and materials.bake_engine return for the same `which`."""
    return bake_engine(renderer, _resolve_which(renderer, which))


@torch.no_grad()
def shade_points(renderer, points, view_dirs, normals=None, *, which=None, terms=(), linear=False, _enc=False, _raw=False, _mraw=None):
    """The learned appearance at surface points -> dict of device tensors: 'rgb' [P,3] plus every name asked for in `terms`
    (TERMS: 'diffuse_color', 'specular_color', 'diffuse_light', 'specular_light', 'indirect_light', 'refraction_light' [P,3];
    'occ_prob', 'reflection_weight' [P]) -- the reference's validation images before their display clamps, the two light images
    linear (nu_surface_shade_fwd in include/nu_nerf.h).

    points, view_dirs (towards the camera), normals: [P, >= 3] float32 device tensors, rows contiguous and a fixed number of floats
    apart; directions and normals need not be unit.  normals=None: the SDF's gradient at the points (nu_sdf_grad_fwd).  The raw
    material heads come from the material bake kernel.  which: see shade_engine.  linear=True: 'rgb' skips linear_to_srgb.
    _enc / _raw / _mraw: the kernel's test outputs ('enc', 'raw') and a caller's raw material heads [P, >= 6]."""
    terms = (terms,) if isinstance(terms, str) else tuple(terms)
    unknown = [t for t in terms if t not in TERMS]
    if unknown:
        raise ValueError(f"terms={terms!r}: expected names of {tuple(TERMS)}")
    eng = shade_engine(renderer, which)
    dev = eng.dev
    points, x_ld = _rows(points, dev, "points")
    P = points.shape[0]
    view_dirs, v_ld = _rows(view_dirs, dev, "view directions", P)
    if normals is not None:
        normals, n_ld = _rows(normals, dev, "normals", P)
    if _mraw is not None:
        _mraw = _rows(_mraw, dev, "raw material heads", P)[0]
        if _mraw.shape[1] < 6 or not _mraw.is_contiguous():
            raise _bad("raw material heads", f"have shape {tuple(_mraw.shape)}, expected contiguous [P, >= 6]")
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    kout = {'color': e(P, 3)}
    for t in terms:
        kout[t] = e(P, 3) if TERMS[t] == 3 else e(P)
    enc = e(P, 3 * eng.ld_ol + 352 + eng.ld_rl) if _enc else None
    raw = e(P, 20) if _raw else None
    out = {'rgb': kout['color'], **{t: kout[t] for t in terms}}
    if _enc:
        out['enc'] = enc
    if _raw:
        out['raw'] = raw
    if P == 0:
        return out
    eng.pack()
    if normals is None:
        normals, n_ld = e(P, 3), 3
        eng.sdf_grad(points.data_ptr(), x_ld, P, grad=normals)
    if _mraw is None:
        _mraw = torch.zeros(P, 8, dtype=torch.float32, device=dev)
        met, rough, alb, tr = e(P), e(P), e(P, 3), e(P)
        eng.material_bake(points.data_ptr(), x_ld, P, met, rough, alb, tr, raw=True)
        _mraw[:, 0], _mraw[:, 1], _mraw[:, 2:5], _mraw[:, 5] = met, rough, alb, tr
    eng.surface_shade(points.data_ptr(), x_ld, view_dirs.data_ptr(), v_ld, normals.data_ptr(), n_ld, _mraw.data_ptr(), _mraw.shape[1], P,
                      linear=linear, out=kout, enc=enc, raw=raw)
    return out
