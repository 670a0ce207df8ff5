"""Float64 evaluation of the learned appearance at surface points (TEST INFRASTRUCTURE -- not a test, not product code).

A thin wrapper over oracle/stage1_oracle.py run in float64: sdf_forward gives the feature, autograd through it the normal,
shading_forward the colour (AppShadingNetwork.forward, network/field.py:684-777).  The individual terms (the validation images of
field.py:751-770 before their display clamps, as nu_surface_shade_fwd in include/nu_nerf.h defines them) and the raw heads are restated
here from the same formulas with the oracle's own predictor / encoding functions; `terms64` also takes the two settings shading_forward
has no argument for (light_pos_freq, the refraction cap of AppShadingNetwork_SpecInner).  No code of the kernel or of
nu_nerf_amd/surface_shade.py is used.
"""
import contextlib

import numpy as np
import torch

from oracle import stage1_oracle as O

TERMS = ('diffuse_color', 'specular_color', 'diffuse_light', 'specular_light', 'indirect_light', 'refraction_light', 'occ_prob',
         'reflection_weight')


@contextlib.contextmanager
def _float64_tables():
    """The oracle's IDE coefficient table as float64 (the same values: the table IS fp32 data) for the duration of a float64 call."""
    keep = O._IDE_MAT
    O._IDE_MAT = keep.astype(np.float64)
    try:
        yield
    finally:
        O._IDE_MAT = keep


def params64(params):
    return {k: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v), dtype=torch.float64) for k, v in params.items()}


def _t(a):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float64)


def geometry64(params, x, prefix='sdf_network'):
    """(feature [P,256], gradient [P,3]) of the SDF network at x, float64."""
    p, x = params64(params), _t(x)
    y = O.sdf_forward(p, x, prefix)
    return y[:, 1:].detach(), O.sdf_gradient(p, x, prefix).detach()


def terms64(params, cfg, points, normals, view_dirs, feats, prefix='color_network', pos_freq=6, refrac_exp_max=None):
    """dict of float64 numpy arrays: 'rgb' (sRGB), 'linear', the TERMS, 'reflective', 'raw' [P,20] (the heads before activation in the
    kernel's order: outer_light diffuse | specular | mirror, inner_light specular | mirror, inner_weight, refrac_light, 0) and 'mraw'."""
    p = params64(params)
    x, nrm, view, feats = _t(points), _t(normals), _t(view_dirs), _t(feats)
    exp_max, sd, rf = float(cfg['light_exp_max']), bool(cfg['sphere_direction']), int(cfg.get('refrac_freq', 6))
    rl_max = exp_max if refrac_exp_max is None else min(exp_max, float(refrac_exp_max))
    with _float64_tables():
        n = torch.nn.functional.normalize(nrm, dim=-1)
        v = torch.nn.functional.normalize(view, dim=-1)
        nov = torch.sum(n * v, -1, keepdim=True)
        refl = nov * n * 2 - v
        fx = torch.cat([feats, x], -1)
        mraw = torch.cat([O.predictor(p, f'{prefix}.{m}', fx, 'none') for m in
                          ('metallic_predictor', 'roughness_predictor', 'albedo_predictor', 'transmisstion_weight')], -1)
        m = torch.sigmoid(mraw)
        metallic, rough, albedo, trans = m[:, 0:1], m[:, 1:2], m[:, 2:5], m[:, 5:6]
        ones, zeros = torch.ones_like(rough), torch.zeros_like(rough)

        def outer(direction, kappa, kappa_sph):
            enc = O.ide(direction, kappa)
            if sd:
                sp = O.offset_points_to_sphere(x)
                sp = torch.nn.functional.normalize(sp + direction * O.sphere_exit_distance(sp, direction), dim=-1)
                enc = torch.cat([enc, O.ide(sp, kappa_sph)], -1)
            return O.predictor(p, f'{prefix}.outer_light', enc, 'none')
        pe = O.embed(x, pos_freq)
        raw = torch.cat([outer(n, ones, ones), outer(refl, rough, rough), outer(refl, zeros, rough),
                         O.predictor(p, f'{prefix}.inner_light', torch.cat([pe, O.ide(refl, rough)], -1), 'none'),
                         O.predictor(p, f'{prefix}.inner_light', torch.cat([pe, O.ide(refl, zeros)], -1), 'none'),
                         O.predictor(p, f'{prefix}.inner_weight', torch.cat([pe, O.embed(refl, 6)], -1), 'none'),
                         O.predictor(p, f'{prefix}.refrac_light', torch.cat([O.embed(x, rf), O.embed(v, rf)], -1), 'none'),
                         torch.zeros_like(rough)], -1)
        ex = lambda r: torch.exp(torch.clamp(r, max=exp_max))      # noqa: E731
        diffuse_light, direct, direct0, indirect, indirect0 = ex(raw[:, 0:3]), ex(raw[:, 3:6]), ex(raw[:, 6:9]), ex(raw[:, 9:12]), ex(raw[:, 12:15])
        refrac = torch.exp(torch.clamp(raw[:, 16:19], max=rl_max))
        occ = raw[:, 15:16] * 0.5 + 0.5
        occ_c = torch.clamp(occ, 0.0, 1.0)
        light = indirect * occ_c + direct * (1 - occ_c)
        light0 = indirect0 * occ_c + direct0 * (1 - occ_c)
        t = torch.clamp(1 - nov, 0.0, 1.0)
        fres = torch.clamp(0.04 + 0.96 * t * t * t * t * t, 0.0, 1.0)
        fg = O.lut_bilinear_clamp(p[f'{prefix}.FG_LUT'][0], torch.cat([torch.clamp(nov, 0.0, 1.0), torch.clamp(rough, 0.0, 1.0)], -1))
        diffuse_color = (1 - metallic) * albedo * diffuse_light
        spec_color = ((0.04 * (1 - metallic) + metallic * albedo) * fg[:, 0:1] + fg[:, 1:2]) * light
        linear = (diffuse_color + spec_color) * (1 - trans) + (fres * light0 + (1 - fres) * refrac) * trans
        out = {   # field.py:751-770 before the display clamps; the two light images linear
            'rgb': O.linear_to_srgb(linear), 'linear': linear,
            'diffuse_color': O.linear_to_srgb(diffuse_color),
            'specular_color': O.linear_to_srgb(spec_color) * (1 - trans) + fres * light0 * trans,
            'diffuse_light': diffuse_light, 'specular_light': light0, 'indirect_light': indirect * occ_c,
            'refraction_light': O.linear_to_srgb((1 - fres) * refrac * trans),
            'occ_prob': occ[:, 0], 'reflection_weight': fres[:, 0],
            'reflective': refl, 'raw': raw, 'mraw': mraw}
    return {k: v.detach().numpy() for k, v in out.items()}


def shade64(params, cfg, points, view_dirs, normals=None, feats=None, sdf_prefix='sdf_network', prefix='color_network', pos_freq=6,
            refrac_exp_max=None):
    """The float64 appearance at `points`: feature and normal from the SDF network unless given, colour from the oracle's
    shading_forward where it applies (pos_freq 6, no refraction cap; 'rgb' is then ITS result, 'rgb_terms' the restated one), plus the
    terms of terms64."""
    if feats is None or normals is None:
        f, g = geometry64(params, points, sdf_prefix)
        feats = f if feats is None else feats
        normals = g if normals is None else normals
    out = terms64(params, cfg, points, normals, view_dirs, feats, prefix, pos_freq, refrac_exp_max)
    out['rgb_terms'] = out['rgb']
    if pos_freq == 6 and refrac_exp_max is None:
        with _float64_tables():
            col, info = O.shading_forward(params64(params), cfg, _t(points), _t(normals), _t(view_dirs), _t(feats), prefix)
        out['rgb'] = col.detach().numpy()
        out['reflective'] = info['reflective'].detach().numpy()
        out['occ_prob_oracle'] = info['occ_prob'].detach().numpy()[:, 0]
    return out


def clamp_overrides(params, cfg, points, normals, view_dirs, feats, prefix='color_network', pos_freq=6):
    """Head overrides that put the rows on both sides of every clamp, from the float64 evaluation alone (as
    tests/environment_oracle.clamp_overrides does for the light bake): the bias of each exp head (outer_light, inner_light,
    refrac_light) is moved so that the median raw value of its channel over all its queries of the given rows is light_exp_max; the
    occlusion head's gain (weight_g) and bias put the quartiles of 0.5 raw + 0.5 at 0 and 1.  -> {parameter name: float32 array}."""
    raw = terms64(params, cfg, points, normals, view_dirs, feats, prefix, pos_freq)['raw']
    exp_max = float(cfg['light_exp_max'])
    arr = lambda k: np.asarray(params[k].detach().cpu() if torch.is_tensor(params[k]) else params[k], np.float64)      # noqa: E731
    over = {}
    for name, cols in (('outer_light', (0, 3, 6)), ('inner_light', (9, 12)), ('refrac_light', (16,))):
        pool = np.concatenate([raw[:, c:c + 3] for c in cols], 0)
        over[f'{prefix}.{name}.6.bias'] = (arr(f'{prefix}.{name}.6.bias') + exp_max - np.median(pool, axis=0)).astype(np.float32)
    b = float(arr(f'{prefix}.inner_weight.6.bias').reshape(-1)[0])
    lin = raw[:, 15] - b
    q25, q75 = np.quantile(lin, 0.25), np.quantile(lin, 0.75)
    gain = 2.0 / (q75 - q25)
    over[f'{prefix}.inner_weight.6.weight_g'] = (arr(f'{prefix}.inner_weight.6.weight_g') * gain).astype(np.float32)
    over[f'{prefix}.inner_weight.6.bias'] = np.asarray([-1.0 - gain * q25], np.float32)
    return over
