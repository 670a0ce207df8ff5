"""Writes tests/golden/human_light_{encode,shading_sd0,shading_sd1,render}.npz: shader_config.human_light as the REFERENCE's own
modules compute it on the CPU (network/field.py:411-445, :614-667, :773-774; network/renderer_zerothick.py render_core).

Run once on a machine with the reference checkout, from its directory (the import shims are those of oracle/gen_golden.py):

    cd <reference> && python <repo>/scripts/gen_human_light_golden.py

The test suite needs neither this script nor the reference, only the .npz files.  Parameters and inputs are seed-generated
(randomize_for_parity(init_stage1_params(6033, human_light=True), seed=1); tests/human_light_oracle.py encode_inputs /
shading_inputs), so a fixture holds expected arrays, measured deviations and the overrides only.

Overrides: the human-light head starts at bias log 0.01, i.e. w = 0.01 -- the light is invisible and a no-op implementation would
pass.  The head's bias and weight_g are therefore replaced (human_light_oracle.human_head_overrides) and recorded as
`override__<key>`; the generator asserts that on hit rows the reference's colour with the key on differs from its colour with the
key off by at least 100 x the colour tolerance of the tests (median over the hit rows of the largest channel difference), and the
tests re-assert it on the fixture.

  human_light_encode.npz       1000 rows of human_light_oracle.encode_inputs: the float64 oracle's hit flags, the number of rows next
                               to a threshold, and the largest deviation of the reference's fp32 encoding / fp32 autograd gradients
                               (raw normal, roughness logit) from the float64 oracle -- the tests' tolerances are 4 x these figures.
  human_light_shading_sd*.npz  AppShadingNetwork.forward(inter_results=True) on 512 points + backward of sum(colour * gcol):
                               colour, colour with the key off, the human_light image, d normals, d features (rows 0..63 and the
                               per-row norms), the gradient norm of every parameter, and the rows that sit on a ReLU kink.
  human_light_render.npz       network/renderer_zerothick.py render_core on 24 rays from 3 poses at its own z_vals, train (losses, gradient
                               norms) and eval (the human_light image and ray_rgb).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from gen_golden import install_shims, to_t   # noqa: E402
import human_light_oracle as HO              # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
COLOUR_TOL = 1e-4               # the colour tolerance of the stage-1 parity tests (tests/test_core_parity_gpu.py: rtol 1e-4 on O(1) values)
SHADER = {'human_light': True, 'light_exp_max': 5.0}
KINK_EPS = 1e-6


def color_params(sd, rf=6):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    p = randomize_for_parity(init_stage1_params(6033, sphere_direction=sd, refrac_freq=rf, human_light=True), seed=1)
    over = HO.human_head_overrides(p)
    p.update(over)
    return p, over


def gen_encode(rfield):
    I = HO.encode_inputs()
    P = I['n'].shape[0]
    col = rfield.AppShadingNetwork(dict(SHADER, sphere_direction=False))
    seen = {}
    col.human_light_predictor.register_forward_pre_hook(lambda mod, args: seen.__setitem__('enc', args[0]))
    # the reference in fp32: reflective / roughness as AppShadingNetwork.forward forms them (field.py:686-688), then its own
    # predict_human_light; the predictor's input is taken by the hook
    n32 = torch.from_numpy(I['n']).requires_grad_(True)
    lg32 = torch.from_numpy(I['mraw'][:, 1:2].copy()).requires_grad_(True)
    pt = torch.from_numpy(I['pt'])
    normals, view = F.normalize(n32, dim=-1), F.normalize(-pt[:, 4:7], dim=-1)
    reflective = torch.sum(view * normals, -1, keepdim=True) * normals * 2 - view
    poses = torch.from_numpy(I['poses'])[torch.from_numpy(I['idx'] // I['S']).long()]
    col.predict_human_light(pt[:, :3].contiguous(), reflective, poses, torch.sigmoid(lg32))
    enc32 = seen['enc']
    g = torch.from_numpy(I['g'])
    dn32, dl32 = torch.autograd.grad((enc32 * g).sum(), (n32, lg32))
    hit32 = ~(enc32.detach() == HO.non_hit_row()[None]).all(1)

    n64 = torch.from_numpy(I['n']).double().requires_grad_(True)
    lg64 = torch.from_numpy(I['mraw'][:, 1:2].copy()).double().requires_grad_(True)
    o = HO.encode_chain(I, torch.float64, n64, lg64)
    dn64, dl64 = torch.autograd.grad((o['enc'] * g.double()).sum(), (n64, lg64))
    near, hit = o['near'].numpy(), o['hit'].numpy()
    inter, dist, ok, _ = HO.plane(pt[:, :3].double(), HO.shade_dirs(n64.detach(), pt[:, 4:7].double())[3], poses.double())
    outside = ok.numpy() & (dist.numpy() > 0) & ~hit
    behind = ok.numpy() & (dist.numpy() <= 0)
    counts = dict(hits=int(hit.sum()), behind=int(behind.sum()), outside=int(outside.sum()), no_plane=int((~ok.numpy()).sum()))
    assert min(counts['hits'], counts['behind'], counts['outside']) > 50 and counts['no_plane'] == 4, counts
    assert int(near.sum()) == 0, "the reference alone must leave out no row"
    assert np.array_equal(hit32.numpy(), hit), "fp32 and float64 hit flags of the reference differ"
    keep = ~near
    res = {'hit': hit, 'n_near': np.asarray(int(near.sum())),
           'enc_dev': np.asarray(float((enc32.detach().double() - o['enc'].detach())[keep].abs().max())),
           'dn_dev': np.asarray(float((dn32.double() - dn64)[keep].abs().max())),
           'dlogit_dev': np.asarray(float((dl32.double() - dl64)[keep].abs().max())),
           'dn_max': np.asarray(float(dn64.abs().max())), 'dlogit_max': np.asarray(float(dl64.abs().max())),
           'counts': np.asarray([counts['hits'], counts['behind'], counts['outside'], counts['no_plane']])}
    assert float(dn32[~hit32].abs().max()) == 0.0 and float(dl32[~hit32].abs().max()) == 0.0
    np.savez_compressed(os.path.join(OUT, 'human_light_encode.npz'), **res)
    print('encode', counts, {k: float(v) for k, v in res.items() if v.ndim == 0})


def gen_shading(rfield, sd):
    I = HO.shading_inputs()
    p, over = color_params(sd)
    col = rfield.AppShadingNetwork(dict(SHADER, sphere_direction=sd))
    col.load_state_dict(to_t({k[len('color_network.'):]: v for k, v in p.items() if k.startswith('color_network.')}), strict=True)
    t = lambda k: torch.from_numpy(I[k])
    normals, feats = t('normals').requires_grad_(True), t('feats').requires_grad_(True)
    # rows with a ReLU input within KINK_EPS of zero in any stack: the reference's INPUT gradient of such a row jumps when another
    # valid fp32 order rounds that pre-activation to the other side (a 256-term fp32 dot product of O(1) terms is uncertain by
    # ~sqrt(256) 2^-24 ~ 1e-6), so the tests leave these rows out of the per-row gradient comparisons (never out of anything else)
    kink = torch.zeros(I['points'].shape[0], dtype=torch.bool)
    def mark(mod, inputs, out):
        kink.logical_or_((out.detach().abs() < KINK_EPS).any(1))
    hooks = [m.register_forward_hook(mark) for m in col.modules() if isinstance(m, torch.nn.Linear) and m.out_features == 256]
    color, _, inter = col(t('points'), normals, t('view_dirs'), feats, t('human_poses'), inter_results=True, step=0)
    for h in hooks:
        h.remove()
    assert 0 < int(kink.sum()) <= 0.1 * kink.numel(), int(kink.sum())
    (color * t('gcol')).sum().backward()
    col.cfg['human_light'] = False
    with torch.no_grad():
        color_off, _ = col(t('points'), t('normals'), t('view_dirs'), t('feats'), None, step=0)
    col.cfg['human_light'] = True
    hl = inter['human_light'].detach().numpy()
    hit = np.abs(hl).max(1) > 0
    diff = np.abs(color.detach().numpy() - color_off.numpy()).max(1)
    assert hit.sum() >= 128, int(hit.sum())
    assert float(np.median(diff[hit])) >= 100 * COLOUR_TOL, float(np.median(diff[hit]))
    assert float(diff[~hit].max()) == 0.0
    names = sorted(n for n, q in col.named_parameters() if q.grad is not None)
    gn = dict(col.named_parameters())
    assert sum(n.startswith('human_light_predictor.') for n in names) == 12
    res = {'kink_rows': kink.numpy(), 'color': color.detach().numpy(), 'color_off': color_off.numpy(), 'human_light': hl, 'd_normals': normals.grad.numpy(),
           'd_feats_head': feats.grad[:64].numpy().copy(), 'd_feats_rownorm': feats.grad.double().norm(dim=1).numpy(),
           'grad_names': np.asarray(['color_network.' + n for n in names]),
           'grad_norms': np.asarray([float(gn[n].grad.double().norm()) for n in names]),
           'param_names': np.asarray(['color_network.' + n for n, _ in col.named_parameters() if n.startswith('human_light_predictor.')]),
           'param_shapes': np.asarray([list(q.shape) + [0] * (2 - q.dim()) for n, q in col.named_parameters()
                                       if n.startswith('human_light_predictor.')]),
           **{'override__' + k: v for k, v in over.items()}}
    np.savez_compressed(os.path.join(OUT, f'human_light_shading_sd{int(sd)}.npz'), **res)
    print('shading sd', sd, 'hit rows', int(hit.sum()), 'median on/off colour difference', float(np.median(diff[hit])),
          'max image', float(hl.max()))


def gen_render():
    from network.renderer_zerothick import NeROShapeRenderer as RefStd   # reference, the renderer of the core_step*_r48 fixtures
    from network.loss import name2loss
    from nu_nerf_amd.synthetic import make_jitter
    cfg = {'name': 'golden_hl', 'network': 'shape', 'database_name': 'custom/x/720', 'apply_occ_loss': True,
           'occ_loss_step': 15000, 'is_nerf': False, 'freeze_inv_s_step': 15000, 'eikonal_weight': 0.05, 'get_mask': False,
           'shader_config': dict(SHADER, sphere_direction=False, refrac_freq=3),      # (this renderer's per-ray mirror query is 72-d)
           'loss': ['nerf_render', 'eikonal', 'std', 'init_sdf_reg', 'occ', 'outer_reg'],
           'outer_reg_loss_weight': 0.1, 'n_samples': 32, 'n_importance': 32, 'n_bg_samples': 16}
    net = RefStd(cfg, training=False)
    p, over = color_params(False, rf=3)
    # a transparent background and a sharp surface, as the eval fixture (oracle/gen_golden_eval.py): the expected depth of the
    # validation pass then lands on the SDF surface and the human_light image is not masked out
    over['deviation_network.variance'] = p['deviation_network.variance'] = np.asarray(0.55, np.float32)
    over['outer_nerf.alpha_linear.bias'] = p['outer_nerf.alpha_linear.bias'] = np.full((1,), -10.0, np.float32)
    print('load_state_dict:', net.load_state_dict(to_t(p), strict=True))
    losses = [name2loss[n](cfg) for n in cfg['loss']]
    R, step, n_img = 24, 20000, 3
    cams = HO.camera_poses(n_img, 515, dist=2.0)
    g = np.random.Generator(np.random.PCG64(516))
    idxs = np.repeat(np.arange(n_img), R // n_img)
    dirs = np.concatenate([g.uniform(-0.22, 0.22, (R, 2)), np.ones((R, 1))], 1).astype(np.float32)     # pixel directions K^-1 (u, v, 1)
    poses = torch.from_numpy(cams)
    # rays and human frames through the reference's own functions (pose by pose: get_human_coordinate_poses writes in place into
    # an expanded tensor and raises for more than one pose under the installed torch, oracle/gen_golden_r2.py)
    hp = torch.cat([net.get_human_coordinate_poses(poses[i:i + 1].clone()) for i in range(n_img)], 0)
    assert np.allclose(hp.numpy(), HO.human_poses(cams), atol=1e-6)
    it = torch.from_numpy(idxs).long()
    o = (poses[:, :, :3].permute(0, 2, 1) @ -poses[:, :, 3:])[it, :, 0]
    dn = F.normalize((poses[it, :, :3].permute(0, 2, 1) @ torch.from_numpy(dirs).unsqueeze(-1))[..., 0], dim=-1)
    hpr = hp[it]
    rgbs = torch.from_numpy(g.uniform(0, 1, (R, 3)).astype(np.float32))
    u1, u2 = make_jitter(R, cfg['n_bg_samples'], seed=523)
    draws = [torch.from_numpy(u1), torch.from_numpy(u2)]
    real_rand = torch.rand
    torch.rand = lambda *a, **k: draws.pop(0)
    try:
        near, far = net.near_far_from_sphere(o, dn)
        net.zero_grad()
        z = net.sample_ray(o, dn, near, far, 1.0)
        outputs = net.render_core(o, dn, z, hpr, cos_anneal_ratio=net.get_anneal_val(step), step=step, is_train=True, is_nerf=False)
    finally:
        torch.rand = real_rand
    outputs['loss_rgb'] = net.compute_rgb_loss(outputs['ray_rgb'], rgbs)
    log = {}
    for ls in losses:
        log.update(ls(outputs, {}, step))
    total = 0
    for k, v in log.items():
        if k.startswith('loss'):
            total = total + torch.mean(v)
    total.backward()
    res = {'rays_o': o.numpy(), 'rays_d': dn.numpy(), 'human_poses_rays': hpr.numpy(), 'rgbs': rgbs.numpy(), 'step': np.asarray(step),
           'z_vals': z.numpy(), 'total_loss': total.detach().numpy(), **{'override__' + k: v for k, v in over.items()}}
    for k in ('ray_rgb', 'acc', 'color_bkgr', 'color_spec', 'gradient_error', 'loss_occ', 'loss_rgb'):
        res['out_' + k] = outputs[k].detach().numpy()
    assert np.isfinite(float(total.detach()))
    for k, v in log.items():
        if k.startswith('loss'):
            res['term_' + k] = torch.mean(v).detach().numpy()
    gn = {n: q.grad for n, q in net.named_parameters() if q.grad is not None}
    assert sum('human_light_predictor' in n for n in gn) == 12
    res['grad_names'] = np.asarray(sorted(gn.keys()))
    res['grad_norms'] = np.asarray([float(gn[k].double().norm()) for k in sorted(gn.keys())])
    for k in ('color_network.human_light_predictor.0.weight_v', 'color_network.human_light_predictor.6.bias',
              'color_network.roughness_predictor.6.bias', 'sdf_network.lin0.weight_v'):
        res['grad__' + k] = gn[k].numpy().copy()
    # the same rays with the key off: the feature must be visible in the training colour
    net.color_network.cfg['human_light'] = False
    with torch.no_grad():
        off = net.render_core(o, dn, z, hpr, cos_anneal_ratio=net.get_anneal_val(step), step=step, is_train=True, is_nerf=False)
    net.color_network.cfg['human_light'] = True
    res['out_ray_rgb_off'] = off['ray_rgb'].numpy()
    d_on_off = np.abs(res['out_ray_rgb'] - res['out_ray_rgb_off']).max(1)
    # (rays whose surface reflection misses the photographer's disc change by rounding only: at least a third of the rays must hit)
    assert int((d_on_off >= 100 * COLOUR_TOL).sum()) >= R // 3, np.sort(d_on_off)
    # validation pass at the same z (compute_validation_info)
    with torch.no_grad():
        ev = net.render_core(o, dn, z, hpr, cos_anneal_ratio=0.0, step=step, is_train=False, is_nerf=False)
    for k in ('ray_rgb', 'human_light', 'depth', 'specular_light', 'roughness'):
        res['eval_' + k] = ev[k].detach().numpy()
    assert float(res['eval_human_light'].max()) > 0.05, float(res['eval_human_light'].max())
    np.savez_compressed(os.path.join(OUT, 'human_light_render.npz'), **res)
    print('render loss', float(total), {k: float(v) for k, v in res.items() if k.startswith('term_')}, 'rays changed by the key',
          int((d_on_off >= 100 * COLOUR_TOL).sum()), 'eval human_light max', float(res['eval_human_light'].max()),
          'inner points', int(outputs['gradient_error'].numel()))


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import network.field as rfield
    which = sys.argv[1:] or ['encode', 'shading', 'render']
    if 'encode' in which:
        gen_encode(rfield)
    if 'shading' in which:
        gen_shading(rfield, False)
        gen_shading(rfield, True)
    if 'render' in which:
        gen_render()


if __name__ == '__main__':
    main()
