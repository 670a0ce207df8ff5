"""shader_config.human_light on the device: the encoder pair and the blended BRDF mix against the float64 oracle
(tests/human_light_oracle.py), the whole shading and a render_core step against fixtures written by the reference's own modules
(scripts/gen_human_light_golden.py), and the key switched off against the path that never builds the new code.

Tolerances
  * encoder forward / backward: 4 x the largest deviation of the REFERENCE's fp32 evaluation (its fp32 autograd for the gradients) from
    the float64 oracle on the same 1000 rows, stored in tests/golden/human_light_encode.npz (enc_dev 7.1e-7, dn_dev 9.2e-6 on gradients
    up to 19, dlogit_dev 6.9e-7 on gradients up to 1.0); the 4 x is the project's margin for a different but valid fp32 order.
  * blended mix: colour rtol 1e-5 / atol 1e-6 and gradients 3e-4 of the largest element + 1e-7 -- the bounds
    tests/test_stage2_ops_gpu.py::test_fused_brdf_mix_matches_the_eager_shading holds the same kernel's other instantiations to.
  * whole shading / render step: the bounds of tests/test_core_parity_gpu.py for the same kinds of quantities (colour rtol 1e-4 /
    atol 2e-6, loss terms 1e-4, gradient norms and stored gradients 3e-4; the occlusion target's second sampler keeps inner_weight
    at 2e-3), validation images rtol 1e-3 / atol 5e-4 (tests/test_eval_gpu.py).
"""
import functools

import numpy as np
import pytest
import torch

import human_light_oracle as HO
from helpers import golden, rel_err

pytestmark = pytest.mark.gpu

COLOUR_TOL = 1e-4
NORM_TOL = ELEM_TOL = 3e-4
SHADER = {'human_light': True, 'light_exp_max': 5.0}


def host(t):
    return t.detach().cpu().double()


@pytest.fixture(scope="module")
def L(gpu):
    from nu_nerf_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def encode_case():
    """Inputs, fixture and the float64 oracle (values and autograd gradients) of the encoder tests: computed once."""
    I, fx = HO.encode_inputs(), golden('human_light_encode.npz')
    n64 = torch.from_numpy(I['n']).double().requires_grad_(True)
    lg64 = torch.from_numpy(I['mraw'][:, 1:2].copy()).double().requires_grad_(True)
    o = HO.encode_chain(I, torch.float64, n64, lg64)
    dn, dl = torch.autograd.grad((o['enc'] * torch.from_numpy(I['g']).double()).sum(), (n64, lg64))
    return I, fx, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in o.items()}, dn, dl


def run_encode_fwd(L, gpu, I, poses=None, ld_hl=64):
    P = I['n'].shape[0]
    d = {k: torch.from_numpy(np.ascontiguousarray(I[k])).to(gpu) for k in ('n', 'pt', 'mraw', 'idx')}
    d['poses'] = torch.from_numpy(I['poses'] if poses is None else poses).to(gpu)
    HL, rec = torch.full((P, ld_hl), float('nan'), device=gpu), torch.full((P, 4), float('nan'), device=gpu)
    L.load().nu_human_encode_fwd(L.ptr(d['n']), L.ptr(d['pt']), 8, L.ptr(d['mraw']), 8, L.ptr(d['idx']), I['S'], L.ptr(d['poses']),
                                 d['poses'].shape[0], P, ld_hl, L.ptr(HL), L.ptr(rec), L.stream())
    torch.cuda.synchronize()
    return d, HL, rec


def test_encode_forward_vs_float64(gpu, L):
    """P = 1000 (a partial 256-lane block), S = 5 (idx // S gather), 3 poses; every branch of the hit flag is in the set."""
    I, fx, o, _, _ = encode_case()
    P = I['n'].shape[0]
    hit64, near = o['hit'].numpy(), o['near'].numpy()
    assert np.array_equal(hit64, fx['hit']) and int(fx['n_near']) == 0            # the oracle here is the generator's
    n_hit, n_behind, n_outside, n_noplane = (int(v) for v in fx['counts'])
    assert min(n_hit, n_behind, n_outside) > 50 and n_noplane == 4                # hits, dist <= 0, |mean| >= 1.5, |r'_z| <= 1e-4 (both signs)
    _, HL, rec = run_encode_fwd(L, gpu, I)
    hit = rec[:, 0].cpu().numpy() > 0.5
    assert set(np.unique(rec[:, 0].cpu().numpy())) <= {0.0, 1.0}
    assert near.sum() <= 0.01 * P
    keep = ~near
    assert np.array_equal(hit[keep], hit64[keep]), np.nonzero(hit != hit64)[0]
    assert not hit[:4].any()                                                       # the hand-placed near-parallel rows
    tol = 4.0 * float(fx['enc_dev'])
    enc = host(HL[:, :24])
    err = (enc - o['enc'])[torch.from_numpy(keep)].abs().max()
    print(f"HUMAN-LIGHT encode fwd: max err {float(err):.3g}, bound {tol:.3g} (reference fp32 deviation {float(fx['enc_dev']):.3g})")
    assert bool(torch.isfinite(enc).all()) and float(err) <= tol
    assert float(HL[:, 24:].abs().max()) == 0.0                                    # zero padding up to the GEMM's K
    non = torch.from_numpy(~hit)
    assert torch.equal(HL[:, :24].cpu()[non], HO.non_hit_row()[None].expand(int(non.sum()), 24))     # exactly IPE(0, 0)
    r = rec.cpu()
    assert float(r[non][:, 1:].abs().max()) == 0.0
    torch.testing.assert_close(r[~non][:, 1].double(), o['dist'][~non], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r[~non][:, 2:].double(), o['mean'][~non], rtol=1e-5, atol=2e-6)


def test_encode_selects_instead_of_multiplying(gpu, L):
    """A NaN in t_x of pose 2 makes mean_x NaN on EVERY row of that pose, rows that would otherwise hit included: none of them may
    hit (each comparison of the hit flag is false on NaN), all of them must encode IPE(0, 0) exactly -- selected, so no NaN reaches
    the output -- and the rows of the other poses are untouched.  The inputs are otherwise finite; nothing faults."""
    I, fx, o, _, _ = encode_case()
    ray = I['idx'] // I['S']
    poses = I['poses'].copy()
    poses[2, 0, 3] = np.nan                    # t_x of pose 2: x'_x, hence mean_x, of every row of pose 2
    _, HL, rec = run_encode_fwd(L, gpu, I, poses)
    assert bool(torch.isfinite(HL).all()) and bool(torch.isfinite(rec).all())
    sel = torch.from_numpy(ray == 2)
    assert float(rec[:, 0].cpu()[sel].max()) == 0.0 and int(sel.sum()) > 100
    assert torch.equal(HL[:, :24].cpu()[sel], HO.non_hit_row()[None].expand(int(sel.sum()), 24))
    _, HL0, rec0 = run_encode_fwd(L, gpu, I)
    assert torch.equal(HL.cpu()[~sel], HL0.cpu()[~sel]) and torch.equal(rec.cpu()[~sel], rec0.cpu()[~sel])


def test_encode_rejects_short_rows_and_unaligned_records(gpu, L):
    """Both are refused by the host entry before anything is launched: rows shorter than the 24 columns, and a record buffer that is
    not 16-byte aligned (the kernel stores the record as one float4)."""
    I = HO.encode_inputs()
    with pytest.raises(L.NuNerfLibraryError):
        run_encode_fwd(L, gpu, I, ld_hl=16)
    P = I['n'].shape[0]
    d = {k: torch.from_numpy(np.ascontiguousarray(I[k])).to(gpu) for k in ('n', 'pt', 'mraw', 'idx', 'poses')}
    HL, rec = torch.zeros(P, 64, device=gpu), torch.zeros(P + 1, 4, device=gpu)
    with pytest.raises(L.NuNerfLibraryError):
        L.load().nu_human_encode_fwd(L.ptr(d['n']), L.ptr(d['pt']), 8, L.ptr(d['mraw']), 8, L.ptr(d['idx']), I['S'], L.ptr(d['poses']), 3, P, 64,
                                     L.ptr(HL), L.c_p(rec.data_ptr() + 4), L.stream())
    with pytest.raises(L.NuNerfLibraryError):
        L.load().nu_human_encode_bwd(L.ptr(d['n']), L.ptr(d['pt']), 8, L.ptr(d['mraw']), 8, L.ptr(d['idx']), I['S'], L.ptr(d['poses']), 3,
                                     L.c_p(rec.data_ptr() + 4), L.ptr(HL), 64, P, L.ptr(torch.zeros(P, 3, device=gpu)),
                                     L.ptr(torch.zeros(P, 8, device=gpu)), 8, L.stream())
    torch.cuda.synchronize()
    assert float(HL.abs().max()) == 0.0


def test_encode_backward_vs_float64_autograd(gpu, L):
    I, fx, o, dn64, dl64 = encode_case()
    P = I['n'].shape[0]
    d, HL, rec = run_encode_fwd(L, gpu, I)
    g = torch.zeros(P, 64, device=gpu)
    g[:, :24] = torch.from_numpy(I['g']).to(gpu)
    g[:, 24:] = float('nan')                     # the padding's cotangent is never read
    gen = torch.Generator().manual_seed(5)
    pat_n, pat_m = torch.randn(P, 3, generator=gen).to(gpu), torch.randn(P, 8, generator=gen).to(gpu)
    dn, dm = pat_n.clone(), pat_m.clone()
    L.load().nu_human_encode_bwd(L.ptr(d['n']), L.ptr(d['pt']), 8, L.ptr(d['mraw']), 8, L.ptr(d['idx']), I['S'], L.ptr(d['poses']),
                                 d['poses'].shape[0], L.ptr(rec), L.ptr(g), 64, P, L.ptr(dn), L.ptr(dm), 8, L.stream())
    torch.cuda.synchronize()
    hit = rec[:, 0].cpu() > 0.5
    keep = torch.from_numpy(~o['near'].numpy())
    # accumulation: pattern + gradient; rows without a hit and every column but the roughness logit keep the pattern bit for bit
    assert torch.equal(dn.cpu()[~hit], pat_n.cpu()[~hit]) and torch.equal(dm.cpu()[~hit], pat_m.cpu()[~hit])
    cols = [0, 2, 3, 4, 5, 6, 7]
    assert torch.equal(dm.cpu()[:, cols], pat_m.cpu()[:, cols])
    got_n, got_l = host(dn) - host(pat_n), host(dm[:, 1:2]) - host(pat_m[:, 1:2])
    # (the subtraction of the pattern costs one rounding of pattern + gradient: 2^-24 of |pattern| + |gradient|, inside the bounds)
    tol_n, tol_l = 4.0 * float(fx['dn_dev']), 4.0 * float(fx['dlogit_dev'])
    en, el = float((got_n - dn64)[keep].abs().max()), float((got_l - dl64)[keep].abs().max())
    print(f"HUMAN-LIGHT encode bwd: dn err {en:.3g} (bound {tol_n:.3g}, max |dn| {float(dn64.abs().max()):.3g}), "
          f"dlogit err {el:.3g} (bound {tol_l:.3g})")
    slack_n = 2.0 ** -23 * (float(pat_n.abs().max()) + float(dn64.abs().max()))
    slack_l = 2.0 ** -23 * (float(pat_m.abs().max()) + float(dl64.abs().max()))
    assert en <= tol_n + slack_n and el <= tol_l + slack_l
    assert float(dn64[~hit].abs().max()) == 0.0 and float(dn64[hit].abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------ blended mix
def combine_inputs(P=1000, seed=77):
    """Raw heads of every stack for P rows: a third of the rows without a hit, raw human heads on both sides of the exp_max = 0 cap
    (w = 1 exactly above it, the upper clamp end) and down to -12 (w = 6e-6: exp never reaches the lower clamp end 0, this is as
    close as a finite head gets)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    hl = 1.2 * rn(P, 4) - 0.6
    hl[:40, 3] = 2.0 + rn(40).abs()            # w clamps at 1
    hl[40:80, 3] = -12.0                        # w ~ 0
    hl[80:120, :3] = 1.0 + rn(40, 3).abs()     # h capped at exp(0)
    hit = torch.rand(P, generator=g) > 0.33
    rec = torch.zeros(P, 4)
    rec[:, 0] = hit.float()
    rec[:, 1:] = rn(P, 3)
    return {'mraw': rn(P, 6), 'ol': 0.8 * rn(3 * P, 3) - 0.7, 'il': 0.8 * rn(2 * P, 3) - 0.7, 'iw': 1.5 * rn(P, 1), 'rl': 0.8 * rn(P, 3) - 0.7,
            'hl': hl, 'nov': (2 * torch.rand(P, 1, generator=g) - 0.6).clamp(-0.5, 1.0), 'rec': rec, 'hit': hit, 'gcol': rn(P, 3)}


def test_combine_with_human_light_vs_float64(gpu):
    from nu_nerf_amd import stage2_ops as O
    from nu_nerf_amd.params import load_fg_lut

    class Eng:          # what the two combine ops read from an engine
        pass
    from nu_nerf_amd import _lib
    eng = Eng()
    eng.lib, eng.stream = _lib.load(), _lib.stream
    C = combine_inputs()
    P, exp_max = C['mraw'].shape[0], 5.0
    lut = torch.from_numpy(load_fg_lut())
    names = ('mraw', 'ol', 'il', 'iw', 'rl', 'hl', 'nov')
    # float64 oracle and its autograd
    ins64 = [C[k].double().requires_grad_(True) for k in names]
    col64, hw64 = HO.combine(*ins64[:5], ins64[6], lut[0].double(), exp_max, hl=ins64[5], hit=C['hit'])
    g64 = torch.autograd.grad((col64 * C['gcol'].double()).sum(), ins64)
    # device
    ins = [C[k].to(gpu).requires_grad_(True) for k in names]
    lut_d = lut.to(gpu)
    col, hw = O.shade_combine_hl(eng, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], C['rec'].to(gpu), ins[6], lut_d, exp_max)
    grads = torch.autograd.grad((col * C['gcol'].to(gpu)).sum(), ins)
    torch.testing.assert_close(host(col), col64.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(host(hw[:, :3]), hw64.detach(), rtol=1e-5, atol=1e-6)
    h64, w64 = HO.heads(C['hl'].double(), C['hit'])
    torch.testing.assert_close(host(hw[:, 3:]), w64, rtol=1e-5, atol=1e-6)
    assert float(w64[:40][C['hit'][:40]].min()) == 1.0 and float(w64[40:80].max()) < 1e-5 and float(h64[80:120][C['hit'][80:120]].min()) == 1.0
    for name, a, b in zip(names, grads, g64):
        scale = float(b.abs().max())
        err = float((host(a) - b).abs().max())
        print(f"HUMAN-LIGHT combine d{name}: err {err:.3g} of scale {scale:.3g}")
        assert err <= 3e-4 * scale + 1e-7, (name, err, scale)
    # rows without a hit: bit for bit today's mix, and no gradient to the human heads
    col0, _ = O.shade_combine(eng, ins[0], ins[1], ins[2], ins[3], ins[4], ins[6], lut_d, exp_max)
    non = ~C['hit']
    assert int(non.sum()) > 200 and torch.equal(col.detach().cpu()[non], col0.detach().cpu()[non])
    assert float(grads[5].cpu()[non].abs().max()) == 0.0 and float(hw.cpu()[non].abs().max()) == 0.0
    assert float((col.detach() - col0.detach()).abs().cpu()[C['hit']].max()) > 100 * COLOUR_TOL
    # the cap of exp(min(raw, 0)): no gradient above it
    capped = (C['hl'] > 0) & C['hit'][:, None]
    assert int(capped.sum()) > 50 and float(grads[5].cpu()[capped].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ whole shading vs the reference
def build_net(gpu, fx, sd, rf=6, cls=None, **cfg_over):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    if cls is None:
        from nu_nerf_amd.renderer import NeROShapeRenderer as cls
    cfg = {'name': 'hl', 'network': 'shape', 'is_nerf': False, 'shader_config': dict(SHADER, sphere_direction=sd, refrac_freq=rf)}
    cfg.update(cfg_over)
    net = cls(cfg, training=False)
    params = randomize_for_parity(init_stage1_params(6033, sphere_direction=sd, refrac_freq=rf, human_light=True), seed=1)
    n_over = 0
    for k in fx:
        if k.startswith('override__'):
            params[k[len('override__'):]] = fx[k]
            n_over += 1
    assert n_over >= 2
    net.load_param_dict(params)
    return net.to(gpu)


def check_shading(fx, color, hl_img, d_normals, d_feats, named):
    np.testing.assert_allclose(color.detach().cpu().numpy(), fx['color'], rtol=1e-4, atol=2e-6)
    if hl_img is not None:
        np.testing.assert_allclose(hl_img.detach().cpu().numpy(), fx['human_light'], rtol=1e-4, atol=2e-6)
    # per-row input gradients: rows that sit on a ReLU kink in the reference (a hidden pre-activation within 1e-6 of zero, the
    # rounding uncertainty of a 256-term fp32 dot product; marked by the generator) are left out -- there the reference's own
    # gradient jumps under any other valid fp32 order.  At most 10 % of the rows; colours and parameter gradients keep every row.
    keep = torch.from_numpy(~fx['kink_rows'])
    assert int(keep.sum()) >= 0.9 * keep.numel()
    e_n = rel_err(d_normals.cpu()[keep], fx['d_normals'][keep.numpy()])
    e_f = rel_err(d_feats[:64].cpu()[keep[:64]], fx['d_feats_head'][keep[:64].numpy()])
    print(f"HUMAN-LIGHT shading: d normals rel err {e_n:.3g}, d features rel err {e_f:.3g} (rows left out: {int((~keep).sum())})")
    assert e_n < ELEM_TOL and e_f < ELEM_TOL, (e_n, e_f)
    np.testing.assert_allclose(d_feats.double().norm(dim=1).cpu().numpy()[keep.numpy()], fx['d_feats_rownorm'][keep.numpy()], rtol=NORM_TOL,
                               atol=1e-7)
    bad, n_human = [], 0
    for n, ref in zip([str(s) for s in fx['grad_names']], fx['grad_norms']):
        gr = named[n].grad
        assert gr is not None, n
        n_human += 'human_light_predictor' in n
        err = abs(float(gr.double().norm()) - ref) / (ref + 1e-12)
        if err > NORM_TOL:
            bad.append((round(err, 7), n))
    assert n_human == 12 and not bad, sorted(bad, reverse=True)[:12]


def assert_fixture_shows_the_light(fx):
    hit = np.abs(fx['human_light']).max(1) > 0
    diff = np.abs(fx['color'] - fx['color_off']).max(1)
    assert hit.sum() >= 128 and float(np.median(diff[hit])) >= 100 * COLOUR_TOL and float(diff[~hit].max()) == 0.0


@pytest.mark.parametrize("sd", [False, True])
def test_whole_shading_through_the_network_ops_vs_reference(gpu, sd):
    """AppShadingNetwork.forward on 512 points through shading_glue.shade: the rendering form (fused encoders + blended mix) and
    the validation form (term by term, with the human_light image)."""
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.shading_glue import shade
    fx, I = golden(f'human_light_shading_sd{int(sd)}.npz'), HO.shading_inputs()
    assert_fixture_shows_the_light(fx)
    net = build_net(gpu, fx, sd)
    eng = net.engine()
    eng.pack()
    nets = Stage1Nets(eng, net._named())
    cn = net.color_network
    t = lambda k: torch.from_numpy(I[k]).to(gpu)
    named = dict(net.named_parameters())
    for inter in (False, True):
        net.zero_grad(set_to_none=True)
        nets.begin_pass()
        normals, feats = t('normals').requires_grad_(True), t('feats').requires_grad_(True)
        out = shade(nets, cn.cfg, cn.FG_LUT, t('points'), normals, t('view_dirs'), feats, inter_results=inter, human_poses=t('human_poses'))
        color = out[0]
        (color * t('gcol')).sum().backward()
        check_shading(fx, color, out[2]['human_light'] if inter else None, normals.grad, feats.grad, named)
    with pytest.raises(ValueError, match="human_poses"):
        shade(nets, cn.cfg, cn.FG_LUT, t('points'), t('normals'), t('view_dirs'), t('feats'))


@pytest.mark.parametrize("sd", [False, True])
def test_whole_shading_through_the_engine_vs_reference(gpu, sd):
    """The same 512 points through Stage1Engine.shading_forward / shading_backward (the training path: launch by launch with the
    fifth stack), one sample per ray so that row p reads human_poses[p]; d features and d normals are the engine's dYX / dn."""
    from nu_nerf_amd.engine import addr
    fx, I = golden(f'human_light_shading_sd{int(sd)}.npz'), HO.shading_inputs()
    net = build_net(gpu, fx, sd)
    eng = net.engine()
    eng.pack()
    assert eng.human_light and len(eng.human_pred) == 4
    t = lambda k: torch.from_numpy(I[k]).to(gpu)
    P = I['points'].shape[0]
    pt = torch.zeros(P, 8, device=gpu)
    pt[:, :3], pt[:, 4:7] = t('points'), -t('view_dirs')
    idx = torch.arange(P, dtype=torch.int32, device=gpu)
    # the SDF activations the shading reads: feature columns of YX, the position embedding E, the raw normal n
    a = eng.sdf_forward(addr(pt), 8, P, keep=True)
    a['YX'][:, 1:257] = t('feats')
    a['n'] = t('normals').contiguous()
    color_rm = torch.zeros(P, 4, device=gpu)
    s = eng.shading_forward(a, pt, idx, P, color_rm, human_poses=t('human_poses'), S_ray=1)
    flat = eng.zeros(eng.n_grad)
    dcol = torch.zeros(P, 4, device=gpu)
    dcol[:, :3] = t('gcol')
    dYX, dn = eng.shading_backward(a, s, pt, idx, dcol, flat)
    eng.unpack_grads(flat)
    torch.cuda.synchronize()

    class G:
        def __init__(self, g):
            self.grad = g
    named = {n: G(flat[off:off + eng.grad_numel[n]].view(shape)) for n, (off, shape) in eng.grad_views.items()}
    hw = s['hw'][:, :3]
    from nu_nerf_amd import torch_glue as TG
    check_shading(fx, color_rm[:, :3], TG.linear_to_srgb(hw), dn, dYX[:, 1:257], named)


# ------------------------------------------------------------------------------------------------ render step vs the reference
def test_render_core_step_vs_reference(gpu):
    """The reference's render_core at its own z_vals: 24 rays from 3 poses, 32 / 32 / 16 samples, real-capture path, human_light on:
    per-ray outputs, every loss term, all gradient norms (the twelve of the human-light predictor among them), and the
    human_light image of the validation pass."""
    from nu_nerf_amd.loss import name2loss, total_loss
    fx = golden('human_light_render.npz')
    d_on_off = np.abs(fx['out_ray_rgb'] - fx['out_ray_rgb_off']).max(1)
    assert int((d_on_off >= 100 * COLOUR_TOL).sum()) >= 8            # the key is visible in the expected colours
    cfg = {'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000, 'eikonal_weight': 0.05, 'outer_reg_loss_weight': 0.1,
           'n_samples': 32, 'n_importance': 32, 'n_bg_samples': 16}
    net = build_net(gpu, fx, False, rf=3, **cfg)
    full_cfg = dict(net.cfg)
    step = int(fx['step'])
    t = lambda k: torch.from_numpy(fx[k]).to(gpu)
    o, dn, z, hp = t('rays_o'), t('rays_d'), t('z_vals'), t('human_poses_rays')
    out = net.render_core(o, dn, z, hp, cos_anneal_ratio=net.get_anneal_val(step), step=step, is_train=True, is_nerf=False)
    out['loss_rgb'] = net.compute_rgb_loss(out['ray_rgb'], t('rgbs'))
    losses = [name2loss[n](full_cfg) for n in ('nerf_render', 'eikonal', 'std', 'init_sdf_reg', 'occ', 'outer_reg')]
    total, log = total_loss(out, losses, step)
    total.backward()
    for k in ('ray_rgb', 'acc', 'color_bkgr', 'color_spec'):
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), fx['out_' + k], rtol=1e-4, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(out['gradient_error'].detach().cpu().numpy(), fx['out_gradient_error'], rtol=1e-4, atol=1e-6)
    n_terms = 0
    for k in fx:
        if k.startswith('term_'):
            np.testing.assert_allclose(float(torch.mean(log[k[5:]]).detach()), float(fx[k]), rtol=1e-4, atol=1e-7, err_msg=k)
            n_terms += 1
    assert n_terms >= 4
    np.testing.assert_allclose(float(total.detach()), float(fx['total_loss']), rtol=1e-5)
    named = dict(net.named_parameters())
    bad, n_human = [], 0
    for n, ref_norm in zip([str(s) for s in fx['grad_names']], fx['grad_norms']):
        tol = 2e-3 if 'inner_weight' in n else NORM_TOL           # the occlusion target's own sampler (tests/test_core_parity_gpu.py)
        n_human += 'human_light_predictor' in n
        err = abs(float(named[n].grad.double().norm()) - ref_norm) / (ref_norm + 1e-12)
        if err > tol:
            bad.append((round(err, 7), n))
    for k in fx:
        if k.startswith('grad__'):
            err = rel_err(named[k[6:]].grad.cpu(), fx[k])
            if err > ELEM_TOL:
                bad.append((round(err, 7), k))
    assert n_human == 12 and not bad, sorted(bad, reverse=True)[:12]
    # validation pass at the same z
    net.zero_grad(set_to_none=True)
    with torch.no_grad():
        ev = net.render_core(o, dn, z, hp, cos_anneal_ratio=0.0, step=step, is_train=False, is_nerf=False)
    assert float(fx['eval_human_light'].max()) > 0.05
    for k in ('human_light', 'specular_light', 'roughness'):
        a, b = ev[k].detach().cpu().numpy(), fx['eval_' + k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=5e-4, err_msg=k)
    np.testing.assert_allclose(ev['ray_rgb'].cpu().numpy(), fx['eval_ray_rgb'], rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("which", ["zero_thickness", "compat_real_capture"])
def test_train_step_and_panel_through_the_real_capture_entry_points(gpu, which):
    """A real-capture ray store with the key on, through the module's own entry points: train_step (rays and human frames from the
    camera poses), the trainer's losses, backward, test_step (the eval output carries `human_light`) and the validation panel with the
    extra image.  `compat_real_capture` is what a configs/shape/real/*.yaml resolves to: the `shape` class of the drop-in registry
    (network/renderer.py semantics: candidate rays at sample 64, spec points, loss_normal) with sphere_direction on and 64 / 32 / 16 samples per
    ray, the sizes of the existing reference step of that class (sample 64, the candidate point, must lie among the inner samples)."""
    from nu_nerf_amd import metrics
    from nu_nerf_amd.loss import name2loss, total_loss
    fx = golden('human_light_render.npz')
    if which == "compat_real_capture":
        from nu_nerf_amd.compat.network.renderer import name2renderer
        net = build_net(gpu, fx, True, rf=3, cls=name2renderer['shape'], database_name='custom/ballstatue/1080', zero_thickness=False,
                        get_mask=False, apply_occ_loss=True, occ_loss_step=15000, freeze_inv_s_step=15000, eikonal_weight=0.1,
                        outer_reg_loss_weight=0.1, n_samples=64, n_importance=32, n_bg_samples=16, train_ray_num=48, test_ray_num=64,
                        test_downsample_ratio=False)
        loss_names = ['nerf_render', 'eikonal', 'std', 'init_sdf_reg', 'occ', 'outer_reg', 'normal_ori']
    else:
        net = build_net(gpu, fx, False, rf=3, n_samples=16, n_importance=16, n_bg_samples=8, train_ray_num=48, test_ray_num=64,
                        test_downsample_ratio=False)
        loss_names = ['nerf_render', 'eikonal', 'std', 'init_sdf_reg', 'occ', 'outer_reg']
    cams = torch.from_numpy(HO.camera_poses(3, 515, dist=2.0))
    h = w = 12
    K = torch.tensor([[30.0, 0.0, w / 2], [0.0, 30.0, h / 2], [0.0, 0.0, 1.0]])
    gen = torch.Generator().manual_seed(3)
    info = {'imgs': torch.rand(3, 3, h, w, generator=gen), 'Ks': K[None].repeat(3, 1, 1), 'poses': cams}
    net.set_ray_store(info, {k: v[:1] for k, v in info.items()})
    out = net.train_step(20000)
    total, _ = total_loss(out, [name2loss[n](dict(net.cfg)) for n in loss_names], 20000)
    assert bool(torch.isfinite(total))
    total.backward()
    named = dict(net.named_parameters())
    for n in ('color_network.human_light_predictor.6.bias', 'color_network.human_light_predictor.0.weight_v', 'sdf_network.lin0.weight_v'):
        assert named[n].grad is not None and bool(torch.isfinite(named[n].grad).all()) and float(named[n].grad.abs().max()) > 0, n
    ev = net.test_step(0, 20000)
    assert ev['human_light'].shape == (h * w, 3) and bool(torch.isfinite(ev['human_light']).all())
    assert float(ev['human_light'].max()) > 0.01                     # some pixel sees the photographer
    img = metrics.panel(ev)
    assert img.shape[1] == 4 * w and img.shape[0] % h == 0
    assert torch.equal(img[:h, 3 * w:4 * w], metrics.to_uint8(ev['human_light']).reshape(h, w, 3))      # row 1, after the normal map
    assert torch.equal(img[:h, 2 * w:3 * w], metrics.to_uint8(ev['normal']).reshape(h, w, 3))


# ------------------------------------------------------------------------------------------------ off means off
def test_key_off_never_builds_the_new_path(gpu):
    """human_light: false: the engine has no fifth stack, shading takes the network-level C entries, and a seeded step gives bit
    for bit the outputs and the flat gradient of an engine whose launch-by-launch path -- the one the key-on code extends -- is
    forced (the two sequencings are bit-identical by tests/test_core_parity_gpu.py; this pins that the added branches are inert)."""
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.synthetic import make_object_rays
    cfg = {'name': 'off', 'network': 'shape', 'is_nerf': False, 'n_samples': 16, 'n_importance': 16, 'n_bg_samples': 8,
           'shader_config': {'sphere_direction': True, 'human_light': False, 'light_exp_max': 5.0}}
    rays = make_object_rays(64, seed=31, aim_radius=0.8)
    o = torch.from_numpy(rays['rays_o']).to(gpu)
    d = torch.nn.functional.normalize(torch.from_numpy(rays['rays_d']).to(gpu), dim=-1)
    res = []
    for py_seq in (False, True):
        net = NeROShapeRenderer(cfg, training=False)
        net.load_param_dict(randomize_for_parity(init_stage1_params(6033, sphere_direction=True), seed=1))
        net = net.to(gpu)
        eng = net.engine()
        eng.py_seq = py_seq
        assert not eng.human_light and eng.human_pred is None
        assert not any('human' in n for n in eng.grad_views)
        eng.pack()
        near, far = net.near_far_from_sphere(o, d)
        with torch.no_grad():
            z = net.sample_ray(o, d, near, far, 0.0)
        called = []
        real = eng._c_shading_forward
        eng._c_shading_forward = lambda *a, **k: (called.append(1), real(*a, **k))[1]
        out, ctx = eng.render_forward(o, d, z, 0.3, human_poses=torch.full((64, 3, 4), float('nan'), device=gpu))   # ignored when off
        assert bool(called) == (not py_seq) and 'HLo' not in ctx['shade']
        flat = eng.render_backward(ctx, torch.ones(64, 3, device=gpu), None, None)
        res.append((out['rgb'].clone(), flat.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][1].abs().max()) > 0
    # the gradient vector of the key-on engine is today's followed by the twelve new tensors: every existing slot keeps its offset
    fx = golden('human_light_shading_sd1.npz')
    on = build_net(gpu, fx, True).engine()
    off_views = eng.grad_views
    assert all(on.grad_views[n] == v for n, v in off_views.items())
    extra = [n for n in on.grad_views if n not in off_views]
    assert sorted(extra) == sorted(str(s) for s in fx['param_names'])
    assert on.n_grad == eng.n_grad + sum(on.grad_numel[n] for n in extra) and min(on.grad_views[n][0] for n in extra) == eng.n_grad
    assert len(on.layers) == len(eng.layers) + 4 and [l.name for l in on.layers[:len(eng.layers)]] == [l.name for l in eng.layers]
