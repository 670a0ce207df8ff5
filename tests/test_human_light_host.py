"""shader_config.human_light without a GPU: the parameter inventory against the reference's own name list (stored in the
fixtures by scripts/gen_human_light_golden.py), state-dict round trip, the two configuration guards, what `human_light: false` leaves
untouched, and the float64 oracle of the GPU tests against the fixtures' figures."""
import math

import numpy as np
import pytest
import torch

import human_light_oracle as HO
from helpers import golden

SHADER_ON = {'sphere_direction': True, 'human_light': True, 'light_exp_max': 5.0}


def cfg(**over):
    c = {'name': 'hl', 'network': 'shape', 'is_nerf': False, 'shader_config': dict(SHADER_ON)}
    c.update(over)
    return c


def test_init_params_match_the_reference_name_list():
    from nu_nerf_amd.params import init_stage1_params
    fx = golden('human_light_shading_sd1.npz')
    off = init_stage1_params(6033, sphere_direction=True)
    on = init_stage1_params(6033, sphere_direction=True, human_light=True)
    extra = [k for k in on if k not in off]
    assert extra == [str(s) for s in fx['param_names']] and len(extra) == 12
    for k, shape in zip(extra, fx['param_shapes']):
        assert list(on[k].shape) == [int(s) for s in shape[:on[k].ndim]], k
        assert on[k].dtype == np.float32
    # every other tensor is the same with the key on and off, and the new block sits between refrac_light and infinity_far_bkgr
    assert all(np.array_equal(on[k], off[k]) for k in off)
    names = list(on)
    assert names[names.index(extra[0]) - 1].startswith('color_network.refrac_light.6.')
    assert names[names.index(extra[-1]) + 1].startswith('infinity_far_bkgr.')
    np.testing.assert_allclose(on['color_network.human_light_predictor.6.bias'], math.log(0.01), rtol=1e-6)
    w = on['color_network.human_light_predictor.0.weight_v']
    assert w.shape == (256, 24) and float(np.abs(w).max()) <= 1 / math.sqrt(24) + 1e-6 and float(w.std()) > 0.05


def test_module_registers_the_predictor_and_round_trips_a_reference_state_dict():
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.renderer_std import NeROShapeRenderer as StdRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    fx = golden('human_light_shading_sd1.npz')
    for cls in (NeROShapeRenderer, StdRenderer):
        net = cls(cfg(), training=False)
        keys = list(net.state_dict())
        human = [k for k in keys if 'human_light_predictor' in k]
        assert human == [str(s) for s in fx['param_names']]                 # the reference's names, in its registration order
        sd = randomize_for_parity(init_stage1_params(77, sphere_direction=True, human_light=True), seed=4)
        ref = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
        assert set(ref) == set(keys)
        net.load_state_dict(ref, strict=True)
        back = net.state_dict()
        assert all(torch.equal(back[k], ref[k]) for k in ref)
        # a fresh module starts at the reference's head bias
        fresh = cls(cfg(), training=False).state_dict()['color_network.human_light_predictor.6.bias']
        torch.testing.assert_close(fresh, torch.full((4,), math.log(0.01)))
    off = NeROShapeRenderer(cfg(shader_config={'sphere_direction': True, 'human_light': False}), training=False)
    assert not any('human' in k for k in off.state_dict())
    with pytest.raises(RuntimeError):                                       # a checkpoint trained with the key needs the key
        off.load_state_dict(ref, strict=True)


def test_configuration_guards():
    from nu_nerf_amd.renderer import NeROShapeRenderer
    with pytest.raises(ValueError, match="camera poses"):
        NeROShapeRenderer(cfg(is_nerf=True), training=False)
    with pytest.raises(NotImplementedError, match="fp32"):
        NeROShapeRenderer(cfg(mlp_dtype='bf16'), training=False)
    NeROShapeRenderer(cfg(mlp_dtype='fp32'), training=False)


def test_compat_registry_constructs_a_real_capture_config_with_the_key():
    """configs/shape/real/*.yaml with human_light flipped to true, through the drop-in package."""
    from nu_nerf_amd.compat.network.renderer import name2renderer
    c = {'name': 'ballstatue', 'network': 'shape', 'database_name': 'custom/ballstatue/1080', 'shader_config': dict(SHADER_ON),
         'apply_occ_loss': True, 'occ_loss_step': 15000, 'get_mask': False, 'zero_thickness': False, 'is_nerf': False}
    net = name2renderer['shape'](c, training=False)
    assert net.color_network.cfg['human_light'] and hasattr(net.color_network, 'human_light_predictor')


def test_oracle_reproduces_the_fixture_and_its_own_fp32():
    """The float64 oracle gives the hit flags the generator stored (it agreed with the reference's fp32 there), no row of the input
    set sits next to a threshold, its fp32 evaluation flags the same rows, and non-hit rows encode IPE(0, 0) exactly."""
    fx, I = golden('human_light_encode.npz'), HO.encode_inputs()
    o64, o32 = HO.encode_chain(I, torch.float64), HO.encode_chain(I, torch.float32)
    assert np.array_equal(o64['hit'].numpy(), fx['hit']) and int(o64['near'].sum()) == int(fx['n_near']) == 0
    assert torch.equal(o32['hit'], o64['hit'])
    assert I['n'].shape == (1000, 3) and I['S'] == 5 and I['poses'].shape == (3, 3, 4) and int(I['idx'].max()) // 5 == 2
    non = ~o64['hit']
    assert torch.equal(o32['enc'][non], HO.non_hit_row()[None].expand(int(non.sum()), 24))
    assert float((o32['enc'].double() - o64['enc']).abs().max()) <= 4 * float(fx['enc_dev'])
    assert not o64['hit'][:4].any() and 1e-8 < float(fx['enc_dev']) < 5e-6 and float(fx['dn_dev']) < 1e-4


def test_fixtures_show_the_light():
    """Without this a no-op implementation passes: on hit rows the reference's colour with the key on differs from its colour with
    the key off by at least 100 x the colour tolerance of the GPU tests, w is around 0.5 and h of order 1."""
    for sd in (0, 1):
        fx = golden(f'human_light_shading_sd{sd}.npz')
        hit = np.abs(fx['human_light']).max(1) > 0
        diff = np.abs(fx['color'] - fx['color_off']).max(1)
        assert hit.sum() >= 128 and float(np.median(diff[hit])) >= 100 * 1e-4 and float(diff[~hit].max()) == 0.0
        assert 0.2 < float(fx['human_light'][hit].max()) <= 1.0
        assert sum('human_light_predictor' in str(n) for n in fx['grad_names']) == 12
        assert float(fx['grad_norms'].min()) > 0
    fx = golden('human_light_render.npz')
    assert int((np.abs(fx['out_ray_rgb'] - fx['out_ray_rgb_off']).max(1) >= 100 * 1e-4).sum()) >= 8
    assert fx['z_vals'].shape[0] == 24 and fx['human_poses_rays'].shape == (24, 3, 4)


def test_stage2_refuses_the_key_at_construction():
    """The key is a stage-1 feature: both stage-2 renderers refuse it when they build their inner shading network, as they always
    did -- no predictor is registered there and no render can reach the stage-1 code path without camera poses.  A stage-1 network
    trained WITH the key may sit inside a stage-2 module (stage1_cfg) whose own shader_config leaves it off."""
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.stage2 import Stage2Renderer as Zero
    from nu_nerf_amd.stage2_thick import Stage2Renderer as Thick
    base = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'stage1_mesh_arrays': icosphere(2, 0.5),
            'stage1_cfg': {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000, 'get_mask': False}}
    for cls in (Zero, Thick):
        with pytest.raises(NotImplementedError, match="human_light"):
            cls(dict(base, shader_config={'sphere_direction': False, 'human_light': True}), training=False)
        net = cls(dict(base, shader_config={'sphere_direction': False, 'human_light': False}), training=False)
        assert not any('human' in k for k in net.state_dict())


def test_panel_appends_the_human_light_image(monkeypatch):
    """metrics.panel's layout on the CPU (its quantiser is a device kernel: replaced here by the same formula in torch): with
    `human_light` in the outputs, row 1 is gt | prediction | normal | human_light, and without it the panel is what it was."""
    from nu_nerf_amd import metrics
    monkeypatch.setattr(metrics, 'to_uint8', lambda x: torch.clamp(x.detach().float() * 255.0, 0.0, 255.0).to(torch.uint8))
    h, w = 4, 5
    g = torch.Generator().manual_seed(9)
    data = {k: torch.rand(h, w, 3, generator=g) for k in ('gt_rgb', 'ray_rgb')}
    data.update({k: torch.rand(h * w, c, generator=g) for k, c in (('normal', 3), ('diffuse_albedo', 3), ('roughness', 1))})
    before = metrics.panel(data)
    assert before.shape == (2 * h, 3 * w, 3)
    data['human_light'] = torch.rand(h * w, 3, generator=g)
    img = metrics.panel(data)
    assert img.shape == (2 * h, 4 * w, 3)
    assert torch.equal(img[:h, 3 * w:], metrics.to_uint8(data['human_light']).reshape(h, w, 3))
    assert torch.equal(img[:, :3 * w], before) and int(img[h:, 3 * w:].max()) == 0          # everything else where it was
