"""The learned illumination read out on the GPU (csrc/light_bake.hip, nu_nerf_amd/environment.py): bit-identity with the layered path,
parity with a float64 evaluation and with the reference fixture, both sides of every clamp, row independence, the map convention,
every renderer class, the C entry's argument handling, the command.

Bounds.  LIGHT_RTOL (tests 2, 4 and 8) bounds the relative error of every radiance output (|mine - want| / |want|, per element; the
radiances here lie in 0.4 .. 0.6).  It is four times the largest deviation measured on an MI355X against the float64 oracle
(tests/environment_oracle.py) and against the reference fixture (never against the kernel itself; run to run there is no spread, the
margin is for another compiler's contraction choices), and may not exceed 1e-4, the colour tolerance of the stage-1 parity tests.
Measured: float64, 1 024 rows: light 3.9e-5 / 3.4e-5, indirect 4.2e-5 / 2.9e-5 (sphere_direction off / on); the probes of test 4:
9.9e-6 .. 1.8e-5; reference fixture: light 2.6e-5 / 2.5e-5, direct 2.6e-5 / 3.0e-5.  4 x 4.2e-5 = 1.7e-4, so the cap of 1e-4 is what is
asserted.
The deviation is not the networks': at rho = 0 the 16th-degree terms of the IDE carry fp32 rounding noise of 1e-3 in any fp32
evaluation (tests/encode_oracle.py IDE_KAPPA); the reference's own fp32 result is 2.9e-5 from the float64 oracle on the fixture's
rows (recorded in the fixture).  OCC_ATOL: the occlusion has no IDE input; absolute, four times the largest measured figure (6.6e-7 against
the fixture, 5.7e-7 against float64).
The layered path (test 1): encoded rows and raw heads are the same bits -- same encoding helpers (csrc/ide.h), same MFMA k order,
same epilogue, same head reduction.  exp is evaluated by the device's expf, held to EXP_ULPS = 2 units in the last place of
exp(min(raw, exp_max)) computed in float64 from the kernel's own raw head and rounded once."""
import functools
import os

import numpy as np
import pytest
import torch

import environment_oracle as EO
from helpers import golden

pytestmark = pytest.mark.gpu

LIGHT_RTOL = 1e-4
assert LIGHT_RTOL <= 1e-4
OCC_ATOL = 2.7e-6
EXP_ULPS = 2
SIZES = (1, 31, 32, 33, 97)


# ---- networks (the builders of tests/test_materials_gpu.py) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage1_arrays(sphere, gain=True):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = randomize_for_parity(init_stage1_params(6033, sphere_direction=sphere), seed=1)
    if gain:
        arrays.update(EO.head_gain_overrides(arrays))
    return arrays


def stage1_net(gpu, sphere=False, overrides=None, gain=True, cfg=None, cls=None):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    arrays = dict(stage1_arrays(sphere, gain))
    arrays.update(overrides or {})
    net = (cls or NeROShapeRenderer)(dict({'name': 'golden', 'shader_config': {'sphere_direction': sphere}}, **(cfg or {})), training=False)
    net.load_param_dict(arrays)
    return net.to(gpu), arrays


def stage2_net(gpu, overrides=None, thick=False):
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, init_stage2_thick_own_params, randomize_for_parity
    from nu_nerf_amd.lbvh import icosphere
    s1 = randomize_for_parity(init_stage1_params(6033), seed=1)
    s1cfg = {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000}
    cfg = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'shader_config': {'sphere_direction': False, 'human_light': False},
           'stage1_cfg': s1cfg, 'stage1_mesh_arrays': icosphere(3, 0.5)}
    if thick:
        from nu_nerf_amd.stage2_thick import Stage2Renderer
        cfg.update({'get_mask': False, 'is_nerf': False})
        cfg['stage1_cfg'] = dict(s1cfg, get_mask=False, is_nerf=False)
        net = Stage2Renderer(cfg, training=False)
        p2 = randomize_for_parity(init_stage2_thick_own_params(7044, net.color_network_inner.cfg), seed=3)
    else:
        from nu_nerf_amd.stage2 import Stage2Renderer
        net = Stage2Renderer(cfg, training=False)
        p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
    p2.update(overrides or {})
    sd = net.state_dict()
    for k in [k for k in p2 if k.startswith('stage1_network.')]:      # the aliases of the same tensors, where the model has them
        if 'color_network.' + k in sd:
            p2['color_network.' + k] = p2[k]
    net.load_param_dict(p2)
    return net.to(gpu), p2


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def ulp_distance(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()      # positive floats: monotone
    return int((ia - ib).abs().max())


def rel_dev(mine, want):
    return float((np.abs(mine.detach().cpu().numpy().astype(np.float64) - want) / np.abs(want)).max())


def exp_of_raw(raw, exp_max):
    """exp(min(raw, exp_max)) of fp32 raw heads in float64, rounded once to fp32 (exp_max as the kernel holds it: fp32)."""
    return torch.exp(torch.clamp(raw.double(), max=float(np.float32(exp_max)))).float()


def layered_outer(eng, named, d, x, sphere):
    """(rows [N, ld_ol], raw heads [N,3]) of the layered path at rho = 0: nu_spec_encode + three NT GEMMs + nu_skinny_fwd."""
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.engine import addr
    N = d.shape[0]
    rows = torch.empty(N, eng.ld_ol, device=d.device)
    with torch.no_grad():
        eng.pack()
        if sphere and x is None:
            x = torch.zeros(N, 3, device=d.device)
        eng.lib.nu_spec_encode(addr(d), addr(x) if sphere else 0, N, 1 if sphere else 0, addr(rows), eng.ld_ol, eng.stream())
        raw = Stage1Nets(eng, named).predictor('outer_light', rows)
    return rows, raw


# ---- 1. the layered path, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_direct_mode_is_the_layered_path_bits(gpu, sphere):
    from nu_nerf_amd.environment import bake_light
    from nu_nerf_amd import torch_glue as G
    net, _ = stage1_net(gpu, sphere)
    eng = net.engine()
    for n in SIZES + (1000,):
        d_np, rho_np, x_np = EO.rows(n, 100 + n, rim=min(n, 4))
        d, x = dev(d_np, gpu), dev(x_np, gpu)
        for pts in (None, x[n // 2].clone(), x):
            out = bake_light(net, d, 0.0, pts, _enc=True, _raw=True)
            xr = None if pts is None else (pts.expand(n, 3).contiguous() if pts.dim() == 1 else pts)
            rows, raw = layered_outer(eng, net._named(), d, xr, sphere)
            assert torch.equal(out['enc'], rows), (n, sphere)
            assert torch.equal(out['raw'][:, :3], raw), (n, sphere)
            assert torch.equal(out['raw'][:, 3:], torch.zeros_like(out['raw'][:, 3:]))
            want = exp_of_raw(raw, eng.exp_max)
            ulps = ulp_distance(out['light'], want)
            assert ulps <= EXP_ULPS, (n, ulps)
        # mixed roughness per row: the first 72 columns are nu_ide's bits at that roughness
        rho = dev(rho_np, gpu)
        out = bake_light(net, d, rho, x, _enc=True)
        assert torch.equal(out['enc'][:, :72], G.ide(d, rho[:, None]))
        assert torch.equal(out['enc'][:, (144 if sphere else 72):], torch.zeros(n, eng.ld_ol - (144 if sphere else 72), device=gpu))
    print(f"direct mode vs layered path (sphere_direction {sphere}): rows and raw heads bit-identical; exp within {EXP_ULPS} ulp")


@pytest.mark.parametrize("sphere", [False, True])
def test_rho_one_is_the_diffuse_block_of_the_shading_step(gpu, sphere):
    """At rho = 1 with per-row points the rows are the diffuse block (rows 0..P-1) of OLin / OLo that shading_forward keeps, for
    normals equal to d (the unit normals the step formed, read back from its SD record)."""
    from nu_nerf_amd.environment import bake_light
    from nu_nerf_amd.engine import addr
    net, _ = stage1_net(gpu, sphere)
    eng = net.engine()
    P = 97
    d_np, _, x_np = EO.rows(P, 321, rim=8)
    g = np.random.Generator(np.random.PCG64(322))
    pt = torch.zeros(P, 8, device=gpu)
    pt[:, :3], pt[:, 4:7] = dev(x_np, gpu), dev(d_np[::-1].copy(), gpu)
    idx = torch.arange(P, dtype=torch.int32, device=gpu)
    with torch.no_grad():
        eng.pack()
        a = eng.sdf_forward(addr(pt), 8, P, keep=True)
        a['n'] = dev((d_np * g.uniform(0.5, 2.0, (P, 1))).astype(np.float32), gpu)
        s = eng.shading_forward(a, pt, idx, P, torch.zeros(P, 4, device=gpu))
    nh = s['SD'][:, :3].contiguous()
    out = bake_light(net, nh, 1.0, pt[:, :3].contiguous(), _enc=True, _raw=True)
    assert torch.equal(out['enc'], s['OLin'][:P])
    assert torch.equal(out['raw'][:, :3], s['OLo'][:P, :3])


# ---- 2. float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_against_float64(gpu, sphere):
    """Measured on an MI355X, largest relative error over x absent / shared / per row, direct and probe mode: light 3.9e-5 /
    3.4e-5, direct 3.1e-5 / 2.7e-5, indirect 4.2e-5 / 2.9e-5 (sphere_direction off / on); occ 5.1e-7 / 5.7e-7 absolute."""
    from nu_nerf_amd.environment import bake_light
    net, arrays = stage1_net(gpu, sphere)
    exp_max = net.engine().exp_max
    n = 1024
    d_np, rho_np, x_np = EO.rows(n, 2026)
    d, rho, x = dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu)
    worst, worst_occ = {}, 0.0
    for name, pts_np, pts in (('absent', None, None), ('shared', x_np[5], x[5].clone()), ('per row', x_np, x)):
        for probe in (False, True):
            if probe and pts is None:
                continue
            want = EO.light64(arrays, d_np, rho_np, pts_np, sphere=sphere, exp_max=exp_max, probe=probe)
            out = bake_light(net, d, rho, pts, probe=probe)
            keys = ('light', 'direct', 'indirect') if probe else ('light',)
            for k in keys:
                live = want[k] > 1e-3                               # indirect = radiance x occ: relative where the occlusion is open
                e = np.abs(out[k].cpu().numpy().astype(np.float64) - want[k])
                worst[k] = max(worst.get(k, 0.0), float((e[live] / want[k][live]).max()))
                assert float(e[~live].max(initial=0.0)) <= OCC_ATOL      # closed occlusion: the radiance (below 1) times the occlusion's error
            if probe:
                worst_occ = max(worst_occ, float(np.abs(out['occ'].cpu().numpy().astype(np.float64) - want['occ']).max()))
                if name == 'per row':        # the inputs reach a clamp of the occlusion (one shared point can leave it in the interior)
                    sh = EO.shares(want, exp_max)
                    assert sh[5] >= 0.1 and max(sh[4], sh[6]) >= 0.1, sh
            else:
                assert set(out) == {'light'}
    print(f"light bake vs float64 (sphere_direction {sphere}, {n} rows): max relative err {({k: '%.3e' % v for k, v in worst.items()})}, "
          f"occ max abs err {worst_occ:.3e}")
    assert max(worst.values()) <= LIGHT_RTOL
    assert worst_occ <= OCC_ATOL


# ---- 3. both sides of every clamp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_both_sides_of_every_clamp(gpu, sphere):
    """Overrides (environment_oracle.clamp_overrides, computed from the float64 oracle alone and checked on the CPU by
    tests/test_environment_host.py): the bias of each exp head puts the median raw value of its channel at exp_max; the occlusion
    head's gain and bias put the quartiles of 0.5 raw + 0.5 at 0 and 1."""
    from nu_nerf_amd.environment import bake_light
    n = 512
    d_np, rho_np, x_np = EO.rows(n, 2027)
    base = stage1_arrays(sphere)
    over = EO.clamp_overrides(base, d_np, rho_np, x_np, sphere=sphere, exp_max=3.0)
    net, arrays = stage1_net(gpu, sphere, over)
    exp_max = net.engine().exp_max
    assert exp_max == 3.0
    want = EO.light64(arrays, d_np, rho_np, x_np, sphere=sphere, exp_max=exp_max, probe=True)
    sh = EO.shares(want, exp_max)
    print(f"clamp shares of the float64 oracle (sphere_direction {sphere}): direct above / below exp_max {sh[0]:.2f} / {sh[1]:.2f}, "
          f"indirect {sh[2]:.2f} / {sh[3]:.2f}, occ 0 / interior / 1 {sh[4]:.2f} / {sh[5]:.2f} / {sh[6]:.2f}")
    assert min(sh) >= 0.1, sh
    out = bake_light(net, dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu), probe=True, _raw=True)
    raw = out['raw'].cpu().numpy()
    # a row is taken as clamped where the float64 oracle AND the kernel's own raw head agree on the side (rows within rounding of a
    # threshold belong to neither set)
    up_d = (want['raw'][:, :3] > exp_max) & (raw[:, :3] > exp_max)
    up_i = (want['raw'][:, 3:6] > exp_max) & (raw[:, 3:6] > exp_max)
    occ0 = (want['occ_raw'] <= 0.0) & (0.5 * raw[:, 6] + 0.5 <= 0.0)
    occ1 = (want['occ_raw'] >= 1.0) & (0.5 * raw[:, 6] + 0.5 >= 1.0)
    assert up_d.any(1).mean() >= 0.1 and up_i.any(1).mean() >= 0.1 and occ0.mean() >= 0.1 and occ1.mean() >= 0.1
    direct, indirect, occ, light = (out[k].cpu().numpy() for k in ('direct', 'indirect', 'occ', 'light'))
    tops = np.unique(direct[up_d])
    assert tops.size == 1                                            # every clamped element is the one value exp(exp_max) ...
    top = torch.from_numpy(tops)
    assert ulp_distance(top, exp_of_raw(torch.full((1,), 1e9), exp_max)) <= EXP_ULPS      # ... of the device's expf
    top = tops[0]
    assert (occ[occ0] == 0.0).all() and (occ[occ1] == 1.0).all()
    assert (indirect[occ0] == 0.0).all() and np.array_equal(light[occ0], direct[occ0])
    assert np.array_equal(light[occ1], indirect[occ1])
    assert (indirect[occ1][up_i[occ1]] == np.float32(top)).all()
    inside = ~(occ0 | occ1)
    assert ((occ[inside] > 0.0) & (occ[inside] < 1.0)).mean() > 0.99
    # and the unclamped rows stay at the float64 values
    lo = (want['raw'][:, :3] < exp_max - 1e-3)
    assert rel_dev(out['direct'][torch.from_numpy(lo).to(gpu)], want['direct'][lo]) <= LIGHT_RTOL


# ---- 4. probe vs the eager composition -------------------------------------------------------------------------------------------
def check_probe(gpu, net, nets, eng, params, prefix, which):
    from nu_nerf_amd.environment import bake_light
    from eager_shading import raw_lights
    n = 97
    d_np, rho_np, x_np = EO.rows(n, 2028)
    d, rho, x = dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu)
    sphere, pf = eng.sphere_direction, eng.light_pos_freq
    out = bake_light(net, d, rho, x, which=which, probe=True, _raw=True)
    with torch.no_grad():
        eng.pack()
        ol, il, iw = raw_lights(nets, x, d, d, rho[:, None], sphere=sphere, pos_freq=pf)
    eager = torch.cat([ol[n:2 * n], il[:n], iw], 1)
    if not sphere:          # (with sphere_direction the eager sphere point is torch arithmetic, not the kernel's)
        assert torch.equal(out['raw'][:, :7], eager), float((out['raw'][:, :7] - eager).abs().max())
    assert torch.allclose(out['raw'][:, :7], eager, rtol=0, atol=2e-5)
    want = EO.light64(params, d_np, rho_np, x_np, sphere=sphere, exp_max=eng.exp_max, pos_freq=pf, probe=True, prefix=prefix)
    e_light, e_dir = rel_dev(out['light'], want['light']), rel_dev(out['direct'], want['direct'])
    e_occ = float(np.abs(out['occ'].cpu().numpy() - want['occ']).max())
    print(f"probe vs float64 ({prefix}, pos_freq {pf}, exp_max {eng.exp_max}): light {e_light:.3e} direct {e_dir:.3e} (relative), occ {e_occ:.3e}")
    assert max(e_light, e_dir) <= LIGHT_RTOL and e_occ <= OCC_ATOL
    return out


def test_probe_against_eager_raw_lights_pos_freq_6(gpu):
    from nu_nerf_amd.nets import Stage1Nets
    for sphere in (False, True):
        net, arrays = stage1_net(gpu, sphere)
        eng = net.engine()
        assert eng.light_pos_freq == 6
        check_probe(gpu, net, Stage1Nets(eng, net._named()), eng, arrays, 'color_network', None)
    net2, p2 = stage2_net(gpu)                                       # the zero-thickness inner network: also 6 frequencies
    n2 = net2.nets()[1]
    assert n2.eng.light_pos_freq == 6
    check_probe(gpu, net2, n2, n2.eng, p2, 'color_network_inner', 'inner')


def test_probe_against_eager_raw_lights_pos_freq_8(gpu):
    net3, p3 = stage2_net(gpu, thick=True)                            # AppShadingNetwork_SpecInner
    n3 = net3.nets()[1]
    assert n3.eng.light_pos_freq == 8
    check_probe(gpu, net3, n3, n3.eng, p3, 'color_network_inner', 'inner')


# ---- 5. row independence -----------------------------------------------------------------------------------------------------------
def test_row_independence_bits(gpu):
    from nu_nerf_amd.environment import bake_light
    net, _ = stage1_net(gpu, True)
    n = 97
    d_np, rho_np, x_np = EO.rows(n, 2029)
    d, rho, x = dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu)
    keys = ('light', 'direct', 'indirect', 'occ')
    cat = lambda o: torch.cat([o[k].reshape(o[k].shape[0], -1) for k in keys], 1)      # noqa: E731
    full = cat(bake_light(net, d, rho, x, probe=True))
    assert torch.equal(cat(bake_light(net, d, rho, x, probe=True)), full)              # two runs, same bits
    single = torch.cat([cat(bake_light(net, d[i:i + 1].contiguous(), rho[i:i + 1].contiguous(), x[i:i + 1].contiguous(), probe=True))
                        for i in range(n)], 0)
    assert torch.equal(single, full)
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).permutation(n)).to(gpu)
    moved = cat(bake_light(net, d[perm].contiguous(), rho[perm].contiguous(), x[perm].contiguous(), probe=True))
    assert torch.equal(moved, full[perm])
    # more tiles than workgroups: the grid-stride tail (257 tiles on at most 256 workgroups) repeats the 97 rows' bits
    reps = 85
    big = cat(bake_light(net, d.repeat(reps, 1), rho.repeat(reps), x.repeat(reps, 1), probe=True))
    assert big.shape[0] == 8245 and torch.equal(big, full.repeat(reps, 1))
    # direct mode gives the probe's direct light
    assert torch.equal(bake_light(net, d, rho, x)['light'], full[:, 3:6])


# ---- 6. the map convention ---------------------------------------------------------------------------------------------------------
def test_map_convention(gpu):
    from nu_nerf_amd.environment import bake_light, environment_map, latlong_dirs
    from nu_nerf_amd import relight
    net, _ = stage1_net(gpu, False)
    h, w = 8, 16
    m = environment_map(net, h, w)
    assert m.dtype == np.float32 and m.shape == (h, w, 3)
    dirs = latlong_dirs(h, w)
    assert np.array_equal(m, bake_light(net, dirs)['light'].cpu().numpy().reshape(h, w, 3))
    pyr = environment_map(net, h, w, [0.0, 0.5, 1.0])
    assert pyr.shape == (3, h, w, 3) and np.array_equal(pyr[0], m)
    assert np.array_equal(pyr[1], environment_map(net, h, w, 0.5)) and not np.array_equal(pyr[1], m)
    assert np.array_equal(net.predict_environment(h, w), m)
    back = relight.env_lookup(dev(relight.pack_env(m), gpu), dev(dirs, gpu)).cpu().numpy().reshape(h, w, 3)
    err = float((np.abs(back - m) / m).max())
    mirror = float((np.abs(m[:, ::-1] - m) / m).max())
    flip = float((np.abs(m[::-1] - m) / m).max())
    print(f"env_lookup(environment_map) at the texel centres: max relative err {err:.3e}; map vs its mirror {mirror:.3e}, vs its flip {flip:.3e}")
    assert err <= 1e-5
    assert mirror > 100 * 1e-5 and flip > 100 * 1e-5


# ---- 7. every renderer class and `which` -------------------------------------------------------------------------------------------
def test_every_renderer_class_and_which(gpu):
    from nu_nerf_amd.environment import bake_light
    from nu_nerf_amd.renderer_std import NeROShapeRenderer as StdRenderer
    n = 97
    d_np, rho_np, x_np = EO.rows(n, 2030)
    d, rho, x = dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu)
    keys = ('light', 'direct', 'indirect', 'occ')
    cat = lambda o: torch.cat([o[k].reshape(n, -1) for k in keys], 1)      # noqa: E731
    net1, _ = stage1_net(gpu, False, gain=False)
    ref = cat(bake_light(net1, d, rho, x, probe=True))
    with pytest.raises(ValueError):
        bake_light(net1, d, rho, x, which='inner')
    # stage 2, both thickness classes: 'outer' (the default here) is the stage-1 bake's bits; 'inner' is another network
    for thick in (False, True):
        net2, _ = stage2_net(gpu, thick=thick)
        assert torch.equal(cat(bake_light(net2, d, rho, x, probe=True)), ref)
        assert torch.equal(cat(bake_light(net2, d, rho, x, which='outer', probe=True)), ref)
        inner = cat(bake_light(net2, d, rho, x, which='inner', probe=True))
        assert not torch.equal(inner, ref) and bool(torch.isfinite(inner).all())
        m = net2.predict_environment(4, 8)
        assert np.array_equal(m, net1.predict_environment(4, 8)) and not np.array_equal(m, net2.predict_environment(4, 8, which='inner'))
    # the standard stage-1 renderer class holds the same networks
    std, _ = stage1_net(gpu, False, gain=False, cls=StdRenderer, cfg={'is_nerf': False})
    assert torch.equal(cat(bake_light(std, d, rho, x, probe=True)), ref)
    assert np.array_equal(std.predict_environment(4, 8, 0.25, (0.1, 0.2, -0.3), probe=True), net1.predict_environment(4, 8, 0.25, (0.1, 0.2, -0.3), probe=True))
    # a bf16-storage engine: the bake reads the fp32 tables, so it returns the fp32 engine's bits
    for md in ('bf16', 'bf16x6'):
        net16, _ = stage1_net(gpu, False, gain=False, cfg={'mlp_dtype': md})
        assert net16.engine().bf16 != 0
        assert torch.equal(cat(bake_light(net16, d, rho, x, probe=True)), ref), md


# ---- 8. the reference fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_reference_fixture(gpu, sphere):
    """Measured on an MI355X: light 2.6e-5 / 2.5e-5, direct 2.6e-5 / 3.0e-5 relative (sphere_direction off / on), indirect 1.1e-5 / 1.2e-5
    and occ 6.6e-7 absolute; the reference's own fp32 result is 2.3e-5 / 2.9e-5 from the float64 oracle on these rows."""
    from nu_nerf_amd.environment import bake_light
    g = golden('environment_stage1.npz')
    pre = f'sd{int(sphere)}__'
    over = {k[len(pre + 'override__'):]: v for k, v in g.items() if k.startswith(pre + 'override__')}
    net, arrays = stage1_net(gpu, sphere, over, gain=False)
    assert net.engine().exp_max == float(g['exp_max'])
    d_np, rho_np, x_np = EO.rows(int(g['n_rows']), int(g['row_seed']))
    out = bake_light(net, dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu), probe=True, _raw=True)
    v = g[pre + 'valid']                                             # the reference's IDE is NaN on the poles: those two rows are left out
    assert int((~v).sum()) == 2
    vt = torch.from_numpy(v).to(gpu)
    e = {k: rel_dev(out[k][vt], g[pre + k][v].astype(np.float64)) for k in ('light', 'direct')}
    ind = np.abs(out['indirect'].cpu().numpy().astype(np.float64) - g[pre + 'indirect'])[v]
    occ_raw = 0.5 * out['raw'][:, 6].cpu().numpy().astype(np.float64) + 0.5
    e_occ = float(np.abs(occ_raw - g[pre + 'occ_raw']).max())
    print(f"light bake vs reference fixture (sphere_direction {sphere}): relative err {({k: '%.3e' % x for k, x in e.items()})}, indirect abs "
          f"{ind.max():.3e}, occ abs {e_occ:.3e}; the fixture's own fp32 deviation from float64: light {float(g[pre + 'dev_light']):.2e}")
    assert max(e.values()) <= LIGHT_RTOL
    assert float(ind.max()) <= LIGHT_RTOL * float(g[pre + 'indirect'][v].max())
    assert e_occ <= OCC_ATOL
    assert np.array_equal(out['occ'].cpu().numpy(), np.clip(0.5 * out['raw'][:, 6].cpu().numpy() + np.float32(0.5), 0, 1))
    assert bool(torch.isfinite(out['light']).all())                  # the kernel's IDE is a polynomial: the poles are ordinary rows


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    import ctypes
    from nu_nerf_amd.environment import bake_light
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.engine import addr
    net, _ = stage1_net(gpu, True)
    eng = net.engine()
    n = 33
    d_np, rho_np, x_np = EO.rows(n, 2031)
    d, rho, x = dev(d_np, gpu), dev(rho_np, gpu), dev(x_np, gpu)
    ref = bake_light(net, d, rho, x, probe=True)
    # N = 0: empty tensors of the right shapes, no launch
    empty = bake_light(net, d[:0], rho[:0], x[:0], probe=True, _raw=True, _enc=True)
    assert [tuple(empty[k].shape) for k in ('light', 'direct', 'indirect', 'occ', 'raw', 'enc')] == [(0, 3), (0, 3), (0, 3), (0,), (0, 8), (0, 384)]
    assert tuple(bake_light(net, d[:0])['light'].shape) == (0, 3)
    # arrays are taken to the device; a scalar roughness is every row's; one point serves all rows
    assert torch.equal(bake_light(net, d_np, rho_np, x_np, probe=True)['light'], ref['light'])
    assert torch.equal(bake_light(net, d, 0.5, x[3].clone())['light'], bake_light(net, d, torch.full((n,), 0.5, device=gpu), x[3].expand(n, 3).contiguous())['light'])
    # wrong dtype, shape, device or contiguity raises before the call
    wide = torch.zeros(n, 8, device=gpu)
    wide[:, :3] = d
    for bad in (wide[:, :3], d.double(), d.half(), d[:, :2].contiguous(), d.reshape(-1), d.t().contiguous().t(), d.cpu()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            bake_light(net, bad, rho, x)
    for bad in (rho.double(), rho[:-1].contiguous(), rho.repeat_interleave(2)[::2], rho.cpu(), rho[:, None].contiguous()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            bake_light(net, d, bad, x)
    for bad in (x.double(), x[:-1].contiguous(), x[:, :2].contiguous(), wide[:, 3:6], x.cpu(), x[0, :2].contiguous()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            bake_light(net, d, rho, bad)
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        bake_light(net, d, rho, None, probe=True)                    # probe needs the point
    with pytest.raises(ValueError):
        bake_light(net, d, rho, x, which='middle')
    # the C entry: every NU_ERR_ARG case
    eng.pack()
    lib, sn, S = eng.lib, ctypes.byref(eng._shade_net), eng.stream()
    light = torch.full((n, 3), -7.0, device=gpu)
    call = lambda net_p, dirs, kinv, xp, xs, pf, nn, probe: lib.nu_light_bake_fwd(net_p, dirs, kinv, xp, xs, pf, nn, probe, addr(light), 0, 0, 0, 0, 0, S)      # noqa: E731
    for args in ((None, addr(d), addr(rho), addr(x), 3, 6, n, 0),          # no network
                 (sn, 0, addr(rho), addr(x), 3, 6, n, 0),                  # no directions
                 (sn, addr(d), 0, addr(x), 3, 6, n, 0),                    # no roughness
                 (sn, addr(d), addr(rho), addr(x), 3, 6, -1, 0),           # negative N
                 (sn, addr(d), addr(rho), 0, 0, 6, n, 1),                  # probe without x
                 (sn, addr(d), addr(rho), addr(x), 2, 6, n, 0),            # points closer than 3 floats apart
                 (sn, addr(d), addr(rho), addr(x), 3, 9, n, 1),            # pos_enc wider than the input tile
                 (sn, addr(d), addr(rho), addr(x), 3, 8, n, 1)):           # pos_freq that is not the network's
        with pytest.raises(NuNerfLibraryError, match=r"nu_light_bake_fwd failed with code -1"):
            call(*args)
    assert bool((light == -7.0).all())                                     # nothing was launched
    assert call(sn, addr(d), addr(rho), addr(x), 3, 6, 0, 1) == 0          # N = 0 returns at once
    assert bool((light == -7.0).all())
    assert call(sn, addr(d), addr(rho), addr(x), 3, 6, n, 1) == 0          # every other output may be NULL
    torch.cuda.synchronize()
    assert torch.equal(light, ref['light'])


# ---- 10. the command ---------------------------------------------------------------------------------------------------------------
def test_command_writes_a_map_relight_accepts(gpu, tmp_path, monkeypatch, capsys):
    import json
    import yaml
    from nu_nerf_amd import extract_environment, relight
    from nu_nerf_amd.mesh import write_ply
    from nu_nerf_amd.lbvh import icosphere
    net, _ = stage1_net(gpu, False)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}},
               'data/model/tiny/model.pth')
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = extract_environment.main(['--cfg', 'tiny.yaml', '--height', '8', '--width', '16', '--roughness', '0', '0.5', '1'])
    assert out == os.path.join('data', 'environment', 'tiny-1234')
    assert sorted(os.listdir(out)) == ['env.hdr', 'env.npy', 'env.png', 'env_pyramid.npy', 'roughness.npy']
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    env, pyr = np.load(os.path.join(out, 'env.npy')), np.load(os.path.join(out, 'env_pyramid.npy'))
    assert env.dtype == np.float32 and env.shape == (8, 16, 3) and pyr.shape == (3, 8, 16, 3) and np.array_equal(pyr[0], env)
    assert np.array_equal(env, net.predict_environment(8, 16)) and np.array_equal(pyr, net.predict_environment(8, 16, [0.0, 0.5, 1.0]))
    assert np.array_equal(np.load(os.path.join(out, 'roughness.npy')), np.asarray([0.0, 0.5, 1.0], np.float32))
    assert line['shape'] == [3, 8, 16, 3] and line['paths']['hdr'] == os.path.join(out, 'env.hdr')
    assert abs(line['mean'] - float(env.mean())) < 1e-6 and line['min'] == float(env.min()) and line['max'] == float(env.max())
    back = relight.read_hdr(os.path.join(out, 'env.hdr'))
    assert back.shape == env.shape and (np.abs(back - env) <= 2.0 ** -8 * env.max(-1, keepdims=True)).all()
    from nu_nerf_amd.mask_render import _pillow
    assert _pillow().open(os.path.join(out, 'env.png')).size == (16, 8)
    # relight takes the file as it is
    V, F = icosphere(1, 0.5)
    V = np.asarray(V, np.float32)
    write_ply('ball.ply', V, F)
    os.makedirs('mat')
    np.save('mat/metallic.npy', np.full((len(V), 1), 0.5, np.float32))
    np.save('mat/roughness.npy', np.full((len(V), 1), 0.4, np.float32))
    np.save('mat/albedo.npy', np.full((len(V), 3), 0.7, np.float32))
    frames = relight.main(['--mesh', 'ball.ply', '--material', 'mat', '--hdr', os.path.join(out, 'env.hdr'), '--name', 'tiny', '--num', '1',
                           '--width', '16', '--height', '16', '--samples', '4', '--cam_dist', '2'])
    img = np.asarray(_pillow().open(relight.frame_path(frames, 0)))
    assert img.shape == (16, 16, 4) and img[..., 3].max() == 255 and img[..., :3][img[..., 3] == 255].max() > 0
