"""Curvature from the SDF's Hessian on the GPU (csrc/sdf_jet.hip, nu_nerf_amd/curvature.py): the value row's bits, row independence, a
float64 oracle (tests/curvature_oracle.py: torch autograd over oracle.stage1_oracle.sdf_forward), an analytic network with a closed
form, the degenerate gradient, the C entry's arguments, Gauss-Bonnet on a device-extracted mesh, and the opt-in consumers.

Bounds (test 3, also used by tests 5 and 7).  Each is four times the largest error measured on an MI355X against the float64 oracle
(never against the kernel itself; run to run there is no spread, the margin is for another compiler's contraction choices, DESIGN.md
sections 19 and 26), over 4096 points at radius 0.2 .. 0.95 on the parity network, the init network and both SDFs of the stage-2
model (inner, and outer = the parity network at other points); sdf, gradient and Hessian absolute, the curvatures relative to max(1, |reference|).  Measured / bound / cap:
    sdf        1.036e-6 / 4.14e-6 / 1e-5
    gradient   7.62e-7  / 3.05e-6 / 1e-5
    hessian    1.094e-5 / 4.38e-5 / 1e-4      (entries up to 10.1)
    mean       8.43e-6  / 3.37e-5 / 1e-4
    gaussian   4.74e-5  / 1.90e-4 / 1e-3      (|K| up to 263)
No rows are left out; the smallest |g| of the oracle on these points is 0.167 (stage-2 inner), 0.265 (parity), 0.272 (init).
Test 4: the reverse sweep's gradient (sdf_network.gradient) measured 9.73e-7 against float64 on the parity network's points, the jet's
6.30e-7 (the two differ by 1.01e-6);
the jet is held to twice the reverse sweep's measured error."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import curvature_oracle as CO
from helpers import golden

pytestmark = pytest.mark.gpu

T = 6                                                # points per tile of sdf_jet_fwd_kernel
BOUND = {'sdf': 4.14e-6, 'gradient': 3.05e-6, 'hessian': 4.38e-5, 'mean': 3.37e-5, 'gaussian': 1.90e-4}
CAP = {'sdf': 1e-5, 'gradient': 1e-5, 'hessian': 1e-4, 'mean': 1e-4, 'gaussian': 1e-3}
assert all(BOUND[k] <= CAP[k] for k in CAP)
REVERSE_SWEEP_MEASURED = 9.73e-7                      # max abs error of sdf_network.gradient against float64 (test 4)
G_MIN = 0.15                                         # below the smallest |g| of the float64 oracle on the test points (0.167)
KEYS = ('sdf', 'gradient', 'hessian', 'mean', 'gaussian', 'normal')


# ---- the networks of tests/test_materials_gpu.py ---------------------------------------------------------------------------------
def stage1_arrays(init_only=False):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = init_stage1_params(6033)
    return arrays if init_only else randomize_for_parity(arrays, seed=1)


def stage1_net(gpu, overrides=None, init_only=False):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    arrays = stage1_arrays(init_only)
    arrays.update(overrides or {})
    net = NeROShapeRenderer({'name': 'golden'}, training=False)
    net.load_param_dict(arrays)
    return net.to(gpu), arrays


def stage2_net(gpu):
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, randomize_for_parity
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.stage2 import Stage2Renderer
    s1 = randomize_for_parity(init_stage1_params(6033), seed=1)
    s1cfg = {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000}
    cfg = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'shader_config': {'sphere_direction': False, 'human_light': False},
           'stage1_cfg': s1cfg, 'stage1_mesh_arrays': icosphere(3, 0.5)}
    net = Stage2Renderer(cfg, training=False)
    p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
    sd = net.state_dict()
    for k in [k for k in p2 if k.startswith('stage1_network.')]:      # the aliases of the same tensors, where the model has them
        if 'color_network.' + k in sd:
            p2['color_network.' + k] = p2[k]
    net.load_param_dict(p2)
    return net.to(gpu), p2


def shell_points(n, seed, gpu, lo=0.2, hi=0.95):
    g = np.random.Generator(np.random.PCG64(seed))
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((d * g.uniform(lo, hi, (n, 1))).astype(np.float32)).to(gpu)


def bake(net, x, which=None):
    from nu_nerf_amd.curvature import bake_curvature
    return bake_curvature(net, x, which=which, hessian=True)


def flat(out):
    """Every output of a point side by side [P,15]: equal rows = equal bits of everything."""
    return torch.cat([out['sdf'][:, None], out['gradient'], out['hessian'], out['mean'][:, None], out['gaussian'], out['normal']], 1)


def errors(out, ref):
    """max errors against the float64 dict `ref`: sdf, gradient, hessian absolute; mean, gaussian relative to max(1, |ref|).  All rows."""
    e = {}
    for k in ('sdf', 'gradient', 'hessian'):
        e[k] = float(np.abs(out[k].cpu().numpy().astype(np.float64) - ref[k]).max())
    for k in ('mean', 'gaussian'):
        got = out[k].cpu().numpy().astype(np.float64).reshape(-1)
        e[k] = float((np.abs(got - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
    return e


@pytest.fixture(scope='module')
def parity(gpu):
    """(net, arrays, x [4096,3], the kernel's outputs, the float64 oracle) of the parity network: computed once, never modified."""
    net, arrays = stage1_net(gpu)
    x = shell_points(4096, 64, gpu)
    return net, arrays, x, bake(net, x), CO.sdf_jet64(arrays, x.cpu().numpy(), device=gpu)


# ---- 1. the value row carries the bits of nu_sdf_fused_fwd -------------------------------------------------------------------------
def test_value_bits(gpu, parity):
    from nu_nerf_amd.engine import addr
    net, _, x, full, _ = parity
    eng = net.engine()
    eng.pack()
    for n in (1, T - 1, T, T + 1, 2 * T + 1, 4096):
        xs = x[:n].contiguous()
        out = bake(net, xs)
        fused = eng.sdf_forward(addr(xs), 3, n, keep=False, want_feat=False)['sdf']       # nu_sdf_fused_fwd
        assert torch.equal(out['sdf'], fused), n
        assert torch.equal(flat(out), flat(full)[:n]), n               # and a prefix of the batch is the batch's prefix


# ---- 2. row independence -----------------------------------------------------------------------------------------------------------
def test_row_independence_bits(gpu, parity):
    net, _, x, full, _ = parity
    ref = flat(full)
    assert torch.equal(flat(bake(net, x)), ref)                         # two runs, equal bits
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(4096)).to(gpu)
    assert torch.equal(flat(bake(net, x[perm].contiguous())), ref[perm])
    rolled = torch.roll(torch.arange(4096, device=gpu), 1)             # every point in the next slot of its tile (or the next tile)
    assert torch.equal(flat(bake(net, x[rolled].contiguous())), ref[rolled])
    for i in (0, 1, 5, 6, 2047, 4095):                                  # a point alone against the same point inside 4096
        assert torch.equal(flat(bake(net, x[i:i + 1].contiguous()))[0], ref[i]), i
    for pos in range(T + 1):                                            # every slot of a tile, different neighbours
        batch = shell_points(T + 1, 100 + pos, gpu)
        batch[pos] = x[77]
        assert torch.equal(flat(bake(net, batch))[pos], ref[77]), pos


# ---- 3. float64 ----------------------------------------------------------------------------------------------------------------------
def check_float64(name, out, ref):
    e = errors(out, ref)
    gn = np.linalg.norm(ref['gradient'], axis=1)
    print(f"sdf jet vs float64 ({name}): " + "  ".join(f"{k} {v:.3e}" for k, v in e.items())
          + f"   |g| {gn.min():.3f} .. {gn.max():.3f}  max|H| {np.abs(ref['hessian']).max():.2f}  max|K| {np.abs(ref['gaussian']).max():.1f}")
    assert gn.min() >= G_MIN
    n_err = float(np.abs(out['normal'].cpu().numpy().astype(np.float64) - ref['normal']).max())
    for k in e:
        assert e[k] <= BOUND[k], (name, k, e[k])
    assert n_err <= 2 * BOUND['gradient'] / G_MIN, (name, n_err)        # n = g / |g|: |dn| <= 2 |dg| / |g|
    return e


def test_float64_parity_network(gpu, parity):
    _, _, _, out, ref = parity
    check_float64('parity', out, ref)


def test_float64_init_network(gpu):
    net, arrays = stage1_net(gpu, init_only=True)
    x = shell_points(4096, 65, gpu)
    check_float64('init', bake(net, x), CO.sdf_jet64(arrays, x.cpu().numpy(), device=gpu))


def test_float64_stage2_inner(gpu):
    net, p2 = stage2_net(gpu)
    x = shell_points(4096, 66, gpu)
    out = bake(net, x)                                                  # a stage-2 renderer's default is its inner SDF
    assert torch.equal(flat(out), flat(bake(net, x, which='inner')))
    check_float64('stage-2 inner', out, CO.sdf_jet64(p2, x.cpu().numpy(), prefix='sdf_network_inner', device=gpu))
    outer = bake(net, x, which='outer')
    check_float64('stage-2 outer', outer, CO.sdf_jet64(p2, x.cpu().numpy(), prefix='stage1_network.sdf_network', device=gpu))
    assert not torch.equal(outer['sdf'], out['sdf'])
    pc = net.predict_curvature((x[:50].cpu().numpy(), np.zeros((0, 3), np.int32)), which='outer')
    assert set(pc) == {'gaussian', 'mean', 'normal'} and pc['gaussian'].shape == (50, 1) and pc['gaussian'].dtype == np.float32
    assert np.array_equal(pc['gaussian'], outer['gaussian'][:50].cpu().numpy()) and np.array_equal(pc['mean'], outer['mean'][:50].cpu().numpy())


# ---- 4. the gradient against the existing path ----------------------------------------------------------------------------------------
def test_gradient_against_the_reverse_sweep(gpu, parity):
    """Not held to each other: both to float64.  The jet's error is at most twice the reverse sweep's own measured error."""
    net, _, x, out, ref = parity
    rev = net.sdf_network.gradient(x).detach()
    e_rev = float(np.abs(rev.cpu().numpy().astype(np.float64) - ref['gradient']).max())
    e_jet = float(np.abs(out['gradient'].cpu().numpy().astype(np.float64) - ref['gradient']).max())
    print(f"gradient vs float64: reverse sweep {e_rev:.3e}  jet {e_jet:.3e}  (jet vs reverse sweep {float((rev - out['gradient']).abs().max()):.3e})")
    assert e_rev <= 4 * REVERSE_SWEEP_MEASURED <= CAP['gradient']
    assert e_jet <= 2 * REVERSE_SWEEP_MEASURED


# ---- 5. the analytic network ---------------------------------------------------------------------------------------------------------
def test_analytic_network(gpu):
    """Pass-through hidden layers, head = a sum of embedding columns through the main path and through the skip (every frequency up to
    k = 5 on both): value, gradient, Hessian and curvatures against the closed form, with the bounds of test 3."""
    A, B = CO.analytic_coefficients()
    template = stage1_arrays()
    net, _ = stage1_net(gpu, CO.analytic_overrides(A, B, template))
    x = shell_points(1000, 67, gpu)
    out = bake(net, x)
    f, g, H6 = CO.analytic_jet(A, B, x.cpu().numpy())
    mean, gauss, normal = CO.curvatures(g, H6)
    ref = {'sdf': f, 'gradient': g, 'hessian': H6, 'mean': mean, 'gaussian': gauss, 'normal': normal}
    assert np.abs(H6[:, :3]).max() > 2.0 and np.linalg.norm(g, axis=1).min() >= G_MIN
    assert not out['hessian'][:, 3:].any()                              # a separable field: the mixed derivatives are exact zeros
    check_float64('analytic', out, ref)


# ---- 6. degenerate gradient, P = 0, nullable outputs, argument errors -----------------------------------------------------------------
def test_degenerate_and_edges(gpu, parity):
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.curvature import bake_curvature
    from nu_nerf_amd.engine import addr
    A0, B0 = CO.analytic_coefficients(only_cos0=True)
    net0, _ = stage1_net(gpu, CO.analytic_overrides(A0, B0, stage1_arrays()))
    x0 = torch.zeros(T + 1, 3, device=gpu)
    x0[1:] = shell_points(T, 5, gpu)
    out = bake(net0, x0)
    assert all(bool(torch.isfinite(out[k]).all()) for k in KEYS)
    assert not out['gradient'][0].any() and float(out['mean'][0]) == 0 and float(out['gaussian'][0]) == 0 and not out['normal'][0].any()
    C = A0.astype(np.float64) + B0.astype(np.float64)
    want_h = [-C[CO.embed_col(0, c, True)] for c in range(3)]
    assert np.abs(out['hessian'][0, :3].cpu().numpy() - want_h).max() <= BOUND['hessian'] and not out['hessian'][0, 3:].any()
    assert abs(float(out['sdf'][0]) - float(C.sum())) <= BOUND['sdf']
    assert out['gradient'][1:].abs().sum(1).min() > 0 and out['normal'][1:].norm(dim=1).sub(1).abs().max() < 1e-6

    net, _, x, full, _ = parity
    empty = bake(net, x[:0])
    assert {k: tuple(v.shape) for k, v in empty.items()} == {'sdf': (0,), 'normal': (0, 3), 'gradient': (0, 3), 'mean': (0,),
                                                             'gaussian': (0, 1), 'hessian': (0, 6)}
    assert 'hessian' not in bake_curvature(net, x[:7]) and tuple(bake_curvature(net, x[:7])['gaussian'].shape) == (7, 1)
    eng = net.engine()
    n = 1000
    e = lambda *s: torch.full(s, -7.0, device=gpu)                      # noqa: E731
    only_k, only_h = e(n), e(n, 6)
    eng.sdf_jet(addr(x), 3, n, gauss=only_k)                            # nullable outputs: any subset, same bits
    eng.sdf_jet(addr(x), 3, n, hess=only_h)
    assert torch.equal(only_k, full['gaussian'][:n, 0]) and torch.equal(only_h, full['hessian'][:n])
    eng.sdf_jet(addr(x), 3, n)                                          # nothing asked for: still a valid call
    wide = torch.full((n, 8), float('nan'), device=gpu)                 # x_ld = 8: the other columns are never read
    wide[:, :3] = x[:n]
    assert torch.equal(flat(bake(net, wide)), flat(full)[:n])
    # the C entry's own argument checks
    lib, net_ref, S = eng.lib, ctypes.byref(eng._sdf_net), eng.stream()
    eng.sdf_jet(addr(x), 3, 0, gauss=only_k)                            # P == 0: nothing launched, nothing written
    assert torch.equal(only_k, full['gaussian'][:n, 0])
    for args in ((None, addr(x), 3, n), (net_ref, None, 3, n), (net_ref, addr(x), 3, -1), (net_ref, addr(x), 2, n), (None, None, 3, 0)):
        with pytest.raises(NuNerfLibraryError, match=r"nu_sdf_jet_fwd failed with code -1"):
            lib.nu_sdf_jet_fwd(*args, addr(only_k), None, None, None, None, None, S)
    torch.cuda.synchronize()
    assert torch.equal(only_k, full['gaussian'][:n, 0])
    for bad in (x.double(), x[:, :2].contiguous(), x.reshape(-1), x.t().contiguous().t(), x.cpu()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            bake(net, bad)
    with pytest.raises(ValueError):
        bake(net, x, which='inner')


# ---- 7. Gauss-Bonnet on the device ------------------------------------------------------------------------------------------------------
def test_gauss_bonnet_on_the_device(gpu):
    from nu_nerf_amd.curvature import curvature_stats, euler_characteristic, gauss_bonnet_ratio, vertex_areas
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.lbvh import vertex_normals_and_curvature
    from nu_nerf_amd.mesh import extract_geometry
    net, arrays = stage1_net(gpu, init_only=True)
    eng = net.engine()
    eng.pack()

    def query(p):
        p = p.contiguous()
        return eng.sdf_forward(addr(p), 3, p.shape[0], keep=False, want_feat=False)['sdf']
    V, F = extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), 48, 0.0, query)
    assert euler_characteristic(len(V), F) == 2
    K = bake(net, torch.from_numpy(V).to(gpu))['gaussian'].cpu().numpy().reshape(-1)
    ratio = gauss_bonnet_ratio(K, V, F)
    ref = CO.sdf_jet64(arrays, V, device=gpu)['gaussian']
    ratio64 = gauss_bonnet_ratio(ref, V, F)
    defect = vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F.astype(np.int64)))[1].numpy()
    print(f"Gauss-Bonnet on the device, init network 48^3: V {len(V)}  ratio {ratio:.6f}  float64 on the same vertices {ratio64:.6f}")
    print(f"  K from the SDF: {curvature_stats(K)}\n  K from the angle defect (clipped to +-10): {curvature_stats(defect)}")
    assert abs(ratio - 1.0) <= 0.01
    # the sums differ by at most sum_v |dK_v| A_v <= bound * sum_v max(1, |K_v|) A_v
    A = vertex_areas(V, F)
    assert abs(ratio - ratio64) <= BOUND['gaussian'] * float(np.sum(np.maximum(1.0, np.abs(ref)) * A)) / (4.0 * math.pi)
    assert (np.abs(K - ref) <= BOUND['gaussian'] * np.maximum(1.0, np.abs(ref))).all()


# ---- 8. consumers ---------------------------------------------------------------------------------------------------------------------
def test_scene_takes_a_curvature(gpu):
    from nu_nerf_amd.lbvh import Scene, icosphere, vertex_normals_and_curvature
    V, F = icosphere(2, 0.5)
    Vt, Ft = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    plain = Scene(Vt, Ft)
    normals, curv = vertex_normals_and_curvature(Vt.cpu(), Ft.cpu())    # what Scene computed before it took a curvature
    assert torch.equal(plain.gaussian_curvatures.cpu(), curv) and torch.equal(plain.normals.cpu(), normals)
    assert torch.equal(Scene(Vt, Ft, curvature=None).gaussian_curvatures, plain.gaussian_curvatures)
    c = torch.linspace(-25.0, 140.0, len(V), device=gpu)
    for given in (c, c[:, None], c.cpu().numpy()):
        s = Scene(Vt, Ft, curvature=given)
        assert s.gaussian_curvatures.is_cuda and tuple(s.gaussian_curvatures.shape) == (len(V), 1)
        assert torch.equal(s.gaussian_curvatures[:, 0], c.clamp(-10.0, 10.0))
        assert torch.equal(s.normals, plain.normals)
    bad = c.clone()
    bad[3] = float('nan')
    for given in (bad, c[:-1], torch.stack([c, c], 1)):
        with pytest.raises(ValueError, match='curvature'):
            Scene(Vt, Ft, curvature=given)


def build_thick(gpu, g, shell_curvature=None):
    """The non-zero-thickness stage-2 model of tests/test_stage2_thick_gpu.py (its reference fixture's parameters and rays)."""
    from nu_nerf_amd.stage2_thick import Stage2Renderer
    from nu_nerf_amd.params import init_stage1_params, load_fg_lut, params_from_manifest, randomize_for_parity
    from nu_nerf_amd.lbvh import icosphere
    losses = ('eikonal', 'std', 'nerf_render')
    s1 = randomize_for_parity(init_stage1_params(6033, sphere_direction=True), seed=1)
    shader = {'sphere_direction': True, 'human_light': False, 'light_exp_max': 5.0}
    s1cfg = {'name': 's1', 'network': 'shape', 'get_mask': False, 'database_name': 'real/x/raw_1024', 'is_nerf': False,
             'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000, 'zero_thickness': False, 'shader_config': shader}
    cfg = {'name': 'golden_s2t', 'network': 'stage2', 'get_mask': False, 'database_name': 'real/x/raw_1024', 'is_nerf': False,
           'shader_config': shader, 'loss': list(losses), 'eikonal_weight': 0.02, 'freeze_inv_s_step': 5000, 'occ_loss_step': 20000,
           'stage1_cfg': s1cfg, 'stage1_mesh_arrays': icosphere(3, 0.5)}
    if shell_curvature is not None:
        cfg['shell_curvature'] = shell_curvature
    net = Stage2Renderer(cfg, training=False)
    manifest = [(str(n), tuple(int(x) for x in str(s).split(',') if x)) for n, s in zip(g['manifest_names'], g['manifest_shapes'])]
    p2 = params_from_manifest(manifest, int(g['manifest_seed']))
    inner = randomize_for_parity(init_stage1_params(7044, sphere_direction=True), seed=3)
    for k, v in inner.items():
        if k.startswith('sdf_network.'):
            p2['sdf_network_inner.' + k[len('sdf_network.'):]] = v
    p2['deviation_network_inner.variance'] = inner['deviation_network.variance']
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
        p2['color_network.stage1_network.' + k] = v
        if k.startswith('infinity_far_bkgr.'):
            p2[k] = v
    p2 = {k: v for k, v in p2.items() if not k.endswith('FG_LUT')}
    net.load_param_dict(p2)
    with torch.no_grad():
        lut = torch.from_numpy(load_fg_lut())
        net.color_network_inner.FG_LUT.copy_(lut.reshape(net.color_network_inner.FG_LUT.shape))
        net.stage1_network.color_network.FG_LUT.copy_(lut.reshape(net.stage1_network.color_network.FG_LUT.shape))
    return net.to(gpu), cfg


def thick_step(net, cfg, g, gpu):
    from nu_nerf_amd.loss import name2loss, total_loss
    step = int(g['step'])
    batch = {k: torch.from_numpy(g[k]).to(gpu) for k in ('rays_o', 'rays_d', 'rgbs')}
    net.zero_grad(set_to_none=True)
    out = net.train_step_rays(batch, step)
    total, _ = total_loss(out, [name2loss[n](cfg) for n in cfg['loss']], step)
    total.backward()
    return out, total


def test_thick_stage2_shell_curvature(gpu):
    from nu_nerf_amd.curvature import bake_curvature
    from nu_nerf_amd.stage2_thick import Stage2Renderer
    g = golden('stage2_thick_step6000_r24.npz')
    net_d, cfg_d = build_thick(gpu, g)
    net_m, cfg_m = build_thick(gpu, g, 'mesh')
    assert net_d.cfg['shell_curvature'] == 'mesh'
    out_d, total_d = thick_step(net_d, cfg_d, g, gpu)
    out_m, total_m = thick_step(net_m, cfg_m, g, gpu)
    assert torch.equal(net_m.scene.gaussian_curvatures, net_d.scene.gaussian_curvatures)
    assert torch.equal(out_m['ray_rgb'], out_d['ray_rgb']) and torch.equal(total_m, total_d)
    assert torch.equal(out_m['tir_mask'], out_d['tir_mask'])
    for a, b in zip(out_m['_paths'], out_d['_paths']):
        assert torch.equal(a, b)
    # 'sdf': the stage-1 SDF's curvature at the mesh vertices, clipped, in the scene; one step runs
    net_s, cfg_s = build_thick(gpu, g, 'sdf')
    out_s, total_s = thick_step(net_s, cfg_s, g, gpu)
    V = torch.from_numpy(np.ascontiguousarray(net_s._mesh[0], np.float32)).to(gpu)
    want = bake_curvature(net_s, V, which='outer')['gaussian'].clamp(-10.0, 10.0)
    assert torch.equal(net_s.scene.gaussian_curvatures, want) and tuple(want.shape) == (len(V), 1)
    assert not torch.equal(net_s.scene.gaussian_curvatures, net_d.scene.gaussian_curvatures)
    assert torch.equal(net_s.scene.normals, net_d.scene.normals)
    assert bool(torch.isfinite(total_s)) and bool(torch.isfinite(out_s['ray_rgb']).all())
    assert tuple(out_s['tir_mask'].shape) == tuple(out_d['tir_mask'].shape) and out_s['tir_mask'].dtype == out_d['tir_mask'].dtype
    assert len(out_s['_paths']) == 3 and all(bool(torch.isfinite(p).all()) for p in out_s['_paths'])
    assert [p.shape for p in out_s['_paths']][0] == out_d['_paths'][0].shape
    assert all(bool(torch.isfinite(d).all()) for d in out_s['_directions'])
    print(f"thick stage 2, one step: loss mesh curvature {float(total_d.detach()):.6f}  SDF curvature {float(total_s.detach()):.6f}")
    with pytest.raises(ValueError, match='shell_curvature'):
        Stage2Renderer({**cfg_d, 'shell_curvature': 'pymesh'}, training=False)


def test_command_writes_its_three_files(gpu, tmp_path, monkeypatch, capsys):
    import json
    import yaml
    from nu_nerf_amd import extract_curvature
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mesh import write_ply
    net, _ = stage1_net(gpu)
    V, F = icosphere(2, 0.5)
    V = np.asarray(V, np.float32)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    os.makedirs('data/meshes')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}},
               'data/model/tiny/model.pth')
    write_ply('data/meshes/tiny-1234.ply', V, F)
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = extract_curvature.main(['--cfg', 'tiny.yaml'])
    assert out == os.path.join('data', 'materials', 'tiny-1234')
    want = net.predict_curvature((V, F))
    assert sorted(os.listdir(out)) == ['curvature.npy', 'mean_curvature.npy', 'sdf_normal.npy']
    for fn, key, shape in (('curvature.npy', 'gaussian', (len(V), 1)), ('mean_curvature.npy', 'mean', (len(V),)),
                           ('sdf_normal.npy', 'normal', (len(V), 3))):
        a = np.load(os.path.join(out, fn))
        assert a.dtype == np.float32 and a.shape == shape and np.array_equal(a, want[key])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep['V'] == len(V) and rep['step'] == 1234 and set(rep['sdf']) == set(rep['angle_defect']) == {'p5', 'p50', 'p95', 'outside_pm10'}
    assert rep['gauss_bonnet'] is not None and np.isfinite(rep['gauss_bonnet'])
    assert abs(rep['angle_defect']['p50'] - 4.0) < 0.4                  # the icosphere of radius 0.5: 1 / r^2
