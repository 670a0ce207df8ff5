"""Material baking on the GPU (csrc/bake.hip, nu_nerf_amd/materials.py): parity with the reference fixture and a float64 evaluation,
bit-identity with the layered path, row independence, the C entry's argument handling, the command.

Bounds.  PARITY_ATOL (tests 1 and 5) is four times the largest absolute error measured on an MI355X against the reference fixture and
against the float64 evaluation (never against the kernel itself; run to run there is no spread, the margin is for another compiler's
contraction choices), and may not exceed 1e-5: measured 4.5e-7 (stage-1 fixture), 4.2e-7 (stage-2 inner fixture) and 5.8e-7 (float64, 4096
points; the head gain of 30 the fixtures carry is in all three), so 4 x 5.8e-7 = 2.3e-6; see DESIGN.md section 19.
The layered path (test 4): sdf, feature columns and the raw heads are the same bits -- same MFMA k order, same epilogue functions, same
head reduction (the three foreign blocks of the block-diagonal 1024-wide head row add exact zeros).  The sigmoid is evaluated by
another routine than torch's, so the outputs are held to SIGMOID_ULPS = 2 units in the last place of the result: each of the two is a
correctly rounded division of a 1-ulp exp, and d sigmoid / d exp error is below 1/4."""
import os

import numpy as np
import pytest
import torch

from helpers import golden

pytestmark = pytest.mark.gpu

PARITY_ATOL = 2.3e-6
assert PARITY_ATOL <= 1e-5
SIGMOID_ULPS = 2
KEYS = ('metallic', 'roughness', 'albedo')


def stage1_net(gpu, overrides=None):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = randomize_for_parity(init_stage1_params(6033), seed=1)
    arrays.update(overrides or {})
    net = NeROShapeRenderer({'name': 'golden'}, training=False)
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


def overrides_of(g):
    return {k[len('override__'):]: v for k, v in g.items() if k.startswith('override__')}


def layered(eng, named, x):
    """(YX [P,288] = sdf | feature | x, raw heads [P,6]) of the gradient-carrying layered path under no_grad."""
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.engine import addr
    with torch.no_grad():
        eng.pack()
        YX = eng.sdf_forward(addr(x), x.shape[1], x.shape[0], keep=False, want_feat=True)['YX']
        raw = Stage1Nets(eng, named).materials(YX[:, 1:257].contiguous(), x[:, :3].contiguous())
    return YX, raw


def five(out):
    return torch.cat([out['metallic'], out['roughness'], out['albedo']], 1)


def ball(n, seed, gpu, radius=0.95):
    g = np.random.Generator(np.random.PCG64(seed))
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((d * g.random((n, 1)) ** (1 / 3) * radius).astype(np.float32)).to(gpu)


def ulp_distance(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()      # positive floats: monotone
    return int((ia - ib).abs().max())


# ---- 1. reference parity ------------------------------------------------------------------------------------------------------
def check_against_fixture(net, g, which, gpu):
    from nu_nerf_amd.materials import bake_materials
    nv = int(g['n_mesh_vertices'])
    pm = net.predict_materials((g['points'][:nv], g['faces'])) if which is None else net.predict_materials((g['points'][:nv], g['faces']), which)
    assert set(pm) == set(KEYS)
    worst = 0.0
    for k in KEYS:
        assert isinstance(pm[k], np.ndarray) and pm[k].dtype == np.float32 and pm[k].shape == g[k][:nv].shape
        worst = max(worst, float(np.abs(pm[k].astype(np.float64) - g[k][:nv]).max()))
    out = bake_materials(net, torch.from_numpy(g['points']).to(gpu), which=which, sdf=True, _feat=True)
    for k in KEYS:
        assert out[k].is_cuda and out[k].dtype == torch.float32 and tuple(out[k].shape) == g[k].shape
        worst = max(worst, float(np.abs(out[k].cpu().numpy().astype(np.float64) - g[k]).max()))
        assert np.array_equal(out[k].cpu().numpy()[:nv], pm[k])
    e_sdf = float(np.abs(out['sdf'].cpu().numpy() - g['sdf']).max())
    nf = g['feature'].shape[0]
    e_feat = float(np.abs(out['feature'].cpu().numpy()[:nf] - g['feature']).max())
    print(f"materials vs reference fixture ({which}): max abs err {worst:.3e}  sdf {e_sdf:.3e}  feature {e_feat:.3e}")
    assert worst <= PARITY_ATOL
    # the SDF MLP at fixed points: what test_extract_fields_and_sdf_surface_vs_reference holds it to
    assert np.allclose(out['sdf'].cpu().numpy(), g['sdf'], rtol=1e-5, atol=2e-6)
    assert np.allclose(out['feature'].cpu().numpy()[:nf], g['feature'], rtol=1e-5, atol=2e-6)


def test_reference_parity_stage1(gpu):
    g = golden('materials_stage1.npz')
    net, _ = stage1_net(gpu, overrides_of(g))
    check_against_fixture(net, g, None, gpu)


def test_reference_parity_stage2_inner(gpu):
    g = golden('materials_stage2_inner.npz')
    net, _ = stage2_net(gpu, overrides_of(g))
    check_against_fixture(net, g, 'inner', gpu)


def test_stage2_outer_is_the_stage1_bake_and_the_thick_model_bakes(gpu):
    from nu_nerf_amd.materials import bake_materials
    g = golden('materials_stage1.npz')
    x = torch.from_numpy(g['points']).to(gpu)
    net1, _ = stage1_net(gpu, overrides_of(g))
    ref = five(bake_materials(net1, x))
    over = {'stage1_network.' + k: v for k, v in overrides_of(g).items()}
    net2, _ = stage2_net(gpu, over)
    assert torch.equal(five(bake_materials(net2, x, which='outer')), ref)
    pm = net2.predict_materials((g['points'][:100], g['faces'][:0]), which='outer')
    assert np.array_equal(pm['albedo'], ref[:100, 2:5].cpu().numpy())
    assert not torch.equal(five(bake_materials(net2, x)), ref)                    # the default of a stage-2 model is the inner networks
    # non-zero thickness: AppShadingNetwork_SpecInner has the same three predictors; inner against its own layered path, outer as above
    net3, _ = stage2_net(gpu, over, thick=True)
    assert torch.equal(five(bake_materials(net3, x, which='outer')), ref)
    eng = net3.nets()[1].eng
    out = bake_materials(net3, x, transmission=True, _raw=True)
    _, raw = layered(eng, net3.nets()[1].named, x)
    assert torch.equal(torch.cat([five(out), out['transmission']], 1), raw)
    with pytest.raises(ValueError):
        bake_materials(net1, x, which='inner')


# ---- 2. feature columns and sdf, bit for bit ------------------------------------------------------------------------------------
def test_feature_and_sdf_bits(gpu):
    from nu_nerf_amd.materials import bake_materials
    from nu_nerf_amd.engine import addr
    net, _ = stage1_net(gpu)
    eng = net.engine()
    for n in (1, 32, 1000, 20000):
        x = ball(n, 11 + n, gpu)
        out = bake_materials(net, x, sdf=True, _feat=True)
        YX, _ = layered(eng, net._named(), x)
        assert torch.equal(out['feature'], YX[:, 1:257]) and torch.equal(out['sdf'], YX[:, 0])
        fused = eng.sdf_forward(addr(x), 3, n, keep=False, want_feat=False)['sdf']       # nu_sdf_fused_fwd
        assert torch.equal(out['sdf'], fused)


# ---- 3. row independence --------------------------------------------------------------------------------------------------------
def test_row_independence_bits(gpu):
    from nu_nerf_amd.materials import bake_materials
    net, _ = stage1_net(gpu)
    big = ball(100003, 77, gpu)
    full = bake_materials(net, big, transmission=True)
    full5 = torch.cat([five(full), full['transmission']], 1)
    again = bake_materials(net, big, transmission=True)
    assert torch.equal(torch.cat([five(again), again['transmission']], 1), full5)         # two calls, same bits
    probe = [0, 31, 32, 8191, 8192, 50001, 100002]
    for i in probe:
        for n in (1, 31, 32, 33, 8192):
            for pos in sorted({0, n // 2, n - 1}):
                batch = ball(n, 1000 + n + pos, gpu)
                batch[pos] = big[i]
                o = bake_materials(net, batch, transmission=True)
                row = torch.cat([five(o), o['transmission']], 1)[pos]
                assert torch.equal(row, full5[i]), (i, n, pos)
    # another position of the large batch (another tile, another slot in it, the ragged last tile)
    perm = torch.roll(torch.arange(100003, device=gpu), 12345)
    moved = bake_materials(net, big[perm].contiguous(), transmission=True)
    assert torch.equal(torch.cat([five(moved), moved['transmission']], 1), full5[perm])


# ---- 4. the layered path ---------------------------------------------------------------------------------------------------------
def test_against_the_layered_path(gpu):
    from nu_nerf_amd.materials import bake_materials
    net, _ = stage1_net(gpu)
    eng = net.engine()
    x = ball(50000, 4, gpu)
    YX, raw = layered(eng, net._named(), x)
    o_raw = bake_materials(net, x, transmission=True, _raw=True)
    assert torch.equal(torch.cat([five(o_raw), o_raw['transmission']], 1), raw)           # raw heads: the same bits
    out = bake_materials(net, x, transmission=True, sdf=True)
    mine = torch.cat([five(out), out['transmission']], 1)
    want = torch.sigmoid(raw)
    d = ulp_distance(mine, want)
    print(f"materials vs sigmoid(layered raw heads): max ulp distance {d}, max abs {float((mine - want).abs().max()):.3e}")
    assert d <= SIGMOID_ULPS
    assert torch.equal(out['sdf'], YX[:, 0])
    # nullable outputs: without transmission / sdf the others keep their bits; each of the first three may be left out too
    assert torch.equal(five(bake_materials(net, x)), mine[:, :5])
    e = lambda *s: torch.full(s, -7.0, device=gpu)                                        # noqa: E731
    alb, rough = e(50000, 3), e(50000)
    eng.material_bake(x.data_ptr(), 3, 50000, None, rough, alb)
    assert torch.equal(alb, mine[:, 2:5]) and torch.equal(rough, mine[:, 1])


# ---- 5. float64 ------------------------------------------------------------------------------------------------------------------
def test_against_float64(gpu):
    from nu_nerf_amd.materials import bake_materials
    from oracle import stage1_oracle as O
    g = golden('materials_stage1.npz')
    net, arrays = stage1_net(gpu, overrides_of(g))
    x = ball(4096, 64, gpu)
    out = bake_materials(net, x, transmission=True)
    p64 = {k: torch.from_numpy(np.asarray(v)).double().to(gpu) for k, v in arrays.items() if not k.endswith('FG_LUT')}
    with torch.no_grad():
        x64 = x.double()
        feat = O.sdf_forward(p64, x64)[:, 1:]
        inp = torch.cat([feat, x64], -1)
        want = torch.cat([O.predictor(p64, 'color_network.' + n, inp, 'sigmoid') for n in
                          ('metallic_predictor', 'roughness_predictor', 'albedo_predictor', 'transmisstion_weight')], 1)
    mine = torch.cat([five(out), out['transmission']], 1).double()
    err = float((mine - want).abs().max())
    span = (want.max(0).values - want.min(0).values).cpu().numpy()
    print(f"materials vs float64: max abs err {err:.3e}; channel spans {np.round(span, 4)}")
    assert (span[:5] >= 0.02).all()
    assert err <= PARITY_ATOL


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    from nu_nerf_amd.materials import bake_materials
    from nu_nerf_amd._lib import NuNerfLibraryError
    net, _ = stage1_net(gpu)
    x = ball(777, 9, gpu)
    ref = five(bake_materials(net, x))
    empty = bake_materials(net, x[:0], transmission=True)
    assert [tuple(empty[k].shape) for k in ('metallic', 'roughness', 'albedo', 'transmission')] == [(0, 1), (0, 1), (0, 3), (0, 1)]
    wide = torch.full((777, 8), float('nan'), device=gpu)                                 # x_ld = 8: the other columns are never read
    wide[:, :3] = x
    assert torch.equal(five(bake_materials(net, wide)), ref)
    for bad in (wide[:, :3], x.double(), x.half(), x[:, :2].contiguous(), x.reshape(-1), x.t().contiguous().t(), x.cpu()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            bake_materials(net, bad)
    assert torch.equal(five(bake_materials(net, x.cpu().numpy())), ref)                   # arrays are taken to the device


# ---- 7. the command --------------------------------------------------------------------------------------------------------------
def test_command_writes_the_relight_directory(gpu, tmp_path, monkeypatch):
    import yaml
    from nu_nerf_amd import extract_materials
    from nu_nerf_amd.mesh import write_ply, read_ply
    from nu_nerf_amd.lbvh import icosphere
    g = golden('materials_stage1.npz')
    net, _ = stage1_net(gpu, overrides_of(g))
    V, F = icosphere(1, 0.5)
    V = np.asarray(V, np.float32)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    os.makedirs('data/meshes')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}},
               'data/model/tiny/model.pth')
    write_ply('data/meshes/tiny-1234.ply', V, F)
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = extract_materials.main(['--cfg', 'tiny.yaml', '--ply'])
    assert out == os.path.join('data', 'materials', 'tiny-1234')
    want = net.predict_materials((V, F))
    for k, cols in (('metallic', 1), ('roughness', 1), ('albedo', 3)):
        a = np.load(os.path.join(out, k + '.npy'))
        assert a.dtype == np.float32 and a.shape == (len(V), cols) and np.array_equal(a, want[k])
    assert sorted(os.listdir(out)) == ['albedo.npy', 'metallic.npy', 'roughness.npy', 'tiny-1234_albedo.ply']
    V2, F2, C = read_ply(os.path.join(out, 'tiny-1234_albedo.ply'), colors=True)
    assert np.array_equal(V2, V) and np.array_equal(F2, np.asarray(F, np.int32))
    assert np.array_equal(C, np.rint(255.0 * want['albedo'].astype(np.float64)).astype(np.uint8))
    assert C.max() - C.min() >= 5
