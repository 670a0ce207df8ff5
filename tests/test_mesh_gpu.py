"""Mesh extraction on the GPU (nu_nerf_amd.mesh, csrc/mcubes.hip): marching cubes against the tables and an independent numpy
marching cubes, topology / orientation on analytic SDFs, the device SDF grid against extract_fields and the reference-generated
grid, determinism, the stage-1 -> stage-2 hand-over, and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import golden
from test_mesh_host import CORNERS, EDGES, parse_tables, numpy_marching_cubes, directed_edge_defects

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S1CFG = {'name': 'golden', 'network': 'shape', 'database_name': 'synthetic/64', 'apply_occ_loss': True, 'occ_loss_step': 15000,
         'is_nerf': True, 'freeze_inv_s_step': 15000, 'n_samples': 32, 'n_importance': 32, 'n_bg_samples': 16}


def golden_net(gpu):
    """The stage-1 network of tests/golden/eval_step20000_r40.npz (as test_eval_gpu builds it)."""
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    g = golden("eval_step20000_r40.npz")
    net = NeROShapeRenderer(dict(S1CFG), training=False)
    params = randomize_for_parity(init_stage1_params(6033), seed=1)
    for k in g:
        if k.startswith('override__'):
            params[k[len('override__'):]] = g[k]
    net.load_param_dict(params)
    return net.to(gpu), g


def nograd_query(eng):
    from nu_nerf_amd.engine import addr
    eng.pack()

    def q(x):
        x = x.contiguous()
        return eng.sdf_forward(addr(x), 3, x.shape[0], keep=False, want_feat=False)['sdf']
    return q


def test_all_256_cube_cases(gpu):
    from nu_nerf_amd.mesh import marching_cubes
    _, tri = parse_tables()
    for c in range(256):
        u = torch.ones(2, 2, 2)
        for b, (dx, dy, dz) in enumerate(CORNERS):
            if (c >> b) & 1:
                u[dx, dy, dz] = -1.0
        V, F = marching_cubes(u.to(gpu), 0.0)
        V, F = V.cpu().numpy(), F.cpu().numpy()
        assert len(F) * 3 == len(tri[c]), c
        mids = {}
        for a, b in EDGES:
            if (u[CORNERS[a]] < 0) != (u[CORNERS[b]] < 0):
                mids[tuple((np.array(CORNERS[a]) + np.array(CORNERS[b])) / 2.0)] = True
        assert len(V) == len(mids), c
        for v in V:
            assert tuple(v.astype(np.float64)) in mids, (c, v)
        for f in F:
            assert len(set(f.tolist())) == 3, c
            area = np.cross(V[f[1]] - V[f[0]], V[f[2]] - V[f[0]])
            assert np.linalg.norm(area) > 1e-6, c
        Vn, Fn = numpy_marching_cubes(u.numpy(), 0.0)
        assert np.array_equal(F, Fn) and np.array_equal(V, Vn), c


@pytest.mark.parametrize("field", ["random", "golden"])
def test_marching_cubes_matches_numpy_reference(gpu, field):
    from nu_nerf_amd.mesh import marching_cubes
    if field == "random":
        u = np.random.default_rng(5).normal(size=(17, 23, 19)).astype(np.float32)      # non-cubic: axis mix-ups show
    else:
        u = golden("eval_step20000_r40.npz")['grid']
        assert u.shape == (24, 24, 24)
    V, F = marching_cubes(u, 0.0)                             # numpy in, numpy out
    Vn, Fn = numpy_marching_cubes(u, 0.0)
    assert len(Fn) > 50
    assert F.dtype == np.int32 and V.dtype == np.float32
    assert np.array_equal(F, Fn)
    np.testing.assert_allclose(V, Vn, rtol=0, atol=1e-5)
    Vd, Fd = marching_cubes(torch.from_numpy(u).to(gpu), 0.0)   # device in, device out
    assert Vd.is_cuda and torch.equal(Fd.cpu(), torch.from_numpy(F))


def _analytic(res, kind):
    x = torch.linspace(-1.0, 1.0, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(x, x, x, indexing='ij')
    if kind == "sphere":
        return (torch.sqrt(X * X + Y * Y + Z * Z) - 0.6).float()
    return (torch.sqrt((torch.sqrt(X * X + Y * Y) - 0.5) ** 2 + Z * Z) - 0.2).float()


@pytest.mark.parametrize("kind,euler", [("sphere", 2), ("torus", 0)])
def test_topology_and_orientation_on_analytic_sdfs(gpu, kind, euler):
    from nu_nerf_amd.mesh import marching_cubes, _to_world
    res = 64
    V, F = marching_cubes(_analytic(res, kind).to(gpu), 0.0)
    W = _to_world(V, res, (-1, -1, -1), (1, 1, 1)).astype(np.float64)
    F = F.cpu().numpy()
    assert directed_edge_defects(F) == 0                                        # closed, consistently oriented 2-manifold
    n_edges = 3 * len(F) // 2
    assert len(W) - n_edges + len(F) == euler
    cell = 2.0 / (res - 1)
    if kind == "sphere":
        assert np.abs(np.linalg.norm(W, axis=1) - 0.6).max() < cell
    else:
        rho = np.sqrt((np.linalg.norm(W[:, :2], axis=1) - 0.5) ** 2 + W[:, 2] ** 2)
        assert np.abs(rho - 0.2).max() < cell
    Ff = np.fliplr(F)                                                            # extract_mesh_stage1.py:40
    a, b, c = W[Ff[:, 0]], W[Ff[:, 1]], W[Ff[:, 2]]
    vol = float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
    exact = 4.0 / 3.0 * np.pi * 0.6 ** 3 if kind == "sphere" else 2 * np.pi ** 2 * 0.5 * 0.2 ** 2
    assert vol > 0 and abs(vol - exact) < 0.02 * exact, (vol, exact)


def test_inside_test_matches_torch_norm_bit_for_bit(gpu):
    """The compaction's |x| >= 1 test against torch.norm on coordinates packed around the unit sphere (x = y = z ~ 1/sqrt(3))."""
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd.mesh import _lib as mlib, _workspace
    from nu_nerf_amd.engine import addr
    lib = mlib()
    g = torch.Generator().manual_seed(0)
    n = 96
    X, Y, Z = ((0.5773503 + (torch.rand(n, generator=g) - 0.5) * 2e-6).float() for _ in range(3))
    ws, nb = _workspace(lib, gpu, n, n, n)
    rows_at = torch.empty(2, dtype=torch.int64, device=gpu)
    Xd, Yd, Zd = X.to(gpu), Y.to(gpu), Z.to(gpu)
    c_p, c_ll = ctypes.c_void_p, ctypes.c_longlong
    npts = n ** 3
    chunk = (npts + 255) // 256 * 256
    L.check(lib.nu_grid_inside_count(c_p(addr(Xd)), c_p(addr(Yd)), c_p(addr(Zd)), n, n, n, c_ll(chunk), c_p(addr(ws)), c_ll(nb),
                                     c_p(addr(rows_at)), L.stream()), "nu_grid_inside_count")
    P = int(rows_at[1])
    u = torch.empty(n, n, n, device=gpu)
    val = torch.zeros(max(P, 1), device=gpu)
    L.check(lib.nu_grid_scatter(c_p(addr(Xd)), c_p(addr(Yd)), c_p(addr(Zd)), n, n, n, c_ll(0), c_ll(npts), c_p(addr(ws)), c_ll(nb),
                                c_p(addr(val)), ctypes.c_float(1.0), c_p(addr(u)), L.stream()), "nu_grid_scatter")
    xx, yy, zz = torch.meshgrid(X, Y, Z, indexing='ij')
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).to(gpu)
    outside = (torch.norm(pts, dim=-1) >= 1.0).reshape(n, n, n)
    assert 0.2 < float(outside.float().mean()) < 0.8                             # the test really straddles the sphere
    assert torch.equal(u == 1.0, outside) and P == int((~outside).sum())


@pytest.mark.parametrize("res,slab", [(24, None), (97, 50000)])
def test_sdf_grid_matches_extract_fields(gpu, res, slab):
    from nu_nerf_amd.mesh import sdf_grid
    from nu_nerf_amd.validation import extract_fields
    net, g = golden_net(gpu)
    eng = net.engine()
    bmin, bmax = torch.from_numpy(g['grid_min']).to(gpu), torch.from_numpy(g['grid_max']).to(gpu)
    u = sdf_grid(eng, bmin, bmax, res, slab_points=slab).cpu().numpy()
    if slab is not None:
        assert res ** 3 % (slab // 256 * 256) != 0 and res ** 3 > 4 * slab           # several uneven slabs
    # the same no-grad forward on the queried points: bit-identical
    ref = extract_fields(bmin, bmax, res, nograd_query(eng))
    assert (u == 1.0).sum() == (ref == 1.0).sum() and np.array_equal(u == 1.0, ref == 1.0)
    assert np.array_equal(u.view(np.int32), ref.view(np.int32))
    # the gradient-carrying SdfFn path (its sdf column may come from another head kernel)
    ref2 = extract_fields(bmin, bmax, res, lambda x: net.sdf_network.sdf(x))
    assert np.array_equal(u == 1.0, ref2 == 1.0)
    np.testing.assert_allclose(u, ref2, rtol=1e-5, atol=2e-6)
    if res == 24:
        # the reference-generated grid stores -sdf (outside: 1)
        un = sdf_grid(eng, bmin, bmax, res, outside_val=-1.0).cpu().numpy()
        assert np.array_equal(un == -1.0, g['grid'] == 1.0)
        np.testing.assert_allclose(un, -g['grid'], rtol=1e-5, atol=2e-6)


def test_extraction_is_deterministic(gpu):
    from nu_nerf_amd.mesh import extract_mesh, sdf_grid
    net, _ = golden_net(gpu)
    u1 = sdf_grid(net.engine(), (-1, -1, -1), (1, 1, 1), 128)
    u2 = sdf_grid(net.engine(), (-1, -1, -1), (1, 1, 1), 128)
    assert torch.equal(u1.view(torch.int32), u2.view(torch.int32))
    V1, F1 = extract_mesh(net, 128)
    V2, F2 = extract_mesh(net, 128)
    assert len(F1) > 1000
    assert V1.tobytes() == V2.tobytes() and np.array_equal(F1, F2)


def test_extract_geometry_any_query_func(gpu):
    from nu_nerf_amd.mesh import extract_geometry, extract_mesh
    net, _ = golden_net(gpu)
    eng = net.engine()
    b = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    V, F = extract_geometry(b[0], b[1], 40, 0.0, nograd_query(eng))
    Vm, Fm = extract_mesh(net, 40)
    assert V.tobytes() == Vm.tobytes() and np.array_equal(F, Fm)


def _stage2_net(gpu, mesh_arrays):
    from nu_nerf_amd.stage2 import Stage2Renderer
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, randomize_for_parity
    s1 = randomize_for_parity(init_stage1_params(6033), seed=1)
    p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
        p2['color_network.stage1_network.' + k] = v
    cfg = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'shader_config': {'sphere_direction': False, 'human_light': False},
           'eikonal_weight': 0.02, 'freeze_inv_s_step': 5000,
           'stage1_cfg': {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000},
           'stage1_mesh_arrays': mesh_arrays}
    net = Stage2Renderer(cfg, training=False)
    net.load_param_dict(p2)
    return net.to(gpu), cfg


def test_stage1_mesh_feeds_stage2(gpu):
    from nu_nerf_amd.mesh import extract_mesh
    from nu_nerf_amd.loss import name2loss, total_loss
    from nu_nerf_amd.lbvh import LBVH
    net1, _ = golden_net(gpu)
    V, F = extract_mesh(net1, 64)
    F = np.ascontiguousarray(np.fliplr(F))
    assert len(F) > 500
    net, cfg = _stage2_net(gpu, (V, F))
    g = golden("stage2_step6000_r24.npz")
    batch = {k: torch.from_numpy(g[k]).to(gpu) for k in ('rays_o', 'rays_d', 'rgbs')}
    out = net.train_step_rays(batch, int(g['step']))
    total, log = total_loss(out, [name2loss[n](cfg) for n in ('eikonal', 'std', 'nerf_render')], int(g['step']))
    total.backward()
    assert torch.isfinite(total).item()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(gr).all()) for gr in grads)
    assert any(float(gr.abs().sum()) > 0 for gr in grads)
    bvh = LBVH(torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu))
    rng = np.random.default_rng(11)
    o = rng.normal(size=(20000, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 3.0
    d = rng.normal(size=(20000, 3)) * 0.3 - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32)).to(gpu)
    h1, i1 = bvh.intersect(rays)
    h2, i2 = bvh.intersect_brute(rays)
    assert int((h1 > 0).sum()) > 1000
    assert torch.equal(h1, h2) and torch.equal(i1, i2)


def _run_cli(args, cwd):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, "-m", "nu_nerf_amd.extract_mesh"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_stage1_and_stage2(gpu, tmp_path):
    import yaml
    from nu_nerf_amd.mesh import extract_mesh, marching_cubes, sdf_grid, stage2_inner_grid, write_ply, _to_world
    from nu_nerf_amd.stage2 import read_ply
    from nu_nerf_amd.train_glue import save_checkpoint
    from nu_nerf_amd.lbvh import icosphere
    net, _ = golden_net(gpu)
    cfg = dict(S1CFG, zero_thickness=True)
    (tmp_path / "s1.yaml").write_text(yaml.safe_dump(cfg))
    os.makedirs(tmp_path / "data" / "model" / "golden")
    save_checkpoint(str(tmp_path / "data" / "model" / "golden" / "model.pth"), net, torch.optim.Adam(net.parameters()), 1234)
    _run_cli(["--cfg", "s1.yaml", "--resolution", "40"], str(tmp_path))
    V, F = read_ply(str(tmp_path / "data" / "meshes" / "golden-1234.ply"))
    Vm, Fm = extract_mesh(net, 40)
    assert len(F) > 500 and V.tobytes() == Vm.tobytes() and np.array_equal(F, np.fliplr(Fm))

    # --stage2 on a Stage2Renderer checkpoint; its mesh comes from a PLY the config names
    write_ply(str(tmp_path / "ico.ply"), *icosphere(3, 0.5))
    net2, cfg2 = _stage2_net(gpu, icosphere(3, 0.5))
    cfg2 = {k: v for k, v in cfg2.items() if k != 'stage1_mesh_arrays'}
    cfg2.update(zero_thickness=True, stage1_mesh_dir=str(tmp_path / "ico.ply"))
    (tmp_path / "s2.yaml").write_text(yaml.safe_dump(cfg2))
    save_checkpoint(str(tmp_path / "s2.pth"), net2, torch.optim.Adam(net2.parameters()), 77)
    _run_cli(["--cfg", "s2.yaml", "--resolution", "40", "--stage2", "--ckpt", "s2.pth", "--out", "inner.ply"], str(tmp_path))
    V2, F2 = read_ply(str(tmp_path / "inner.ply"))
    u = stage2_inner_grid(net2, 40)
    s1 = sdf_grid(net2.stage1_network.engine(), (-1, -1, -1), (1, 1, 1), 40)
    inner = sdf_grid(net2.nets()[1].eng, (-1, -1, -1), (1, 1, 1), 40)
    sel = torch.where(s1 < 0, inner, torch.ones_like(inner))
    assert torch.equal(u.view(torch.int32), sel.view(torch.int32))
    Vr, Fr = marching_cubes(u, 0.0)
    assert len(F2) > 100 and V2.tobytes() == _to_world(Vr, 40, (-1, -1, -1), (1, 1, 1)).tobytes()
    assert np.array_equal(F2, Fr.cpu().numpy())                                 # no face flip for the stage-2 mesh
