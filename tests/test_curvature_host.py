"""Curvature from the SDF's Hessian, host side (no GPU): the float64 oracle of tests/curvature_oracle.py against closed forms (the
formulas and their sign), Gauss-Bonnet of the oracle on the init network, the analytic network's parameters against its closed form
through the oracle, the command's argument parser, and the validation of the opt-in consumers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import curvature_oracle as CO
from test_mesh_host import directed_edge_defects, numpy_marching_cubes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def points(n, seed, lo=0.2, hi=0.95):
    g = np.random.Generator(np.random.PCG64(seed))
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * g.uniform(lo, hi, (n, 1))


def test_formulas_and_sign_on_a_sphere():
    """f = |x - c| - r: mean = 1 / rho, gaussian = 1 / rho^2 on the level set of radius rho = |x - c| (positive: convex body, normal
    outward), normal = (x - c) / rho; to 1e-12."""
    c = torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64)
    x = points(64, 1) + c.numpy()
    f, g, H6 = CO.jet_of(lambda t: (t - c).norm(dim=1) - 0.37, x)
    mean, gauss, normal = CO.curvatures(g, H6)
    rho = np.linalg.norm(x - c.numpy(), axis=1)
    assert np.abs(f - (rho - 0.37)).max() <= 1e-12
    assert np.abs(mean * rho - 1.0).max() <= 1e-12
    assert np.abs(gauss * rho ** 2 - 1.0).max() <= 1e-12
    assert np.abs(normal - (x - c.numpy()) / rho[:, None]).max() <= 1e-12
    # the curvature belongs to the level set, not to the function: any increasing reparametrisation gives the same numbers
    _, g2, H62 = CO.jet_of(lambda t: ((t - c) ** 2).sum(1) * 3.0, x)
    mean2, gauss2, _ = CO.curvatures(g2, H62)
    assert np.abs(mean2 * rho - 1.0).max() <= 1e-12 and np.abs(gauss2 * rho ** 2 - 1.0).max() <= 1e-12
    # and the inside-out function flips the mean curvature's sign, not the Gaussian's
    mean3, gauss3, normal3 = CO.curvatures(-g, -H6)
    assert np.array_equal(mean3, -mean) and np.array_equal(gauss3, gauss) and np.array_equal(normal3, -normal)


def test_formulas_on_an_ellipsoid():
    abc = np.array([0.9, 0.6, 0.4])
    x = points(64, 2)
    t_abc = torch.from_numpy(abc)
    for fn in (lambda t: ((t / t_abc) ** 2).sum(1) - 1.0, lambda t: ((t / t_abc) ** 2).sum(1).sqrt()):
        _, g, H6 = CO.jet_of(fn, x)
        _, gauss, _ = CO.curvatures(g, H6)
        want = CO.ellipsoid_gaussian(x, abc)
        assert np.abs(gauss / want - 1.0).max() <= 1e-12


def test_degenerate_gradient_gives_zeros():
    g = np.array([[0.0, 0.0, 0.0], [1e-7, 0.0, 0.0], [0.0, 2e-6, 0.0]])
    H6 = np.ones((3, 6))
    mean, gauss, normal = CO.curvatures(g, H6)
    assert mean[0] == 0 and gauss[0] == 0 and not normal[0].any() and mean[1] == 0 and not normal[1].any()
    assert np.isfinite(mean).all() and np.isfinite(gauss).all() and abs(normal[2, 1] - 1.0) <= 1e-15


@pytest.fixture(scope='module')
def init_arrays():
    from nu_nerf_amd.params import init_stage1_params
    return init_stage1_params(6033)


def test_gauss_bonnet_of_the_oracle(init_arrays):
    """The init network (a sphere of radius ~0.5 by the geometric initialisation) on a 48^3 grid over [-1,1]^3: the marching-cubes mesh
    of the float64 SDF is closed with Euler characteristic 2, and sum_v K(v) A_v / 4 pi is within 0.01 of 1 (measured 0.0036)."""
    from oracle import stage1_oracle as O
    from nu_nerf_amd.curvature import euler_characteristic, gauss_bonnet_ratio, vertex_areas
    n = 48
    ax = np.linspace(-1.0, 1.0, n)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    p64 = CO.params64(init_arrays)
    with torch.no_grad():
        u = O.sdf_forward(p64, torch.from_numpy(grid))[:, 0].numpy().reshape(n, n, n)
    Vg, F = numpy_marching_cubes(u, 0.0)
    V = -1.0 + Vg.astype(np.float64) * (2.0 / (n - 1))
    assert directed_edge_defects(F) == 0
    chi = euler_characteristic(len(V), F)
    assert chi == 2
    K = CO.sdf_jet64(init_arrays, V)['gaussian']
    A = vertex_areas(V, F)
    ratio = float(np.sum(K * A) / (4.0 * math.pi))
    print(f"Gauss-Bonnet of the float64 oracle, init network, {n}^3: V {len(V)}  sum K A / 4 pi = {ratio:.6f}")
    assert abs(ratio - 1.0) <= 0.01
    assert abs(gauss_bonnet_ratio(K, V, F) - ratio) <= 1e-12            # the package's host statistic is the same sum


def test_analytic_network_is_its_closed_form(init_arrays):
    """The pass-through parameters of curvature_oracle.analytic_overrides, evaluated by the float64 oracle of the real network, give the
    closed form: value, gradient and Hessian to the rounding of the float32 parameters (weight norm and the skip's sqrt 2 are float32
    numbers: 1e-7 relative on coefficients whose second derivatives reach 4), including the k = 5 columns and the skip path."""
    A, B = CO.analytic_coefficients()
    assert all(A[CO.embed_col(5, c, s)] != 0 and B[CO.embed_col(5, c, s)] != 0 for c in range(3) for s in (False, True))
    arrays = dict(init_arrays)
    arrays.update(CO.analytic_overrides(A, B, init_arrays))
    x = points(256, 3).astype(np.float32)
    got = CO.sdf_jet64(arrays, x)
    f, g, H6 = CO.analytic_jet(A, B, x)
    errs = [float(np.abs(got[k] - w).max()) for k, w in (('sdf', f), ('gradient', g), ('hessian', H6))]
    print("analytic network, float64 oracle vs closed form: max abs err sdf %.2e gradient %.2e hessian %.2e" % tuple(errs))
    assert errs[0] <= 1e-6 and errs[1] <= 1e-6 and errs[2] <= 2e-6
    assert np.abs(H6[:, :3]).max() > 2.0 and np.abs(H6[:, 3:]).max() == 0.0
    # the field whose gradient vanishes at the origin
    A0, B0 = CO.analytic_coefficients(only_cos0=True)
    arrays.update(CO.analytic_overrides(A0, B0, init_arrays))
    z = CO.sdf_jet64(arrays, np.zeros((1, 3)))
    assert not z['gradient'].any() and z['mean'][0] == 0 and z['gaussian'][0] == 0 and not z['normal'].any()
    assert np.abs(z['hessian'][0, :3]).min() > 0.1


def test_command_parser_and_help():
    r = subprocess.run([sys.executable, "-m", "nu_nerf_amd.extract_curvature", "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--cfg", "--mesh", "--ckpt", "--out", "--stage2", "--inner", "--outer"):
        assert flag in r.stdout
    from nu_nerf_amd.extract_curvature import FILES, output_paths, parse_args, which_of
    a = parse_args(["--cfg", "x.yaml"])
    assert a.mesh is None and a.ckpt is None and a.out is None and not a.stage2 and which_of(a) == 'outer'
    assert output_paths(a, 'cat', 300000) == (os.path.join('data', 'meshes', 'cat-300000.ply'), os.path.join('data', 'materials', 'cat-300000'))
    assert which_of(parse_args(["--cfg", "x.yaml", "--stage2"])) == 'inner'
    assert which_of(parse_args(["--cfg", "x.yaml", "--stage2", "--outer", "--mesh", "m.ply"])) == 'outer'
    assert FILES == {'gaussian': 'curvature.npy', 'mean': 'mean_curvature.npy', 'normal': 'sdf_normal.npy'}
    with pytest.raises(SystemExit):
        parse_args(["--cfg", "x.yaml", "--outer"])
    with pytest.raises(SystemExit):
        parse_args([])


def test_relight_takes_a_shell_curvature_file(tmp_path):
    from nu_nerf_amd.relight import load_shell_curvature, parse_args
    base = ['--mesh', 'o.ply', '--hdr', 'e.hdr', '--name', 'n']
    nested = base + ['--inner', 'i.ply', '--inner-material', 'mi']
    assert parse_args(nested + ['--shell', '1.5,0.004']).shell_curvature is None
    assert parse_args(nested + ['--shell', '1.5,0.004', '--shell-curvature', 'c.npy']).shell_curvature == 'c.npy'
    with pytest.raises(SystemExit):
        parse_args(nested + ['--shell-curvature', 'c.npy'])           # the solid-glass shell has no curvature input
    p = str(tmp_path / 'curvature.npy')
    np.save(p, np.array([[0.5], [-20.0], [140.0]], np.float32))
    c = load_shell_curvature(p, 3)
    assert c.dtype == np.float32 and c.tolist() == [0.5, -10.0, 10.0]
    with pytest.raises(ValueError):
        load_shell_curvature(p, 4)


def test_consumer_validation():
    from nu_nerf_amd.lbvh import check_vertex_curvature
    from nu_nerf_amd.stage2_thick import Stage2Renderer
    assert Stage2Renderer.default_cfg['shell_curvature'] == 'mesh'
    assert Stage2Renderer.check_shell_curvature('sdf') == 'sdf'
    for bad in ('SDF', 'hessian', None, 1):
        with pytest.raises(ValueError, match='shell_curvature'):
            Stage2Renderer.check_shell_curvature(bad)
    with pytest.raises(ValueError, match='shell_curvature'):            # the constructor refuses it before anything is loaded
        Stage2Renderer({'name': 'x', 'shell_curvature': 'pymesh'}, training=False)
    c = check_vertex_curvature(torch.tensor([0.5, -11.0, 140.0, 10.0]), 4)
    assert tuple(c.shape) == (4, 1) and c.dtype == torch.float32 and c.reshape(-1).tolist() == [0.5, -10.0, 10.0, 10.0]
    assert torch.equal(check_vertex_curvature(np.array([[0.5], [-11.0], [140.0], [10.0]]), 4), c)
    for bad in (torch.zeros(3), torch.zeros(4, 2), torch.tensor([0.0, float('nan'), 0.0, 0.0]), torch.tensor([0.0, float('inf'), 0.0, 0.0])):
        with pytest.raises(ValueError, match='curvature'):
            check_vertex_curvature(bad, 4)


def test_mesh_statistics():
    from nu_nerf_amd.curvature import curvature_stats, euler_characteristic, gauss_bonnet_ratio, vertex_areas
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(2, 0.5)
    assert euler_characteristic(len(V), F) == 2
    A = vertex_areas(V, F)
    assert abs(A.sum() / (4 * math.pi * 0.25) - 1.0) < 0.03
    assert abs(gauss_bonnet_ratio(np.full(len(V), 4.0), V, F) - A.sum() * 4.0 / (4 * math.pi)) <= 1e-12
    torus_like = np.array([[0, 1, 2]])                                  # V - E + F = 3 - 3 + 1
    assert euler_characteristic(3, torus_like) == 1
    s = curvature_stats(np.array([0.0, 1.0, 2.0, 30.0]))
    assert s['outside_pm10'] == 0.25 and s['p50'] == 1.5


def test_kernel_is_bound_and_keeps_no_scratch():
    """The header declares the entry with its eleven arguments and no new struct; the kernel has no VGPR spill, no scratch and the LDS
    footprint DESIGN.md section 26 states."""
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert len(lib.nu_sdf_jet_fwd.argtypes) == 11 and 'SjNet' not in _lib.STRUCTS
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    from kernel_regs import kernel_table
    table = dict(kernel_table(os.path.join(ROOT, 'nu_nerf_amd', 'build', 'sdf_jet.o')))
    (name, r), = [(k, v) for k, v in table.items() if k.startswith('sdf_jet_fwd_kernel')]
    assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] == 150800, (name, r)
