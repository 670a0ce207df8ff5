"""Sphere tracing without a GPU: the float64 restatement of the per-ray algorithm (tests/sphere_trace_oracle.py) against the reference's
own sphere_tracing called one ray per call (tests/golden/sphere_trace.npz, scripts/gen_golden_sphere_trace.py), the float32 restatement
against the float64 one, the argument checks of trace_rays that need no device, and the command's arguments and paths."""
import os

import numpy as np
import pytest
import torch

import sphere_trace_oracle as SO
from helpers import golden


def arrays_of(name):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = init_stage1_params(6033)
    return arrays if name == 'init' else randomize_for_parity(arrays, seed=1)


@pytest.mark.parametrize('name', ['init', 'parity'])
def test_restatement_against_the_reference_fixture(name):
    """Positions and hit flags of the float64 restatement equal the reference's (one ray per call) to 1e-12 on 256 rays."""
    g = golden('sphere_trace.npz')
    o, d = SO.standard_rays()
    assert np.array_equal(o[:256], g['rays_o']) and np.array_equal(d[:256], g['rays_d'])
    assert g['pos_' + name].dtype == np.float64 and g['hit_' + name].dtype == np.bool_
    out = SO.trace(SO.sdf_fn(arrays_of(name)), g['rays_o'], g['rays_d'])
    hit = g['hit_' + name]
    assert np.array_equal(out['hit'], hit)
    assert np.abs(out['pos'] - g['pos_' + name]).max() <= 1e-12
    # the fixture exercises hit, leaving the sphere and never entering it
    moved = np.abs(g['pos_' + name] - g['rays_o']).max(1) > 0
    assert 0 < hit.sum() < moved.sum() < 256
    assert np.array_equal(out['entered'], moved) and not out['iters'][~moved].any()
    lost = moved & ~hit                                 # entered and did not hit: left the sphere, or ran out of iterations
    assert ((np.linalg.norm(g['pos_' + name][lost], axis=1) >= 1.0) | (out['iters'][lost] == 200)).all()


def test_float32_restatement_against_float64():
    """The same algorithm with every operation rounded to float32, on 512 rays of the parity network: the same rays enter, at most 0.5 %
    of them differ in the hit flag, positions of common hits within the 1e-4 cap of the GPU test, iteration counts at most 1 apart."""
    arrays = arrays_of('parity')
    o, d = SO.standard_rays(512)
    r64 = SO.trace(SO.sdf_fn(arrays), o, d)
    r32 = SO.trace(SO.sdf_fn(arrays, dtype=torch.float32), o, d, dtype=torch.float32)
    assert r32['pos'].dtype == np.float32 and np.array_equal(r32['entered'], r64['entered'])
    both = r32['hit'] & r64['hit']
    mism = int((r32['hit'] != r64['hit']).sum())
    err = float(np.abs(r32['pos'][both].astype(np.float64) - r64['pos'][both]).max())
    di = np.abs(r32['iters'][both].astype(np.int64) - r64['iters'][both])
    print(f"fp32 vs fp64 restatement, parity, 512 rays: entered {int(r64['entered'].sum())} hit {int(r64['hit'].sum())} "
          f"flag mismatches {mism}  max|dpos| {err:.3e}  iters equal {float((di == 0).mean()):.4f} max diff {int(di.max())}")
    assert mism <= 0.005 * r64['entered'].sum()
    assert err <= 1e-4 and di.max() <= 1 and (di == 0).mean() >= 0.95


def test_entry_step_orders_and_flags():
    o = torch.tensor([[0.0, 0.0, 3.0], [0.0, 0.0, 0.5], [0.0, 2.0, 3.0]], dtype=torch.float64)
    d = torch.tensor([[0.0, 0.0, -1.0]] * 3, dtype=torch.float64)
    x, t0, bounded = SO.entry(o, d, 1.0)
    assert bounded.tolist() == [True, True, False]
    assert torch.equal(x[0], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)) and float(t0[0]) == 2.0
    assert float(t0[1]) == -0.5 and torch.equal(x[1], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))     # the reference steps back
    assert torch.equal(x[2], o[2]) and float(t0[2]) == 0.0
    x, t0, _ = SO.entry(o, d, 1.0, entry_forward=True)
    assert float(t0[1]) == 0.0 and torch.equal(x[1], o[1])


class _NoEngine:
    """A stand-in renderer: every check below fails before an engine is asked for."""
    cfg = {'name': 'none'}


def test_trace_rays_argument_checks():
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.sdf_trace import trace_rays
    o = torch.zeros(8, 3)
    d = torch.ones(8, 3)
    bad_calls = [
        dict(rays_o=o.numpy(), rays_d=d),                                   # not a tensor
        dict(rays_o=o.double(), rays_d=d),                                  # dtype
        dict(rays_o=o[:, :2], rays_d=d),                                    # fewer than 3 columns
        dict(rays_o=o.reshape(-1), rays_d=d),                               # not 2-D
        dict(rays_o=o.t().contiguous().t(), rays_d=d),                      # column-major
        dict(rays_o=o, rays_d=d[:7]),                                       # counts differ
        dict(rays_o=o, rays_d=d, max_iter=0),
        dict(rays_o=o, rays_d=d, max_iter=2.5),
        dict(rays_o=o, rays_d=d, threshold=0.0),
        dict(rays_o=o, rays_d=d, threshold=float('nan')),
        dict(rays_o=o, rays_d=d, bound_radius=-1.0),
        dict(rays_o=o, rays_d=d, mask=torch.ones(7, dtype=torch.bool)),
        dict(rays_o=o, rays_d=d, mask=torch.ones(8)),
    ]
    for kw in bad_calls:
        with pytest.raises(NuNerfLibraryError, match=r"nu_sdf_trace failed with code -1"):
            trace_rays(_NoEngine(), **kw)
    with pytest.raises(ValueError, match='which'):
        trace_rays(_NoEngine(), o, d, which='inner')                        # a stage-1 renderer has no inner SDF
    with pytest.raises(ValueError, match='which'):
        trace_rays(_NoEngine(), o, d, which='middle')


def test_render_surface_argument_checks():
    from nu_nerf_amd.sdf_trace import AOVS, render_surface
    K, pose = np.eye(3), np.eye(4)[:3]
    assert set(('mask', 'depth', 'position', 'normal', 'albedo', 'roughness', 'metallic', 'mean_curvature', 'gaussian_curvature')) == set(AOVS)
    with pytest.raises(ValueError, match='aovs'):
        render_surface(_NoEngine(), K, pose, 4, 4, aovs=('depth', 'colour'))
    with pytest.raises(ValueError, match='aovs'):
        render_surface(_NoEngine(), K, pose, 4, 4, aovs=())
    with pytest.raises(ValueError, match='chunk'):
        render_surface(_NoEngine(), K, pose, 4, 4, chunk=0)
    with pytest.raises(ValueError):
        render_surface(_NoEngine(), K, pose, 0, 4)
    with pytest.raises(TypeError):
        render_surface(_NoEngine(), K, pose, 4, 4, entry_forward=False)


def test_renderers_have_the_method():
    from nu_nerf_amd import renderer, renderer_std, stage2, stage2_thick
    for cls in (renderer.NeROShapeRenderer, renderer_std.NeROShapeRenderer, stage2.Stage2Renderer, stage2_thick.Stage2Renderer):
        assert callable(getattr(cls, 'render_surface'))


def test_header_declares_the_entry():
    from nu_nerf_amd import _lib
    assert _lib.NU_TRACE_ENTRY_FORWARD == 1
    sig = {name: (res, args) for name, res, args in _lib._signatures()}
    res, args = sig['nu_sdf_trace']
    assert res is _lib.c_int and len(args) == 17
    assert args == [_lib.c_p, _lib.c_p, _lib.c_int, _lib.c_p, _lib.c_int, _lib.c_int, _lib.c_p, _lib.c_int, _lib.c_f, _lib.c_f, _lib.c_int,
                    _lib.c_p, _lib.c_p, _lib.c_p, _lib.c_p, _lib.c_p, _lib.c_p]


def test_kernel_keeps_no_scratch():
    """The register bar of the fused kernels: no VGPR spill, no scratch, and the LDS footprint DESIGN.md section 27 states (one workgroup per CU)."""
    import sys
    from nu_nerf_amd import build
    build.build(verbose=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    from kernel_regs import kernel_table
    table = dict(kernel_table(os.path.join(root, 'nu_nerf_amd', 'build', 'sdf_trace.o')))
    (name, r), = [(k, v) for k, v in table.items() if k.startswith('sdf_trace_kernel')]
    assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] == 153108, (name, r)


def test_command_arguments_and_paths(tmp_path):
    from nu_nerf_amd import relight, render_surface as RS
    f = RS.parse_args(['--cfg', 'a.yaml'])
    assert (f.poses, f.hw, f.aovs, f.ckpt, f.stage2, f.which, f.max_iter, f.threshold, f.bound_radius) == \
        ('relight', 800, ('depth', 'normal', 'mask'), None, False, None, 200, 1e-5, 1.0)
    assert RS.which_of(f) == 'outer'
    assert RS.output_dir(f, 'bear', 300000) == os.path.join('data', 'surface', 'bear-300000')
    paths = RS.frame_paths(RS.output_dir(f, 'bear', 300000), 3, f.aovs)
    assert paths == {'depth': os.path.join('data', 'surface', 'bear-300000', '3_depth.png'),
                     'normal': os.path.join('data', 'surface', 'bear-300000', '3_normal.png'),
                     'mask': os.path.join('data', 'surface', 'bear-300000', '3_mask.png'),
                     'depth.npy': os.path.join('data', 'surface', 'bear-300000', '3_depth.npy')}
    assert 'depth.npy' not in RS.frame_paths('x', 0, ('mask', 'albedo'))
    K, poses = RS.cameras(f)
    assert np.array_equal(K, relight.intrinsics(800, 800)) and np.array_equal(poses, relight.relighting_poses(8, 0.0, 45.0, 3.0))

    f = RS.parse_args(['--cfg', 'a.yaml', '--stage2', '--which', 'outer', '--hw', '64', '--aovs', 'albedo', 'mask', 'albedo', '--out', 'o',
                       '--num', '2', '--ckpt', 'none'])
    assert RS.which_of(f) == 'outer' and f.aovs == ('albedo', 'mask') and RS.output_dir(f, 'n', 1) == 'o' and f.ckpt == 'none'
    assert RS.which_of(RS.parse_args(['--cfg', 'a.yaml', '--stage2'])) == 'inner'
    assert len(RS.cameras(f)[1]) == 2

    np.savez(tmp_path / 'cams.npz', poses=np.tile(np.eye(4)[:3], (5, 1, 1)), K=2 * np.eye(3))
    f = RS.parse_args(['--cfg', 'a.yaml', '--poses', str(tmp_path / 'cams.npz'), '--hw', '32'])
    K, poses = RS.cameras(f)
    assert np.array_equal(K, 2 * np.eye(3)) and poses.shape == (5, 3, 4)
    np.savez(tmp_path / 'bad.npz', poses=np.eye(4))
    with pytest.raises(SystemExit):
        RS.cameras(RS.parse_args(['--cfg', 'a.yaml', '--poses', str(tmp_path / 'bad.npz')]))
    for bad in (['--which', 'inner'], ['--hw', '0'], ['--aovs', 'colour'], ['--poses', 'orbit'], ['--threshold', '0'], ['--max_iter', '0'],
                ['--bound_radius', '-1']):
        with pytest.raises(SystemExit):
            RS.parse_args(['--cfg', 'a.yaml'] + bad)
    with pytest.raises(SystemExit):
        RS.parse_args([])


def test_png_encoding_of_the_aovs():
    from nu_nerf_amd.render_surface import to_rgba
    mask = np.array([[255, 0], [255, 255]], np.uint8)
    depth = np.array([[2.0, 0.0], [3.0, 2.5]], np.float32)
    rgba = to_rgba('depth', depth, mask)
    assert rgba.dtype == np.uint8 and rgba.shape == (2, 2, 4)
    assert rgba[0, 0].tolist() == [0, 0, 0, 255] and rgba[1, 0].tolist() == [255, 255, 255, 255] and rgba[0, 1].tolist() == [0, 0, 0, 0]
    assert rgba[1, 1].tolist() == [128, 128, 128, 255]
    m = to_rgba('mask', mask, mask)
    assert m[0, 1].tolist() == [0, 0, 0, 255] and m[0, 0].tolist() == [255, 255, 255, 255]
    n = np.zeros((2, 2, 3), np.float32)
    n[..., 2] = 1.0
    assert to_rgba('normal', n, mask)[0, 0].tolist() == [128, 128, 255, 255]
    assert to_rgba('gaussian_curvature', np.full((2, 2), 10.0, np.float32), mask)[0, 0].tolist() == [255, 255, 255, 255]
