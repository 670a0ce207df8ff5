"""Writes tests/golden/materials_stage1.npz and materials_stage2_inner.npz: per-vertex materials as the REFERENCE's own modules
compute them on the CPU (predict_materials, network/renderer_zerothick.py:846-864: feature = sdf_network(x)[:, 1:],
color_network.predict_materials(x, feature)).

Run once on a machine with the reference checkout, from its directory (the import shims are those of oracle/gen_golden.py):

    cd <reference> && python <repo>/scripts/gen_materials_golden.py

The test suite needs neither this script nor the reference, only the .npz files.  The parameters are seed-generated
(randomize_for_parity(init_stage1_params(6033), seed=1) as in oracle/gen_golden_eval.py; the stage-2 set of tests/test_stage2_gpu.py),
so a fixture holds the points, the expected arrays (sdf, materials; the feature columns of the first N_FEATURE_ROWS points) and the
overrides only.

Overrides: with the parity parameters as they are the material heads barely move over the points (metallic 0.535..0.536), and a
test could pass on a constant.  The head layers' weight_g are therefore scaled by HEAD_GAIN and recorded as `override__<key>`
entries (the convention of the eval fixture); the generator asserts that each of the five channels spans at least MIN_SPAN and stays
inside [LO, HI], and the tests re-assert it on the fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from gen_golden import install_shims, to_t   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
HEAD_GAIN = 30.0
MIN_SPAN, LO, HI = 0.02, 0.02, 0.98
N_FEATURE_ROWS = 64         # the 256 feature columns are kept for the first rows only (file size)
HEADS = ('metallic_predictor', 'roughness_predictor', 'albedo_predictor')


def points():
    """Vertices of icosphere(3, 0.5) (642) followed by 382 seeded points in the unit ball: 1024 rows."""
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(3, 0.5)
    g = np.random.Generator(np.random.PCG64(4242))
    d = g.standard_normal((382, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ball = d * (g.random((382, 1)) ** (1.0 / 3.0)) * 0.95
    return np.concatenate([np.asarray(V, np.float32), ball.astype(np.float32)], 0), np.asarray(F, np.int32), len(V)


def spread_ok(res):
    for k, cols in (('metallic', 1), ('roughness', 1), ('albedo', 3)):
        a = res[k]
        assert a.shape[1] == cols and a.dtype == np.float32
        for c in range(cols):
            lo, hi = float(a[:, c].min()), float(a[:, c].max())
            assert hi - lo >= MIN_SPAN and lo >= LO and hi <= HI, (k, c, lo, hi)


def evaluate(sdf_net, color_net, x):
    with torch.no_grad():
        xt = torch.from_numpy(x)
        y = sdf_net(xt)
        m, r, a = color_net.predict_materials(xt, y[:, 1:])
    return {'feature': y[:N_FEATURE_ROWS, 1:].numpy(), 'sdf': y[:, 0].numpy(), 'metallic': m.numpy(), 'roughness': r.numpy(), 'albedo': a.numpy()}


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from network.renderer_zerothick import NeROShapeRenderer  # reference
    import network.field as rfield
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, randomize_for_parity

    x, F, nv = points()

    # ---- stage 1: the reference's renderer module ----
    cfg = {'name': 'golden', 'network': 'shape', 'database_name': 'nerf/spherepot', 'is_nerf': True}
    net = NeROShapeRenderer(cfg, training=False)
    params = randomize_for_parity(init_stage1_params(6033), seed=1)
    over = {}
    for h in HEADS:
        key = f'color_network.{h}.6.weight_g'
        over[key] = params[key] = (params[key] * HEAD_GAIN).astype(np.float32)
    net.load_state_dict(to_t(params), strict=True)
    res = evaluate(net.sdf_network, net.color_network, x)
    spread_ok(res)
    res.update(points=x, faces=F, n_mesh_vertices=np.asarray(nv), **{'override__' + k: v for k, v in over.items()})
    np.savez_compressed(os.path.join(OUT, 'materials_stage1.npz'), **res)
    print('stage1', {k: (float(res[k].min()), float(res[k].max())) for k in ('metallic', 'roughness', 'albedo')})

    # ---- stage 2, inner networks: the reference's SDFNetwork + AppShadingNetwork as its Stage2Renderer builds them
    # (renderer_zerothick.py:966-974), loaded with the inner entries of the stage-2 parity parameters ----
    p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    over = {}
    for h in HEADS:
        key = f'color_network_inner.{h}.6.weight_g'
        over[key] = p2[key] = (p2[key] * HEAD_GAIN).astype(np.float32)
    d = NeROShapeRenderer.default_cfg
    sdf_inner = rfield.SDFNetwork(d_out=d['sdf_d_out'], d_in=3, d_hidden=256, n_layers=d['sdf_n_layers'], skip_in=[d['sdf_n_layers'] // 2],
                                  multires=d['sdf_freq'], bias=d['sdf_bias'], scale=1.0, geometric_init=d['geometry_init'],
                                  weight_norm=True, sdf_activation=d['sdf_activation'])
    col_inner = rfield.AppShadingNetwork({'sphere_direction': False, 'human_light': False})
    sdf_inner.load_state_dict(to_t({k[len('sdf_network_inner.'):]: v for k, v in p2.items() if k.startswith('sdf_network_inner.')}), strict=True)
    col_inner.load_state_dict(to_t({k[len('color_network_inner.'):]: v for k, v in p2.items() if k.startswith('color_network_inner.')}),
                              strict=True)
    res = evaluate(sdf_inner, col_inner, x)
    spread_ok(res)
    res.update(points=x, faces=F, n_mesh_vertices=np.asarray(nv), **{'override__' + k: v for k, v in over.items()})
    np.savez_compressed(os.path.join(OUT, 'materials_stage2_inner.npz'), **res)
    print('stage2 inner', {k: (float(res[k].min()), float(res[k].max())) for k in ('metallic', 'roughness', 'albedo')})


if __name__ == '__main__':
    main()
