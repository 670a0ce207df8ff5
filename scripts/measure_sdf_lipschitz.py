"""max |grad f| of the SDF network over uniform points of the unit ball (the Lipschitz bound of the block-sparse mesh
extraction is a default, not a derived number; this is the measurement behind it).

    python3 scripts/measure_sdf_lipschitz.py [--points 4194304] [--seed 0]

Networks: the init network (init_stage1_params(6033)) and the parity network of tests/test_mesh_gpu.py (randomize_for_parity(seed=1)
with the overrides of tests/golden/eval_step20000_r40.npz).  The gradient comes from the first-order jet kernel nu_sdf_grad_fwd
(Engine.sdf_grad).  Prints one JSON line per network: max, 99.9 % and mean of |grad f| and the largest |f| seen."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {'name': 'golden', 'network': 'shape', 'database_name': 'synthetic/64', 'apply_occ_loss': True, 'occ_loss_step': 15000,
       'is_nerf': True, 'freeze_inv_s_step': 15000, 'n_samples': 32, 'n_importance': 32, 'n_bg_samples': 16}


def networks(dev):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    init = NeROShapeRenderer(dict(CFG), training=False)
    init.load_param_dict(init_stage1_params(6033))
    yield 'init', init.to(dev)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'eval_step20000_r40.npz'))
    params = randomize_for_parity(init_stage1_params(6033), seed=1)
    for k in g.files:
        if k.startswith('override__'):
            params[k[len('override__'):]] = g[k]
    parity = NeROShapeRenderer(dict(CFG), training=False)
    parity.load_param_dict(params)
    yield 'parity', parity.to(dev)


@torch.no_grad()
def measure(net, n, seed, dev, chunk=1 << 18):
    from nu_nerf_amd.engine import addr
    eng = net.engine()
    eng.pack()
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0) * 0.9999
    x = d.float().to(dev).contiguous()
    norms, vals = [], []
    for c0 in range(0, n, chunk):
        xc = x[c0:c0 + chunk].contiguous()
        P = xc.shape[0]
        sdf = torch.empty(P, device=dev)
        grad = torch.empty(P, 3, device=dev)
        eng.sdf_grad(addr(xc), 3, P, sdf=sdf, grad=grad)
        norms.append(grad.double().norm(dim=1))
        vals.append(sdf.abs().max())
    gn = torch.cat(norms)
    return dict(points=n, max_grad=float(gn.max()), p999_grad=float(torch.quantile(gn[:: max(1, n // 1_000_000)], 0.999)),
                mean_grad=float(gn.mean()), max_abs_f=float(torch.stack(vals).max()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument('--points', type=int, default=1 << 22)
    ap.add_argument('--seed', type=int, default=0)
    flags = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    for name, net in networks(dev):
        print(json.dumps(dict(network=name, **measure(net, flags.points, flags.seed, dev))), flush=True)


if __name__ == "__main__":
    main()
