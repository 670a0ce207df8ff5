"""tests/golden/sphere_trace.npz from the REFERENCE itself (build container only; shims and conventions of oracle/gen_golden.py).

The reference's own sphere_tracing (network/tracing.py) around its own SDFNetwork (network/field.py), in float64, called ONE RAY PER
CALL -- its whole-batch `break` makes a ray's result depend on the batch it is in; a lone ray has no such dependence, and that is the
semantics of csrc/sdf_trace.hip -- on the first 256 rays of the standard ray set (tests/sphere_trace_oracle.py) and two networks: the
initialised stage-1 SDF (init_stage1_params(6033)) and the parity network (randomize_for_parity(seed=1)), bounding radius 1, 200
iterations, threshold 1e-5.  Only inputs and outputs are stored: rays_o, rays_d [256,3] float32; pos_init, pos_parity [256,3] float64;
hit_init, hit_parity [256] bool.  Tests rebuild the weights from the same seeds.

Usage:  python scripts/gen_golden_sphere_trace.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle.gen_golden import install_shims, OUT   # noqa: E402

N = 256


def reference_sdf(arrays):
    from network.field import SDFNetwork  # reference
    net = SDFNetwork(d_out=257, d_in=3, d_hidden=256, n_layers=8, skip_in=[4], multires=6, bias=0.5, scale=1.0, geometric_init=True,
                     weight_norm=True)
    state = {k[len('sdf_network.'):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in arrays.items() if k.startswith('sdf_network.')}
    print("load_state_dict:", net.load_state_dict(state, strict=True))
    return net.double()


def run(net, o, d):
    from network.tracing import sphere_tracing  # reference
    pos, hit = np.zeros((len(o), 3)), np.zeros(len(o), bool)
    with torch.no_grad():
        for i in range(len(o)):
            p, h = sphere_tracing(net.sdf, torch.from_numpy(o[i:i + 1]).double(), torch.from_numpy(d[i:i + 1]).double(), 200, 1e-5, None, 1.0)
            pos[i], hit[i] = p[0].numpy(), bool(h[0, 0])
    return pos, hit


def main():
    from sphere_trace_oracle import standard_rays
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    o, d = standard_rays()
    o, d = o[:N], d[:N]
    install_shims()
    res = {'rays_o': o, 'rays_d': d}
    for name, arrays in (('init', init_stage1_params(6033)), ('parity', randomize_for_parity(init_stage1_params(6033), seed=1))):
        pos, hit = run(reference_sdf(arrays), o, d)
        res['pos_' + name], res['hit_' + name] = pos, hit
        moved = np.abs(pos - o).max(1) > 0
        print(f"{name}: {int(hit.sum())} of {N} rays hit, {int(moved.sum())} moved")
    path = os.path.join(OUT, 'sphere_trace.npz')
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
