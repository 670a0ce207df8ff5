"""ms/step of a real-capture stage-1 training step with shader_config.human_light off and on.

    python scripts/bench_human_light.py [--rays 4096] [--steps 30] [--warmup 8] [--repeats 3]

The step is bench.py's (forward, fused loss kernels, backward, HIP Adam) on rays built from camera poses -- the key needs the
cameras' human frames, so the batch is {'dirs', 'idxs', 'rgbs'} + poses instead of bench.py's synthetic world-space rays; 64 / 64 / 32
samples per ray (160).  Three legs: key off, key off with the shading stack sequenced launch by launch (engine.py_seq, the sequencing
the key-on path uses), key on.  Each leg is timed `repeats` times, interleaved, every timing the median over `steps` steps of the wall
time between device synchronisations; the result gives the median of the repeats and the repeats themselves.  off_pyseq - off is what
the sequencing costs, on - off_pyseq what the fifth stack and the new kernels cost.  The yardstick beside it: forward + backward of one
existing 256-wide light predictor (refrac_light) and of the new one over the step's P inner rows, timed alone with device events.
One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cameras(n, seed, dist=2.2):
    """n world-to-camera poses looking at the origin from `dist` (the layout of tests/human_light_oracle.camera_poses)."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        az, el = 2 * np.pi * (i + 0.3 * g.random()) / n, 0.25 + 0.3 * g.random()
        c = dist * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        zc = -c / np.linalg.norm(c)
        xc = np.cross(zc, np.array([0.0, 0.0, 1.0]))
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc], 0)
        out.append(np.concatenate([R, (-R @ c)[:, None]], 1))
    return np.asarray(out, np.float32)


def build(key, rays, dev):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params
    cfg = {'name': 'bench_hl', 'network': 'shape', 'database_name': 'custom/x', 'is_nerf': False, 'apply_occ_loss': True,
           'occ_loss_step': 15000, 'freeze_inv_s_step': 15000, 'eikonal_weight': 0.1, 'train_ray_num': rays,
           'n_samples': 64, 'n_importance': 64, 'n_bg_samples': 32, 'up_sample_steps': 4,
           'shader_config': {'sphere_direction': True, 'human_light': key, 'light_exp_max': 5.0}}
    torch.manual_seed(6033)
    net = NeROShapeRenderer(cfg, training=False)
    net.load_param_dict(init_stage1_params(6033, sphere_direction=True, human_light=key))
    return net.to(dev), cfg


def stack_alone(net, P, dev, repeats=7):
    """ms of forward + backward (input and weight gradients) of one predictor stack over P rows, alone on the device."""
    from nu_nerf_amd.nets import Stage1Nets
    eng = net.engine()
    eng.pack()
    nets = Stage1Nets(eng, net._named())
    out = {}
    for name in ('refrac_light', 'human_light_predictor'):
        layers = nets.stack[name][0]
        X = torch.randn(P, layers[0].Kp, device=dev)
        ts = []
        for i in range(repeats + 2):
            nets.begin_pass()
            x = X.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = nets.predictor(name, x)
            y.sum().backward()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        net.zero_grad(set_to_none=True)
        out[f'stack_alone_ms_{name}'] = round(float(np.median(ts)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--legs', default='off,off_pyseq,on', help='which legs to run (a kernel trace of one leg alone)')
    args = ap.parse_args()
    from nu_nerf_amd.loss import name2loss, fused_stage1_loss
    from nu_nerf_amd.train_glue import FusedAdam
    dev = torch.device('cuda:0')
    R, n_img = args.rays, 8
    g = torch.Generator().manual_seed(6033)
    poses = torch.from_numpy(cameras(n_img, 11)).to(dev)
    pool = {'dirs': torch.cat([0.5 * torch.rand(16 * R, 2, generator=g) - 0.25, torch.ones(16 * R, 1)], 1).to(dev),
            'idxs': torch.randint(0, n_img, (16 * R, 1), generator=g).to(dev), 'rgbs': torch.rand(16 * R, 3, generator=g).to(dev)}
    legs = {}
    want = set(args.legs.split(','))
    for key in [k for k, t in ((False, 'off'), ('pyseq', 'off_pyseq'), (True, 'on')) if t in want]:
        net, cfg = build(key is True, R, dev)
        if key == 'pyseq':
            net.engine().py_seq = True
        losses = [name2loss[n](cfg) for n in ('nerf_render', 'eikonal', 'std', 'init_sdf_reg', 'occ', 'outer_reg')]
        legs[key] = dict(net=net, losses=losses, opt=FusedAdam(net.parameters(), lr=1e-3), times=[], P_in=0, n=0)

    def step(leg, it):
        b = {k: v[(it % 16) * R:(it % 16 + 1) * R] for k, v in pool.items()}
        leg['opt'].zero_grad(set_to_none=True)
        total, _, _ = fused_stage1_loss(leg['net'], b, 20000 + it, leg['losses'], poses=poses)
        total.backward()
        leg['opt'].step()
        return leg['net'].engine().last_ctx['P_in']

    for key in legs:
        for it in range(args.warmup):
            step(legs[key], it)
    torch.cuda.synchronize()
    for rep in range(args.repeats):
        for key in legs:
            leg, ts = legs[key], []
            for it in range(args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p_in = step(leg, args.warmup + it)
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
                leg['P_in'] += p_in
                leg['n'] += 1
            leg['times'].append(float(np.median(ts)))
    res = {'rays': R, 'samples_per_ray': 160, 'steps': args.steps, 'repeats': args.repeats}
    for key in legs:
        leg = legs[key]
        tag = {False: 'off', 'pyseq': 'off_pyseq', True: 'on'}[key]
        res[f'ms_per_step_{tag}'] = round(float(np.median(leg['times'])), 3)
        res[f'ms_per_step_{tag}_repeats'] = [round(t, 3) for t in leg['times']]
        res[f'inner_points_per_step_{tag}'] = leg['P_in'] // max(leg['n'], 1)
    if len(legs) == 3:
        res['on_minus_off_ms'] = round(res['ms_per_step_on'] - res['ms_per_step_off'], 3)
        res['sequencing_ms'] = round(res['ms_per_step_off_pyseq'] - res['ms_per_step_off'], 3)
        res['stack_and_kernels_ms'] = round(res['ms_per_step_on'] - res['ms_per_step_off_pyseq'], 3)
        res.update(stack_alone(legs[True]['net'], res['inner_points_per_step_on'], dev))
    # rows through 256-wide predictor stacks per step: outer_light 3P + R, inner_light 2P, inner_weight P, refrac_light P; the key adds P
    P = res[[k for k in res if k.startswith('inner_points_per_step')][0]]
    res['predictor_rows_off'] = 7 * P + R
    res['predictor_rows_added'] = P
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
