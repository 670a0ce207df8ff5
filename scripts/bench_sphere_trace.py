"""Sphere tracing A/B: (a) the fused kernel (csrc/sdf_trace.hip: the whole march of a frame in one launch) against (b) the composition a
user could build without it -- per iteration a `nonzero` compaction of the live rays, sdf_forward(keep=False, want_feat=False) on them and
the update in torch, which returns the same bits -- and (c) nu_sdf_fused_fwd on as many points as the frame has rays: the ceiling of
useful SDF evaluations per second, since the trace cannot beat the forward it wraps.
Workload: the 800 x 800 rays of frame 0 of relight.relighting_poses (relight.intrinsics), bounding radius 1, threshold 1e-5, 200 iterations,
on the initialised and on the parity network.  GPU events around each call (the composition ends in a synchronise of its own), warm-up
first, median of --reps with min and max, the variants run in alternating order on one device.
Also prints, from the iteration counts alone, how the kernel's static schedule spends its passes: a pass is one evaluation of the network on
a workgroup's 64 slots; `slot use` is the share of slot-passes that carried a live ray, `tail` the passes of the busiest workgroup over the
mean (the launch lasts as long as that workgroup).

    python scripts/bench_sphere_trace.py [--hw 800] [--reps 10] [--networks init parity]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402

TM, GRID = 64, 256            # ray slots per workgroup and the largest grid of sdf_trace_kernel


def schedule(iters, tm=TM, grid=GRID, run=1):
    """(passes per workgroup [G], live slot-passes) of the kernel's static schedule for the evaluation counts iters [R]: workgroup b of G
    takes the runs b, b + G, .. of `run` consecutive rays (the kernel: run = 1, ray q G + b is the q-th of workgroup b); a ray with
    iters == 0 never occupies a slot; free slots are refilled in slot order."""
    R = len(iters)
    G = min((R + tm - 1) // tm, grid)
    pad = np.zeros(-(-R // (G * run)) * G * run, np.int64)
    pad[:R] = iters
    seq = pad.reshape(-1, G, run).transpose(1, 0, 2).reshape(G, -1)                     # [G, rays of the workgroup, in order]
    queues = np.zeros_like(seq)
    for b in range(G):
        q = seq[b][seq[b] > 0]
        queues[b, :len(q)] = q
    qlen = (queues > 0).sum(1)
    cursor = np.zeros(G, np.int64)
    left = np.zeros((G, tm), np.int64)
    passes = np.zeros(G, np.int64)
    while True:
        free = left == 0
        rank = np.cumsum(free, 1) - 1
        src = cursor[:, None] + rank
        take = free & (src < qlen[:, None])
        left[take] = queues[np.nonzero(take)[0], src[take]]
        cursor += take.sum(1)
        busy = (left > 0).any(1)
        if not busy.any():
            break
        passes += busy
        left[left > 0] -= 1
    return passes, int(np.sum(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=800)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--networks', nargs='+', default=['init', 'parity'], choices=['init', 'parity'])
    flags = ap.parse_args()
    from nu_nerf_amd import relight
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.mask_render import pinhole_rays
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.sdf_trace import trace_rays

    dev = torch.device('cuda:0')
    h = w = flags.hw
    K = torch.as_tensor(relight.intrinsics(h, w), dtype=torch.float32)
    pose = torch.as_tensor(relight.relighting_poses(8, 0.0, 45.0, 3.0)[0], dtype=torch.float32)[None]
    rays = pinhole_rays(K, pose, h, w, dev)
    o, d = rays[:, :3].contiguous(), rays[:, 3:].contiguous()
    R = o.shape[0]
    thr, rb = torch.tensor(1e-5, device=dev), torch.tensor(1.0, device=dev)

    for name in flags.networks:
        arrays = init_stage1_params(6033)
        if name == 'parity':
            arrays = randomize_for_parity(arrays, seed=1)
        net = NeROShapeRenderer({'name': 'golden'}, training=False)
        net.load_param_dict(arrays)
        net = net.to(dev)
        eng = net.engine()
        eng.pack()

        def kernel():
            return trace_rays(net, o, d, entry_forward=True)

        def forward_only():
            sdf = torch.empty(R, device=dev)
            eng.lib.nu_sdf_fused_fwd(ctypes.byref(eng._sdf_net), addr(o), 3, R, addr(sdf), eng.stream())
            return {'sdf': sdf}

        def composition():
            # entry (torch, the stated order), then per iteration: compaction, forward on the live rays, update, scatter
            dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]      # noqa: E731
            a, b, c = dot(d, d), 2 * dot(d, o), dot(o, o) - rb * rb
            disc = b * b - (4 * a) * c
            bounded = disc >= 0
            t0 = torch.clamp((-b - torch.sqrt(disc)) / (2 * a), min=0)
            fgr = torch.isfinite(o).all(1) & bounded
            x = torch.where(fgr[:, None], o + d * t0[:, None], o)
            t = torch.where(fgr, t0, torch.zeros_like(t0))
            iters = torch.zeros(R, dtype=torch.int32, device=dev)
            last = torch.zeros(R, device=dev)
            hit = torch.zeros(R, dtype=torch.uint8, device=dev)
            idx = fgr.nonzero().reshape(-1)
            for i in range(200):
                if idx.numel() == 0:
                    break
                xl, dl = x[idx], d[idx]
                s = eng.sdf_forward(addr(xl), 3, xl.shape[0], keep=False, want_feat=False)['sdf']
                s = torch.nan_to_num(torch.clamp(s, -10.0, 10.0), nan=10.0)
                xn = xl + dl * s[:, None]
                q = xn * xn
                inside = torch.sqrt((q[:, 0] + q[:, 1]) + q[:, 2]) < rb
                conv = s.abs() < thr
                x[idx], t[idx], last[idx] = xn, t[idx] + s, s
                iters[idx] = i + 1
                hit[idx] = (conv & inside).to(torch.uint8)
                idx = idx[inside & ~conv]
            return {'pos': x, 't': t, 'sdf': last, 'iters': iters, 'hit': hit}

        variants = [('nu_sdf_trace', kernel), ('composition (nonzero + sdf_forward + torch)', composition), ('nu_sdf_fused_fwd', forward_only)]
        times = {n: [] for n, _ in variants}
        outs = {}
        for rep in range(flags.reps + 2):                            # reps 0 and 1: warm-up (allocator, code objects)
            order = variants if rep % 2 == 0 else variants[::-1]
            for vname, fn in order:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[vname].append(e0.elapsed_time(e1))
                outs[vname] = out
        got, comp = outs['nu_sdf_trace'], outs[variants[1][0]]
        equal = {k: bool(torch.equal(got[k], comp[k])) for k in ('pos', 't', 'sdf', 'iters', 'hit')}
        it = got['iters'].cpu().numpy().astype(np.int64)
        n_eval, traced, n_hit = int(it.sum()), int((it > 0).sum()), int(got['hit'].sum())
        med = {n: statistics.median(v) for n, v in times.items()}
        print(f"[{name}] {h} x {w} = {R} rays: {traced} enter the sphere, {n_hit} hit, {n_eval} SDF evaluations "
              f"(per traced ray: mean {n_eval / max(traced, 1):.1f}, max {int(it.max())}); kernel == composition bits: {equal}")
        for vname, _ in variants:
            v = times[vname]
            print(f"[{name}] {vname:46s} median {med[vname]:9.3f} ms  (min {min(v):9.3f}, max {max(v):9.3f}, n {len(v)})")
        fwd_rate = R / med['nu_sdf_fused_fwd'] * 1e3
        for vname in (variants[0][0], variants[1][0]):
            rate = n_eval / med[vname] * 1e3
            print(f"[{name}] {vname:46s} {rate / 1e6:8.2f} M useful evaluations/s = {rate / fwd_rate:5.3f} of nu_sdf_fused_fwd at {R} points "
                  f"({fwd_rate / 1e6:.2f} Mpoints/s)")
        print(f"[{name}] kernel / composition = {med[variants[0][0]] / med[variants[1][0]]:.3f}")
        passes, live = schedule(it)
        print(f"[{name}] static schedule, {len(passes)} workgroups x {TM} slots: passes per workgroup mean {passes.mean():.1f} max {int(passes.max())}"
              f" (tail {passes.max() / max(passes.mean(), 1e-9):.2f}), slot use {live / max(TM * int(passes.sum()), 1):.3f}; "
              f"the launch's {int(passes.max())} passes of 64 = {TM * int(passes.max()) * len(passes)} slot-evaluations for {live} useful "
              f"({live / max(TM * int(passes.max()) * len(passes), 1):.3f}); kernel time per pass {med['nu_sdf_trace'] / max(int(passes.max()), 1) * 1e3:.1f} us, "
              f"fused forward per 64-row tile and CU {med['nu_sdf_fused_fwd'] / max(-(-R // TM) / GRID, 1e-9) * 1e3:.1f} us")


if __name__ == '__main__':
    main()
