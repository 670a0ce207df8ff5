"""Relighting A/B: one 800 x 800 frame of an 81 920-face sphere at S in {64, 1024} through (a) the fused path -- nu_relight_visibility makes
each shadow ray in registers, nu_relight_resolve shades -- and (b) the composition that existed before it: the same rays written out as
[N,6], nu_lbvh_trace (closest hit, three result arrays), shading in torch.  Both share the G-buffer pass and work in sample chunks of
64 (the ray buffer of (b) is 24 bytes per ray).  GPU events, one warm-up then the median of --reps per variant, alternating order, one
process.  Prints ms per frame and shadow rays per second (every sample of every hit pixel counts, traced or not).

    python scripts/bench_relight.py [--size 800] [--samples 64 1024] [--reps 5]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402


def torch_shade(g, rays, bits, lit, env, S, s0, sc):
    """The resolve pass in torch for samples [s0, s0 + sc) of every pixel: g [P,20], rays [P*sc,6], lit [P*sc] -> sum [P,3]."""
    P = g.shape[0]
    l = rays[:, 3:].reshape(P, sc, 3)
    ns, v, alb, met = g[:, None, 7:10], g[:, None, 15:18], g[:, None, 10:13], g[:, None, 13:14]
    spec = (torch.arange(s0, s0 + sc, device=g.device) >= S // 2)[None, :, None]
    h = torch.nn.functional.normalize(l + v, dim=-1)
    a2 = torch.clamp(g[:, None, 14:15] ** 2, min=1e-3) ** 2
    nov = torch.clamp((ns * v).sum(-1, keepdim=True), min=1e-4)
    nol, noh, voh = (ns * l).sum(-1, keepdim=True), (ns * h).sum(-1, keepdim=True), (v * h).sum(-1, keepdim=True)
    g1 = lambda x: 2 * x / (x + torch.sqrt(a2 + (1 - a2) * x * x))    # noqa: E731
    f0 = 0.04 + (alb - 0.04) * met
    w_spec = (f0 + (1 - f0) * (1 - voh.clamp(max=1.0)) ** 5) * (g1(nol) * g1(nov) * voh / (nov * noh))
    w = torch.where(spec, w_spec, (1 - met) * alb)
    H, W = env.shape[:2]
    fx = (0.5 - torch.atan2(l[..., 1], l[..., 0]) / (2 * math.pi)) * W - 0.5
    fy = torch.atan2(torch.hypot(l[..., 0], l[..., 1]), l[..., 2]) / math.pi * H - 0.5
    x0, y0 = torch.floor(fx), torch.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    ix0 = torch.remainder(x0.long(), W)
    ix1 = torch.remainder(ix0 + 1, W)
    iy0, iy1 = y0.long().clamp(0, H - 1), (y0.long() + 1).clamp(0, H - 1)
    e = env[..., :3]
    rad = (1 - ay) * ((1 - ax) * e[iy0, ix0] + ax * e[iy0, ix1]) + ay * ((1 - ax) * e[iy1, ix0] + ax * e[iy1, ix1])
    return torch.where(lit.reshape(P, sc, 1), w * rad, torch.zeros_like(rad)).sum(1) * (2.0 / S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--samples', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--reps', type=int, default=5)
    flags = ap.parse_args()
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _cams

    dev = torch.device('cuda:0')
    V, F = icosphere(6, 0.5)
    mat = np.tile(np.array([0.8, 0.6, 0.4, 0.5, 0.4], np.float32), (len(V), 1))
    scene = R.Scene(V, F, mat, device=dev)
    h = w = flags.size
    g = np.random.Generator(np.random.PCG64(1))
    env = torch.from_numpy(R.pack_env(g.random((256, 512, 3)).astype(np.float32))).to(dev)
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    CH = 64

    def fused(S):
        face, gbuf = R.gbuffer(scene, cams, h, w)
        pix = R.hit_pixels(face)
        out = torch.zeros(h * w, 4, device=dev)
        for s0 in range(0, S, CH):
            vis = R.visibility(scene, gbuf, pix, S, s0, CH, 0)
            R.resolve(gbuf, pix, S, s0, CH, 0, env, vis, out)
        return out, int(pix.numel())

    def composed(S):
        face, gbuf = R.gbuffer(scene, cams, h, w)
        pix = R.hit_pixels(face)
        rows = gbuf.reshape(-1, R.ROW)[pix.long()]
        acc = torch.zeros(pix.numel(), 3, device=dev)
        for s0 in range(0, S, CH):
            rays, bits = R.shadow_rays(gbuf, pix, S, s0, CH, 0)
            hit, _ = scene.bvh.intersect(rays)
            acc += torch_shade(rows, rays, bits, (bits[:, 2] == 1) & (hit == 0), env, S, s0, CH)
        out = torch.zeros(h * w, 4, device=dev)
        out[pix.long(), :3] = acc
        out[pix.long(), 3] = 1.0
        return out, int(pix.numel())

    variants = [('fused (registers -> any hit -> resolve)', fused), ('composed ([N,6] -> nu_lbvh_trace -> torch)', composed)]
    for S in flags.samples:
        times = {n: [] for n, _ in variants}
        outs = {}
        for rep in range(flags.reps + 1):
            for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out, npix = fn(S)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
                outs[name] = out
        a, b = outs[variants[0][0]], outs[variants[1][0]]
        print(f"S={S}: {npix} hit pixels of {h * w}; max |fused - composed| = {float((a - b).abs().max()):.3e}")
        for name, _ in variants:
            ms = statistics.median(times[name])
            print(f"S={S:5d}  {name:44s} median {ms:9.2f} ms/frame (min {min(times[name]):9.2f}, max {max(times[name]):9.2f})  "
                  f"{npix * S / ms * 1e3 / 1e9:7.3f} G shadow rays/s", flush=True)


if __name__ == '__main__':
    main()
