"""Split-sum relighting timings.

  prefilter  the default 256 x 512 map to 5 levels plus the diffuse map at the source's size (the four regressed GGX levels and the
             cosine lobe in ONE nu_env_prefilter call; level 0 is the bilinear tap) against the torch composition of the same sums:
             chunks of f(Dq Ds^T) [chunk, M] per lobe, then a matmul with [w rgb | w].  Pair evaluations per second = queries x source
             points x lobes / time.
  relight    one 800 x 800 frame of the 81 920-face sphere: G-buffer pass + split-sum resolve against the Monte-Carlo path at S = 64
             and S = 1024 (sample chunks of 64, as scripts/bench_relight.py), and the split of the split-sum frame between its two passes.

GPU events, one warm-up then the median of --reps per variant, variants alternating, one process.

    python scripts/bench_splitsum.py [--height 256 --width 512] [--size 800] [--samples 64 1024] [--reps 5] [--torch-chunk 2048]
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


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(variants, reps):
    """{name: [ms]} and the last outputs; repetition 0 is the warm-up, the order flips every repetition."""
    times, outs = {n: [] for n, _ in variants}, {}
    for rep in range(reps + 1):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms, outs[name] = timed(fn)
            if rep:
                times[name].append(ms)
    return times, outs


def line(name, t):
    return f"{name:58s} median {statistics.median(t):9.3f} ms (min {min(t):9.3f}, max {max(t):9.3f})"


def torch_prefilter(sd, rgb, dirs, lobes, chunk):
    """The same sums in torch: per chunk of queries c = Dq Ds^T, per lobe f(c) @ [w rgb | w]."""
    from nu_nerf_amd.environment import lobe_param
    wrgb = torch.cat([sd[:, 3:] * rgb[:, :3], sd[:, 3:]], 1)
    out = torch.empty(len(lobes), dirs.shape[0], 3, device=dirs.device)
    for i0 in range(0, dirs.shape[0], chunk):
        c = dirs[i0:i0 + chunk] @ sd[:, :3].t()
        for l, x in enumerate(lobes):
            kind, rho = (x, None) if isinstance(x, str) else x
            p = lobe_param(kind, rho)
            if kind == 'cosine':
                f = c.clamp_min(0.0)
            elif kind == 'ggx':
                a2 = p * p
                f = c.clamp_min(0.0) * (a2 / math.pi) / (a2 + (1.0 - a2) * 0.5 * (1.0 - c)) ** 2
            else:
                f = torch.exp(p * (c - 1.0))
            s = f @ wrgb
            out[l, i0:i0 + chunk] = s[:, :3] / s[:, 3:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--samples', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-chunk', type=int, default=2048, help="queries per chunk of the torch composition ([chunk, M] floats per lobe)")
    flags = ap.parse_args()
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.environment import DEFAULT_LEVELS, latlong_dirs, lobe_is_tapped, prefilter, prefilter_dirs, source_table
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _cams

    dev = torch.device('cuda:0')
    g = np.random.Generator(np.random.PCG64(1))
    H, W = flags.height, flags.width
    env = (g.random((H, W, 3)) * np.exp2(g.uniform(-3, 3, (H, W, 1)))).astype(np.float32)

    # ---- prefilter -------------------------------------------------------------------------------------------------------------
    sd_np, rgb_np = source_table(env)
    sd, rgb, dirs = torch.from_numpy(sd_np).to(dev), torch.from_numpy(rgb_np).to(dev), torch.from_numpy(latlong_dirs(H, W)).to(dev)
    lobes = [('ggx', r) for r in DEFAULT_LEVELS if not lobe_is_tapped('ggx', r, H)] + ['cosine']
    pairs = dirs.shape[0] * sd.shape[0] * len(lobes)
    variants = [('nu_env_prefilter (one launch, %d lobes)' % len(lobes), lambda: prefilter_dirs((sd, rgb), dirs, lobes, device=dev)[..., :3]),
                ('torch: f(Dq Ds^T) @ [w rgb | w], chunks of %d' % flags.torch_chunk, lambda: torch_prefilter(sd, rgb, dirs, lobes, flags.torch_chunk))]
    times, outs = alternate(variants, flags.reps)
    a, b = outs[variants[0][0]], outs[variants[1][0]]
    print(f"prefilter {H} x {W} -> {H} x {W}, lobes {lobes}: {dirs.shape[0]} queries x {sd.shape[0]} source points x {len(lobes)} lobes = "
          f"{pairs:.3e} pair evaluations; max relative |kernel - torch| = {float(((a - b).abs() / b.abs().clamp_min(1e-2)).max()):.3e}")
    for name, _ in variants:
        ms = statistics.median(times[name])
        print(f"{line(name, times[name])}  {pairs / ms * 1e3 / 1e9:8.1f} G pair evaluations/s", flush=True)
    ms, _ = timed(lambda: prefilter(env, DEFAULT_LEVELS, device=dev))
    print(f"environment.prefilter end to end (host table, upload, launch, tap, download): {ms:.1f} ms")

    # ---- relight ---------------------------------------------------------------------------------------------------------------
    pyramid, diffuse, _ = prefilter(env, DEFAULT_LEVELS, 64, 128, device=dev)
    levels = np.asarray(DEFAULT_LEVELS, np.float32)
    V, F = icosphere(6, 0.5)
    mat = np.tile(np.array([0.8, 0.6, 0.4, 0.5, 0.4], np.float32), (len(V), 1))
    scene = R.Scene(V, F, mat, device=dev)
    h = w = flags.size
    envd = torch.from_numpy(R.pack_env(env)).to(dev)
    packed, lv = R.pack_pyramid(pyramid, levels)
    pyr, dif = torch.from_numpy(packed).to(dev), torch.from_numpy(R.pack_env(diffuse)).to(dev)
    R.fg_table(dev)
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    CH = 64

    def splitsum():
        face, gbuf = R.gbuffer(scene, cams, h, w)
        out = torch.zeros(h * w, 4, device=dev)
        return R.splitsum_resolve(gbuf, R.hit_pixels(face), pyr, lv, dif, out)

    def monte_carlo(S):
        face, gbuf = R.gbuffer(scene, cams, h, w)
        pix = R.hit_pixels(face)
        out = torch.zeros(h * w, 4, device=dev)
        for s0 in range(0, S, CH):
            R.resolve(gbuf, pix, S, s0, CH, 0, envd, R.visibility(scene, gbuf, pix, S, s0, CH, 0), out)
        return out

    variants = [('split-sum (G-buffer + nu_relight_splitsum)', splitsum)] + [('Monte-Carlo S = %d' % S, lambda S=S: monte_carlo(S)) for S in flags.samples]
    times, outs = alternate(variants, flags.reps)
    face, gbuf = R.gbuffer(scene, cams, h, w)
    pix = R.hit_pixels(face)
    print(f"relight {h} x {w}, {len(F)} faces, {int(pix.numel())} hit pixels")
    for name, _ in variants:
        print(line(name, times[name]), flush=True)
    out = torch.zeros(h * w, 4, device=dev)
    parts = [('  G-buffer pass (nu_relight_gbuffer)', lambda: R.gbuffer(scene, cams, h, w)),
             ('  hit list (torch nonzero, one host read)', lambda: R.hit_pixels(face)),
             ('  resolve (nu_relight_splitsum)', lambda: R.splitsum_resolve(gbuf, pix, pyr, lv, dif, out))]
    times, _ = alternate(parts, flags.reps)
    for name, _ in parts:
        print(line(name, times[name]), flush=True)
    frame = statistics.median(alternate(variants[:1], flags.reps)[0][variants[0][0]])
    print(f"360-frame orbit at this frame time: {360 * frame / 1e3:.2f} s of kernels")


if __name__ == '__main__':
    main()
