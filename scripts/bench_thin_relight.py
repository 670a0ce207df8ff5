"""Thin-shell relighting against the solid shell: one 800 x 800 frame of the 81 920-face sphere around the 20 480-face inner
sphere of scripts/bench_nested_relight.py, S in {64, 1024}, through (a) the thin shell -- ThinShellScene, index 1.5, wall 0.005:
nu_relight_thin_chain / nu_relight_thin_light -- and (b) the solid glass shell of DESIGN.md 21 on the same meshes -- NestedScene,
index 1.5: nu_relight_nested_chain / nu_relight_nested_light, kernels this change leaves as they were.  Both end in
nu_relight_nested_resolve and work in sample chunks of 64.  Each variant's passes before the light paths (outer G-buffer, chain,
reflection / exit terms) are also timed alone and subtracted for the rate.  GPU events, one warm-up then the median of --reps per
variant, alternating order, one process.  Prints ms per frame and light paths per second (every sample of every inner pixel counts,
traced or not).  The two pictures differ by design (another shell); the pixel counts are printed.

    python scripts/bench_thin_relight.py [--size 800] [--samples 64 1024] [--reps 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch   # noqa: E402


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
    Vo, Fo = icosphere(6, 0.5)
    Vi, Fi = icosphere(5, 0.2)
    Vi = (Vi + np.array([0.1, 0.0, 0.05], np.float32)).astype(np.float32)
    mat = np.tile(np.array([0.8, 0.6, 0.4, 0.5, 0.4], np.float32), (len(Vi), 1))
    scenes = {'thin': R.ThinShellScene(Vo, Fo, 1.5, 0.005, Vi, Fi, mat, device=dev), 'solid': R.NestedScene(Vo, Fo, 1.5, Vi, Fi, mat, device=dev)}
    h = w = flags.size
    g = np.random.Generator(np.random.PCG64(1))
    env = torch.from_numpy(R.pack_env(g.random((256, 512, 3)).astype(np.float32))).to(dev)
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    CH = 64

    def frame(which, S, light):
        sc_ = scenes[which]
        face, gbuf = R.gbuffer(sc_.outer, cams, h, w)
        pix = R.hit_pixels(face)
        kind, chain, irow = R.thin_chain(sc_, gbuf, pix) if which == 'thin' else R.nested_chain(sc_, gbuf, pix)
        sel = (kind == R.INNER).nonzero().flatten().to(torch.int32)
        other = (kind != R.INNER).nonzero().flatten().to(torch.int32)
        out = torch.zeros(h * w, 4, device=dev)
        R.nested_resolve(irow, chain, kind, pix, other, 2, 0, 0, 0, env, None, True, out)
        if light:
            trace = R.thin_light if which == 'thin' else R.nested_light
            for s0 in range(0, S, CH):
                sc = min(CH, S - s0)
                rec = trace(sc_, irow, sel, S, s0, sc, 0)
                R.nested_resolve(irow, chain, kind, pix, sel, S, s0, sc, 0, env, rec, s0 + sc == S, out)
        return out, (int(sel.numel()), int((kind == R.EXIT).sum()), int((kind == R.DARK).sum()))

    variants = [(f'{which} shell, {"frame" if light else "passes before the light paths"}', which, light)
                for light in (True, False) for which in ('thin', 'solid')]
    for S in flags.samples:
        times = {n: [] for n, _, _ in variants}
        counts = {}
        for rep in range(flags.reps + 1):
            for name, which, light in (variants if rep % 2 == 0 else variants[::-1]):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out, counts[which] = frame(which, S, light)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        for which in ('thin', 'solid'):
            print(f"S={S}: {which} shell: inner / exit / dark pixels {counts[which]} of {h * w}")
        for name, which, light in variants:
            ms = statistics.median(times[name])
            rate = ""
            if light:
                base_name = [n for n, w2, l2 in variants if w2 == which and not l2][0]
                base = statistics.median(times[base_name])
                spread = max(times[base_name]) - min(times[base_name])
                rate = (f"{counts[which][0] * S / (ms - base) * 1e3 / 1e9:7.3f} G light paths/s beyond the earlier passes" if ms - base > max(spread, 1e-3)
                        else "(within the spread of the earlier passes: no rate)")
            print(f"S={S:5d}  {name:50s} median {ms:9.2f} ms/frame (min {min(times[name]):9.2f}, max {max(times[name]):9.2f})  {rate}", flush=True)


if __name__ == '__main__':
    main()
