"""Nested-object relighting A/B: one 800 x 800 frame, the 81 920-face sphere as outer shell (ior 1.5), a 20 480-face inner
sphere, S in {64, 1024}, through (a) the fused path -- nu_relight_nested_light walks the three dependent rays of every sample in
registers, nu_relight_nested_resolve shades -- and (b) the composition of what existed before it: the sample rays written out as
[N,6] (nu_relight_shadow_rays on the inner rows), THREE nu_lbvh_trace calls per sample chunk (inner, outer, outer along the exit
ray) with the surface attributes, the interface event and the shading in torch.  Both share the outer G-buffer pass and the interior
chain (nu_relight_nested_chain, timed on its own as well) and work in sample chunks of 64.  GPU events, one warm-up then the median of
--reps per variant, alternating order, one process.  Prints ms per frame, light paths per second (every sample of every inner pixel
counts, traced or not; a path is up to three walks) and the agreement of the two images.

    python scripts/bench_nested_relight.py [--size 800] [--samples 64 1024] [--reps 5]
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

MISS = 10000000


def dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def torch_leave(V, F, VN, ior, o, d, idx, eps):
    """nu_rln_leave in torch for rays (o, d) [N,3] that met face idx [N] of the outer mesh from inside ->
    (refracts [N] bool, exit origin [N,3], exit direction [N,3], 1 - F_exit [N,1])."""
    f = F[idx.long()].long()
    v0, v1, v2 = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    pv = torch.linalg.cross(d, e2)
    inv = 1.0 / dot(e1, pv)
    tv = o - v0
    u = dot(tv, pv) * inv
    qv = torch.linalg.cross(tv, e1)
    v = dot(d, qv) * inv
    t = dot(e2, qv) * inv
    w0 = 1.0 - u - v
    ng = torch.nn.functional.normalize(torch.linalg.cross(e1, e2), dim=-1)
    ng = torch.where(dot(ng, d) > 0, -ng, ng)
    ns = torch.nn.functional.normalize(w0 * VN[f[:, 0]] + u * VN[f[:, 1]] + v * VN[f[:, 2]], dim=-1)
    ns = torch.where(dot(ns, ng) < 0, -ns, ns)
    index = 1.0 + (w0 * (ior[f[:, 0], None] - 1.0) + u * (ior[f[:, 1], None] - 1.0) + v * (ior[f[:, 2], None] - 1.0))
    n = torch.where(dot(ns, d) > 0, -ns, ns)
    cos_i = -dot(n, d)
    k2 = index * index * (1.0 - cos_i * cos_i)
    refr = ~(k2 > 0.999)
    cos_t = torch.sqrt((1.0 - k2).clamp(min=0.0))
    dn = torch.nn.functional.normalize(index * d + (index * cos_i - cos_t) * n, dim=-1)
    f0 = ((index - 1.0) / (index + 1.0)) ** 2
    fres = torch.where(f0 > 0, f0 + (1.0 - f0) * (1.0 - cos_t).clamp(min=0.0) ** 5, torch.zeros_like(f0))
    x = o + t * d
    return refr[:, 0], x - eps * ng, dn, 1.0 - fres


def torch_shade(g, l, dout, keep, lit, env, S, s0, sc):
    """The nested resolve in torch for samples [s0, s0 + sc) of every inner pixel: g [P,20], sample directions l, exit directions dout
    [P*sc,3], keep [P*sc,1], lit [P*sc] -> sum [P,3] (without T)."""
    P = g.shape[0]
    l, dout = l.reshape(P, sc, 3), dout.reshape(P, sc, 3)
    ns, v, alb, met = g[:, None, 7:10], g[:, None, 15:18], g[:, None, 10:13], g[:, None, 13:14]
    spec = (torch.arange(s0, s0 + sc, device=g.device) >= S // 2)[None, :, None]
    h = torch.nn.functional.normalize(l + v, dim=-1)
    a2 = torch.clamp(g[:, None, 14:15] ** 2, min=1e-3) ** 2
    nov = torch.clamp((ns * v).sum(-1, keepdim=True), min=1e-4)
    nol, noh, voh = (ns * l).sum(-1, keepdim=True), (ns * h).sum(-1, keepdim=True), (v * h).sum(-1, keepdim=True)
    g1 = lambda x: 2 * x / (x + torch.sqrt(a2 + (1 - a2) * x * x))    # noqa: E731
    f0 = 0.04 + (alb - 0.04) * met
    w_spec = (f0 + (1 - f0) * (1 - voh.clamp(max=1.0)) ** 5) * (g1(nol) * g1(nov) * voh / (nov * noh))
    w = torch.where(spec, w_spec, (1 - met) * alb) * keep.reshape(P, sc, 1)
    H, W = env.shape[:2]
    fx = (0.5 - torch.atan2(dout[..., 1], dout[..., 0]) / (2 * math.pi)) * W - 0.5
    fy = torch.atan2(torch.hypot(dout[..., 0], dout[..., 1]), dout[..., 2]) / math.pi * H - 0.5
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
    Vo, Fo = icosphere(6, 0.5)
    Vi, Fi = icosphere(5, 0.2)
    Vi = (Vi + np.array([0.1, 0.0, 0.05], np.float32)).astype(np.float32)
    mat = np.tile(np.array([0.8, 0.6, 0.4, 0.5, 0.4], np.float32), (len(Vi), 1))
    ns = R.NestedScene(Vo, Fo, 1.5, Vi, Fi, mat, device=dev)
    h = w = flags.size
    g = np.random.Generator(np.random.PCG64(1))
    env = torch.from_numpy(R.pack_env(g.random((256, 512, 3)).astype(np.float32))).to(dev)
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    CH, eps = 64, R.ORIGIN_EPS
    o_s = ns.outer

    def shared():
        face, gbuf = R.gbuffer(ns.outer, cams, h, w)
        pix = R.hit_pixels(face)
        kind, chain, irow = R.nested_chain(ns, gbuf, pix)
        sel = (kind == R.INNER).nonzero().flatten().to(torch.int32)
        other = (kind != R.INNER).nonzero().flatten().to(torch.int32)
        out = torch.zeros(h * w, 4, device=dev)
        R.nested_resolve(irow, chain, kind, pix, other, 2, 0, 0, 0, env, None, True, out)
        return pix, kind, chain, irow, sel, out

    def chain_only(S):
        pix, kind, chain, irow, sel, out = shared()
        return out, int(sel.numel())

    def fused(S):
        pix, kind, chain, irow, sel, out = shared()
        for s0 in range(0, S, CH):
            sc = min(CH, S - s0)
            rec = R.nested_light(ns, irow, sel, S, s0, sc, 0)
            R.nested_resolve(irow, chain, kind, pix, sel, S, s0, sc, 0, env, rec, s0 + sc == S, out)
        return out, int(sel.numel())

    def composed(S):
        pix, kind, chain, irow, sel, out = shared()
        rows = irow[sel.long()]
        acc = torch.zeros(sel.numel(), 3, device=dev)
        for s0 in range(0, S, CH):
            sc = min(CH, S - s0)
            rays, bits = R.shadow_rays(irow, sel, S, s0, sc, 0)
            hit_i, _ = ns.inner.bvh.intersect(rays)
            hit_o, idx, _ = o_s.bvh.intersect(rays, return_t=True)
            leaky = hit_o == 0
            refr, o2, d2, keep = torch_leave(o_s.V, o_s.F, o_s.normals, ns.ior, rays[:, :3], rays[:, 3:], torch.where(leaky, 0, idx), eps)
            hit_e, _ = o_s.bvh.intersect(torch.cat([o2, d2], 1))
            alive = (bits[:, 2] == 1) & (hit_i == 0)
            lit = alive & (leaky | (refr & (hit_e == 0)))
            dout = torch.where(leaky[:, None], rays[:, 3:], d2)
            keep = torch.where(leaky[:, None], torch.ones_like(keep), keep)
            acc += torch_shade(rows, rays[:, 3:], dout, keep, lit, env, S, s0, sc)
        p = pix[sel.long()].long()
        out[p, :3] += chain[sel.long(), :1] * acc
        out[p, 3] = 1.0
        R.nested_resolve(irow, chain, kind, pix, sel, S, 0, 0, 0, env, None, True, out)       # the reflection term of the inner pixels
        return out, int(sel.numel())

    variants = [('fused (registers -> 3 walks -> record -> resolve)', fused), ('composed ([N,6] -> 3 x nu_lbvh_trace -> torch)', composed),
                ('shared passes alone (G-buffer, chain, exit terms)', chain_only)]
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
        print(f"S={S}: {npix} inner pixels of {h * w}; max |fused - composed| = {float((a - b).abs().max()):.3e} "
              f"(image maximum {float(a[:, :3].max()):.3f})")
        base = statistics.median(times[variants[2][0]])
        for name, _ in variants:
            ms = statistics.median(times[name])
            rate = ""
            if name != variants[2][0]:
                # a difference of two medians: no rate unless it stands clear of the spread of the shared passes
                spread = max(times[variants[2][0]]) - min(times[variants[2][0]])
                rate = (f"{npix * S / (ms - base) * 1e3 / 1e9:7.3f} G light paths/s beyond the shared passes" if ms - base > max(spread, 1e-3)
                        else "(within the spread of the shared passes: no rate)")
            print(f"S={S:5d}  {name:50s} median {ms:9.2f} ms/frame (min {min(times[name]):9.2f}, max {max(times[name]):9.2f})  {rate}",
                  flush=True)


if __name__ == '__main__':
    main()
