"""Texture-atlas timings.

  texels   nu_atlas_texels over a whole atlas of T = 2048 and 4096 for the 81 920-face icosphere (points + face ids, one 16-byte store
           per texel) against the same computation written in torch ops (index arithmetic, gathers, the barycentric mix), and as a
           share of the store rate a fill of the same bytes reaches (torch's zero_ of the output buffer, timed the same way).  A
           launch is shorter than the host work around it, so the kernel and the fill are also timed as --burst launches back to
           back into one preallocated buffer inside one event pair, divided by the count: the "launch alone" lines.
  bake     bake_textures end to end at T = 2048 on a stage-1 model with random weights, split into its three parts: texel points
           (nu_atlas_texels), selection of the owned texels (nonzero + gather) and the networks (the fused bake kernel).
  gbuffer  nu_atlas_gbuffer on the hit pixels of one 800 x 800 frame against the G-buffer pass it follows (nu_relight_gbuffer).

GPU events, one warm-up then the median of --reps per variant (min .. max beside it), variants alternating, one process.

    python scripts/bench_texture.py [--subdiv 6] [--sizes 2048 4096] [--bake-size 2048] [--frame 800] [--reps 10] [--burst 20]
"""
import argparse
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


def texels_torch(V, F, lay):
    """nu_atlas_texels in torch ops: (points [T,T,3], face [T,T])."""
    T, c, cols, nf, pad, L = lay['size'], lay['cell'], lay['cols'], lay['n_faces'], lay['pad'], lay['L']
    ar = torch.arange(T, device=V.device, dtype=torch.int32)
    y, x = ar[:, None].expand(T, T), ar[None, :].expand(T, T)
    cx, cy = torch.div(x, c, rounding_mode='floor'), torch.div(y, c, rounding_mode='floor')
    i, j = x - cx * c, y - cy * c
    h = (i + j >= c).to(torch.int32)
    f = 2 * (cy * cols + cx) + h
    own = (cx < cols) & (cy < cols) & (i + j != c - 1) & (f < nf)
    s, t = torch.where(h == 1, c - 1 - i, i), torch.where(h == 1, c - 1 - j, j)
    b1, b2 = (s - pad).float() / float(L), (t - pad).float() / float(L)
    b0 = (1.0 - b1) - b2
    tri = V[F[f.clamp(0, nf - 1).long()].long()]                       # [T,T,3,3]
    p = (b0[..., None] * tri[..., 0, :] + b1[..., None] * tri[..., 1, :]) + b2[..., None] * tri[..., 2, :]
    return torch.where(own[..., None], p, torch.zeros_like(p)), torch.where(own, f, torch.full_like(f, -1))


def stage1_net(dev):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.renderer import NeROShapeRenderer
    net = NeROShapeRenderer({'name': 'bench'}, training=False)
    net.load_param_dict(randomize_for_parity(init_stage1_params(6033), seed=1))
    return net.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subdiv', type=int, default=6, help="icosphere level (6: 81 920 faces)")
    ap.add_argument('--sizes', type=int, nargs='+', default=[2048, 4096])
    ap.add_argument('--bake-size', type=int, default=2048)
    ap.add_argument('--frame', type=int, default=800)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--burst', type=int, default=20, help="back-to-back launches of the 'launch alone' lines")
    flags = ap.parse_args()
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _cams
    from nu_nerf_amd.materials import bake_materials

    dev = torch.device('cuda:0')
    V, F = icosphere(flags.subdiv, 0.5)
    Vd, Fd = torch.from_numpy(np.asarray(V, np.float32)).to(dev), torch.from_numpy(np.asarray(F, np.int32)).to(dev)
    print(f"{torch.cuda.get_device_name(0)}; {len(F)} faces, {len(V)} vertices")

    # ---- texels ----------------------------------------------------------------------------------------------------------------
    for T in flags.sizes:
        lay = X.atlas_layout(len(F), T)
        buf = torch.empty(T, T, 4, device=dev)
        lib, B = L.load(), flags.burst

        def burst_kernel():
            for _ in range(B):
                lib.nu_atlas_texels(L.ptr(Vd), len(V), L.ptr(Fd), len(F), None, T, 0, 0, T, L.ptr(buf), None, L.stream())

        def burst_fill():
            for _ in range(B):
                buf.zero_()
        variants = [('nu_atlas_texels', lambda: X.atlas_texels(Vd, Fd, lay)),
                    ('the same in torch ops', lambda: texels_torch(Vd, Fd, lay)),
                    ('zero_ of the same 16 bytes per texel', lambda: buf.zero_()),
                    (f'nu_atlas_texels, launch alone (x {B})', burst_kernel),
                    (f'zero_, launch alone (x {B})', burst_fill)]
        times, outs = alternate(variants, flags.reps)
        a, b = outs['nu_atlas_texels'], outs['the same in torch ops']
        same = bool(torch.equal(a[1], b[1])) and float((a[0] - b[0]).abs().max())
        nbytes = T * T * 16
        print(f"texels T = {T}: cell {lay['cell']}, L {lay['L']}, {int((a[1] >= 0).sum())} owned texels "
              f"({100.0 * int((a[1] >= 0).sum()) / T ** 2:.1f} %); ids equal and max |point difference| to torch ops: {same}")
        for n in list(times):
            if 'launch alone' in n:
                times[n] = [t / B for t in times[n]]
        med = {n: statistics.median(t) for n, t in times.items()}
        for n, _ in variants:
            print(f"{line(n, times[n])}  {nbytes / med[n] * 1e3 / 1e12:6.3f} TB/s stored", flush=True)
        k_alone, f_alone = med[f'nu_atlas_texels, launch alone (x {B})'], med[f'zero_, launch alone (x {B})']
        print(f"  torch ops / kernel (calls) {med['the same in torch ops'] / med['nu_atlas_texels']:.1f} x, / kernel (launch alone) "
              f"{med['the same in torch ops'] / k_alone:.1f} x; the launch alone stores at {100.0 * f_alone / k_alone:.0f} % of the fill's rate")

    # ---- bake_textures ---------------------------------------------------------------------------------------------------------
    net = stage1_net(dev)
    T = flags.bake_size
    lay = X.atlas_layout(len(F), T)
    p, f, _ = X.atlas_texels(Vd, Fd, lay)

    def select():
        sel = (f.reshape(-1) >= 0).nonzero().flatten()
        return p.reshape(-1, 3)[sel].contiguous()
    pts = select()
    variants = [('bake_textures end to end', lambda: X.bake_textures(net, Vd, Fd, size=T)),
                ('  texel points (nu_atlas_texels)', lambda: X.atlas_texels(Vd, Fd, lay)),
                ('  selection (nonzero + gather)', select),
                ('  networks (fused bake kernel)', lambda: bake_materials(net, pts))]
    times, _ = alternate(variants, flags.reps)
    print(f"bake T = {T}: {pts.shape[0]} owned texels of {T * T}")
    for n, _ in variants:
        print(line(n, times[n]), flush=True)
    print(f"  {pts.shape[0] / statistics.median(times['  networks (fused bake kernel)']) * 1e3 / 1e6:.1f} M texels/s through the networks")

    # ---- the G-buffer pass -----------------------------------------------------------------------------------------------------
    tex = torch.rand(T, T, 5, device=dev)
    atlas = X.pack_atlas(tex, lay)
    mat = np.tile(np.array([0.8, 0.6, 0.4, 0.0, 0.9], np.float32), (len(V), 1))
    scene = R.Scene(V, F, mat, device=dev)
    h = w = flags.frame
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    face, gbuf = R.gbuffer(scene, cams, h, w)
    pix = R.hit_pixels(face)
    variants = [('nu_relight_gbuffer', lambda: R.gbuffer(scene, cams, h, w)),
                ('nu_atlas_gbuffer', lambda: X.texture_gbuffer(scene, face, gbuf, pix, atlas))]
    times, _ = alternate(variants, flags.reps)
    print(f"gbuffer {h} x {w}, {int(pix.numel())} hit pixels, atlas T = {T}")
    for n, _ in variants:
        print(line(n, times[n]), flush=True)


if __name__ == '__main__':
    main()
