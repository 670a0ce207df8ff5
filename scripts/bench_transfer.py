"""Visibility-transfer timings.

  bake     every vertex of a mesh at S samples: the fused kernel (nu_transfer_bake, one launch, nothing stored but the rows) against the
           composition the library offered before it -- per chunk of points the rays written out [chunk x S, 6], nu_lbvh_trace on
           them, the transfer sums in torch.  Three meshes: the marching-cubes mesh of a sphere at --mc-res^3 (2.5 M faces at
           1024: the size of an extracted asset), the 81 920-face sphere (convex: every ray leaves at once) and that sphere
           hovering over a ground grid (the ground's rays meet it, the sphere's underside meets the ground).  Rays per second =
           points x S / time; the composition's peak workspace is torch's peak allocation above the resting level.
  resolve  one 800 x 800 frame of the hovering sphere: nu_relight_splitsum against nu_relight_splitsum_occluded in both modes, the
           resolve launch alone.

GPU events, one warm-up then the median of --reps per variant, variants alternating, one process.

    python scripts/bench_transfer.py [--subdiv 6] [--mc-res 1024] [--samples 1024] [--chunk 4096] [--size 800] [--reps 5]
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
    return f"{name:62s} median {statistics.median(t):9.3f} ms (min {min(t):9.3f}, max {max(t):9.3f})"


def sh9(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return torch.stack([torch.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                        0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def composition(bvh, P, N, S, chunk):
    """The rows from separate passes: rays to memory, nu_lbvh_trace, sums in torch (fp32, torch's summation order)."""
    from nu_nerf_amd.transfer import transfer_rays
    out = torch.zeros(P.shape[0], 16, device=P.device)
    for i0 in range(0, P.shape[0], chunk):
        p, n = P[i0:i0 + chunk], N[i0:i0 + chunk]
        rays, _ = transfer_rays(p, n, S, 0, None, i0)
        hit, _ = bvh.intersect(rays)
        vis = (hit == 0).to(torch.float32).reshape(-1, S, 1)
        d = rays[:, 3:].reshape(-1, S, 3)
        out[i0:i0 + chunk, 0:9] = (vis * sh9(d)).sum(1) / S
        out[i0:i0 + chunk, 9] = vis.sum((1, 2)) / S
        b = (vis * d).sum(1)
        ln = b.norm(dim=1, keepdim=True)
        out[i0:i0 + chunk, 10:13] = torch.where(ln < 1e-12, n, b / ln.clamp_min(1e-30))
    return out


def hovering_sphere(subdiv):
    """The sphere of radius 0.3 at height 0.35 over a 64 x 64 grid of quads at z = 0."""
    from nu_nerf_amd.lbvh import icosphere
    Vs, Fs = icosphere(subdiv, 0.3)
    Vs = Vs + np.array([0.0, 0.0, 0.35], np.float32)
    n = 65
    gx, gy = np.meshgrid(np.linspace(-1.2, 1.2, n), np.linspace(-1.2, 1.2, n), indexing='ij')
    Vg = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], 1).astype(np.float32)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).ravel()
    Fg = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int32)
    return np.concatenate([Vs, Vg]), np.concatenate([Fs, Fg + len(Vs)]).astype(np.int32)


def marching_cubes_sphere(res, dev):
    """The r = 0.5 sphere extracted by marching cubes from a res^3 grid (scripts/bench_remesh.py's mesh): 2.5 M faces at 1024^3."""
    from nu_nerf_amd.mesh import marching_cubes
    x = torch.linspace(-1.0, 1.0, res, device=dev)
    u = torch.empty(res, res, res, device=dev)
    for i in range(res):                                   # slab by slab: a 1024^3 float64 meshgrid would not fit
        X, Y, Z = torch.meshgrid(x[i:i + 1].double(), x.double(), x.double(), indexing='ij')
        u[i] = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.5).float()[0]
    V, F = marching_cubes(u, 0.0)
    return (V * (2.0 / (res - 1)) - 1.0).contiguous(), F.flip(1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subdiv', type=int, default=6, help="icosphere level (6: 81 920 faces)")
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--chunk', type=int, default=4096, help="points per chunk of the composition")
    ap.add_argument('--mc-res', type=int, default=1024, help="grid of the marching-cubes sphere (1024: 2.5 M faces); 0 leaves it out")
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--reps', type=int, default=5)
    flags = ap.parse_args()
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.environment import DEFAULT_LEVELS, prefilter, project_sh
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _cams
    from nu_nerf_amd.transfer import bake_transfer

    dev = torch.device('cuda:0')
    S = flags.samples
    scenes = [('marching-cubes sphere %d^3' % flags.mc_res, lambda: marching_cubes_sphere(flags.mc_res, dev))] if flags.mc_res else []
    scenes += [('sphere', lambda: icosphere(flags.subdiv, 0.5)), ('sphere over ground', lambda: hovering_sphere(flags.subdiv))]
    for name, make in scenes:
        V, F = make()
        mat = np.tile(np.array([0.8, 0.6, 0.4, 0.0, 0.9], np.float32), (len(V), 1))
        scene = R.Scene(V, F, mat, device=dev)
        P, N = scene.V, scene.normals
        rays = P.shape[0] * S
        variants = [('nu_transfer_bake (one launch)', lambda: bake_transfer(None, None, S, scene=scene)),
                    ('rays to memory + nu_lbvh_trace + torch sums, chunks of %d' % flags.chunk, lambda: composition(scene.bvh, P, N, S, flags.chunk))]
        torch.cuda.synchronize()
        rest = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        composition(scene.bvh, P, N, S, flags.chunk)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - rest
        times, outs = alternate(variants, flags.reps)
        a, b = outs[variants[0][0]], outs[variants[1][0]]
        print(f"bake {name}: {len(F)} faces, {P.shape[0]} points x {S} samples = {rays:.3e} rays; mean AO {float(a[:, 9].mean()):.4f}; AO equal "
              f"{bool(torch.equal(a[:, 9], b[:, 9]))}, max |T fused - T composition| {float((a[:, :9] - b[:, :9]).abs().max()):.3e}; "
              f"composition peak workspace {peak / 2 ** 20:.1f} MiB (fused: the {P.shape[0] * 64 / 2 ** 20:.1f} MiB of rows)")
        for vname, _ in variants:
            ms = statistics.median(times[vname])
            print(f"{line(vname, times[vname])}  {rays / ms * 1e3 / 1e9:7.2f} G rays/s", flush=True)

    # ---- the resolve of one frame -----------------------------------------------------------------------------------------------
    g = np.random.Generator(np.random.PCG64(1))
    env = (g.random((64, 128, 3)) * np.exp2(g.uniform(-3, 3, (64, 128, 1)))).astype(np.float32)
    pyramid, diffuse, _ = prefilter(env, DEFAULT_LEVELS, 64, 128, device=dev)
    packed, lv = R.pack_pyramid(pyramid, np.asarray(DEFAULT_LEVELS, np.float32))
    pyr, dif = torch.from_numpy(packed).to(dev), torch.from_numpy(R.pack_env(diffuse)).to(dev)
    tr = bake_transfer(None, None, S, scene=scene)
    trd, shd = R._transfer_args(scene, tr, 'sh', project_sh(env))
    R.fg_table(dev)
    h = w = flags.size
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 0.0, 45.0, 1.6))[1:2]
    cams = _cams(R.intrinsics(h, w).astype(np.float32), pose.astype(np.float32), dev)
    face, gbuf = R.gbuffer(scene, cams, h, w)
    pix = R.hit_pixels(face)
    out = torch.zeros(h * w, 4, device=dev)
    variants = [('nu_relight_splitsum', lambda: R.splitsum_resolve(gbuf, pix, pyr, lv, dif, out)),
                ('nu_relight_splitsum_occluded, ao', lambda: R.splitsum_resolve_occluded(scene, gbuf, face, pix, pyr, lv, dif, trd, None, 'ao', out)),
                ('nu_relight_splitsum_occluded, sh', lambda: R.splitsum_resolve_occluded(scene, gbuf, face, pix, pyr, lv, dif, trd, shd, 'sh', out))]
    times, _ = alternate(variants, flags.reps)
    print(f"resolve {h} x {w}, {len(F)} faces, {int(pix.numel())} hit pixels (the launch alone)")
    for vname, _ in variants:
        print(line(vname, times[vname]), flush=True)


if __name__ == '__main__':
    main()
