"""The fused NeRF++ background kernel: A/B against the layered composition and the numbers of DESIGN.md section 36.

    python scripts/bench_background.py --errors             the layered composition's own error against float64 (the bound of the GPU test)
    python scripts/bench_background.py --kernel [--reps 9]  nu_background_fwd against the layered composition, 131 072 / 640 000 rays x 96 nodes
    python scripts/bench_background.py --frame [--hw 800]   a `frame` of the parity network, part by part, against render_eval

--errors: on the 512 rays x 96 default nodes of tests/test_background_gpu.py::test_float64 (half of the rays with a stop), against
tests/background_oracle.py: the layered composition -- nodes -> nu_partition_* -> Engine.nerf_forward -> nu_composite_fwd's rgb_bg with
stopped alphas zeroed in torch; transmittance = torch's fp32 prod of (1 - alpha + 1e-7) over the same alphas -- and the fused kernel,
largest error per output relative to max(1, |ref|) over every ray: LAYERED_ERR of that test.
--kernel: the same rays through both, the layered composition in chunks of at most 65 536 rows (682 rays: a fixed workspace; every
chunk costs it one host read of the inner count).  GPU events around each variant, one warm-up round, median of --reps, alternating
order.  TFLOP/s against the fp32-MFMA peak (157.3 TFLOP/s): ALGORITHMIC FLOP, 604 160 MACs = 1.208 MFLOP per LIVE row; the padded figure
(647 808 MACs for every row of a tile that has a live row: K padded to 96 / 352 / 288, the view layer computed 256 wide) is printed
beside it and marked as such.
--frame: trace, shade and background of one camera of the relight orbit timed separately (GPU events, median of --reps), the whole
render_surface(aovs=('frame', 'mask')) call, and render_eval of the same rays; mean / max |frame - ray_rgb| over hit and missed pixels.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch   # noqa: E402

PEAK = 157.3e12
CHUNK = 65536
MACS, MACS_PADDED = 604160, 647808


def parity_net(dev):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.renderer import NeROShapeRenderer
    net = NeROShapeRenderer({'name': 'parity', 'is_nerf': True}, training=False)
    net.load_param_dict(randomize_for_parity(init_stage1_params(6033), seed=1))
    return net.to(dev)


def timed(fn, reps):
    ts = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts), out


def timed_ab(fns, reps):
    """{name: (median, min, max, last result)} of the variants run in turn, the order reversed every round; the first round warms up."""
    ts, out = {k: [] for k, _ in fns}, {}
    for rep in range(reps + 1):
        for name, fn in (fns if rep % 2 == 0 else fns[::-1]):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ts[name].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v), out[k]) for k, v in ts.items()}


def torch_mid(z):
    dist = z[:, 1:] - z[:, :-1]
    return z + torch.cat([dist, dist[:, -1:]], -1) * 0.5


def layered(eng, o, d, z, stop=None):
    """color_bkgr and the background transmittance of rays through the existing kernels, at most CHUNK rows at a time."""
    from nu_nerf_amd.engine import addr
    lib, S_ = eng.lib, eng.stream()
    R, S = z.shape
    dev = z.device
    color, trans = torch.empty(R, 3, device=dev), torch.empty(R, device=dev)
    per = max(1, CHUNK // S)
    e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)      # noqa: E731
    for i in range(0, R, per):
        oc, dc, zc = o[i:i + per].contiguous(), d[i:i + per].contiguous(), z[i:i + per].contiguous()
        r = zc.shape[0]
        cnt, off, tot = e(r, dtype=torch.int32), e(r, dtype=torch.int32), e(2, dtype=torch.int32)
        lib.nu_partition_count(addr(oc), addr(dc), addr(zc), r, S, addr(cnt), addr(off), addr(tot), S_)
        P_in = int(tot[0].item())
        P_out = r * S - P_in
        pt_in, idx_in = e(max(P_in, 1), 8), e(max(P_in, 1), dtype=torch.int32)
        pt_out, idx_out = e(max(P_out, 1), 8), e(max(P_out, 1), dtype=torch.int32)
        inner_rm = e(r * S, dtype=torch.uint8)
        lib.nu_partition_write(addr(oc), addr(dc), addr(zc), r, S, addr(off), addr(pt_in), addr(idx_in), addr(pt_out), addr(idx_out),
                               addr(inner_rm), S_)
        alpha_rm, color_rm = torch.zeros(r * S, device=dev), torch.zeros(r * S, 4, device=dev)
        if P_out > 0:
            eng.nerf_forward(pt_out, idx_out, P_out, alpha_rm, color_rm)
        if stop is not None:
            alpha_rm = torch.where((torch_mid(zc) < stop[i:i + per, None]).reshape(-1), alpha_rm, torch.zeros_like(alpha_rm))
        rgb, acc, aux = e(r, 3), e(r), e(r)
        lib.nu_composite_fwd(addr(alpha_rm), addr(color_rm), addr(inner_rm), r, S, 0, addr(rgb), addr(acc), addr(color[i:]), addr(aux), S_)
        trans[i:i + per] = torch.prod(1.0 - alpha_rm.view(r, S) + 1e-7, dim=1)
    return color, trans


def errors(dev):
    from test_background_gpu import _err, float64_case
    from test_stage1_gpu import make_net
    net = make_net(dev)
    o, d, z, stop, col, tr = float64_case(net, dev)
    eng = net.engine()
    with torch.no_grad():
        eng.pack()
        lc, lt = layered(eng, o, d, z, stop)
        out = net.render_background(o, d, z=z, t_stop=stop)
    lay = {'color': _err(lc, col), 'transmittance': _err(lt, tr)}
    ker = {'color': _err(out['color'], col), 'transmittance': _err(out['transmittance'], tr)}
    print(f"{z.shape[0]} rays x {z.shape[1]} default nodes, half with a stop; largest error relative to max(1, |ref|) against float64:")
    print("LAYERED_ERR = {" + ', '.join(f"'{k}': {e:.1e}" for k, e in lay.items()) + "}")
    print("bound (4 x)  = {" + ', '.join(f"'{k}': {4 * e:.1e}" for k, e in lay.items()) + "}")
    print("KERNEL_ERR  = {" + ', '.join(f"'{k}': {e:.1e}" for k, e in ker.items()) + "}")
    print(f"kernel colour bits equal the layered composition's on {int((out['color'] == lc).all(1).sum())} of {z.shape[0]} rays "
          "(the kernel composes in sample order, nu_composite_fwd by lanes)")


def kernel(dev, reps):
    from nu_nerf_amd.background import default_nodes
    from test_background_gpu import make_rays
    net = parity_net(dev)
    eng = net.engine()
    print(f"{2 * MACS / 1e6:.3f} MFLOP per live row algorithmic ({MACS} MACs); padded: {2 * MACS_PADDED / 1e6:.3f} MFLOP per row of a live tile")
    for n in (131072, 640000):
        o, d, _ = make_rays(n, 2, 5, dev)
        with torch.no_grad():
            eng.pack()
            z = default_nodes(net, o, d, n_samples=64, n_bg_samples=32)
            x = o[:, None, :] + d[:, None, :] * torch_mid(z)[..., None]
            live = torch.linalg.norm(x, dim=-1) > 1.0
            rows = int(live.sum())
            tiles = int(live.view(n, 3, 32).any(-1).sum())
            del x

            def fused():
                out = net.render_background(o, d, z=z)
                return out['color'], out['transmittance']

            def lay():
                return layered(eng, o, d, z)
            ms = timed_ab((('fused', fused), ('layered', lay)), reps)
            dc = float((ms['fused'][3][0] - ms['layered'][3][0]).abs().max())
            print(f"{n} rays x 96 nodes: {rows} live rows ({rows / (n * 96):.3f}), {tiles} live tiles of {3 * n}")
            for name in ('fused', 'layered'):
                med, lo, hi, _ = ms[name]
                print(f"  {name:8s} median {med:9.3f} ms (min {lo:9.3f}, max {hi:9.3f})  {rows * 2 * MACS / med * 1e3 / 1e12:6.1f} TFLOP/s algorithmic = "
                      f"{rows * 2 * MACS / med * 1e3 / PEAK:5.3f} of peak" +
                      (f"   [padded: {tiles * 32 * 2 * MACS_PADDED / med * 1e3 / 1e12:6.1f} TFLOP/s]" if name == 'fused' else ''))
            print(f"  layered / fused = {ms['layered'][0] / ms['fused'][0]:.2f}   fused / layered = {ms['fused'][0] / ms['layered'][0]:.2f}   "
                  f"max |colour difference| {dc:.1e}")
            del ms


def frame(dev, reps, hw):
    from nu_nerf_amd.background import default_nodes
    from nu_nerf_amd.mask_render import pinhole_rays
    from nu_nerf_amd.relight import intrinsics, relighting_poses
    from nu_nerf_amd.sdf_trace import trace_rays
    from nu_nerf_amd.validation import render_eval
    net = parity_net(dev)
    eng = net.engine()
    K, pose = intrinsics(hw, hw), relighting_poses(8, 0.0, 45.0, 3.0)[0]
    rays = pinhole_rays(torch.as_tensor(K, dtype=torch.float32).reshape(3, 3), torch.as_tensor(pose, dtype=torch.float32).reshape(1, 3, 4), hw, hw, dev)
    with torch.no_grad():
        eng.pack()
        t_tr = timed(lambda: trace_rays(net, rays[:, :3], rays[:, 3:], entry_forward=True), reps)
        tr = t_tr[3]
        stop = torch.where(tr['hit'] != 0, tr['t'], torch.full_like(tr['t'], float('inf')))
        t_sh = timed(lambda: net.render_surface(K, pose, hw, hw, aovs=('rgb',)), reps)
        t_nd = timed(lambda: default_nodes(net, rays[:, :3], rays[:, 3:]), reps)
        z = t_nd[3]
        t_bg = timed(lambda: net.render_background(rays[:, :3], rays[:, 3:], z=z, t_stop=stop), reps)
        t_all = timed(lambda: net.render_surface(K, pose, hw, hw, aovs=('frame', 'mask')), reps)
        img = t_all[3]
        hit = img['mask'] > 0
        print(f"{hw} x {hw} frame of the parity network, {int(hit.sum())} of {hw * hw} pixels hit")
        for name, t in (('trace', t_tr), ('render_surface(rgb): trace + shade', t_sh), ('default nodes', t_nd), ('background kernel', t_bg),
                        ('render_surface(frame, mask)', t_all)):
            print(f"  {name:36s} median {t[0]:9.3f} ms (min {t[1]:9.3f}, max {t[2]:9.3f})")
        batch = {'rays_o': rays[:, :3].contiguous(), 'rays_d': rays[:, 3:6].contiguous()}
        t_ev = timed(lambda: render_eval(net, batch, 300000), 1)
        vol = torch.clamp(t_ev[3]['ray_rgb'].reshape(hw, hw, 3), 0.0, 1.0)
        print(f"  {'render_eval':36s} {t_ev[0]:9.1f} ms   = {t_ev[0] / t_all[0]:.1f} x render_surface(frame, mask)")
        for name, m in (('hit', hit), ('missed', ~hit)):
            dd = (img['frame'][m] - vol[m]).abs()
            print(f"  |frame - ray_rgb| over the {name} pixels: mean {float(dd.mean()):.4f}, max {float(dd.max()):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--errors', action='store_true')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--frame', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--hw', type=int, default=800)
    flags = ap.parse_args()
    dev = torch.device('cuda:0')
    if flags.errors:
        errors(dev)
    if flags.kernel:
        kernel(dev, flags.reps)
    if flags.frame:
        frame(dev, flags.reps, flags.hw)


if __name__ == '__main__':
    main()
