"""Surface shading A/B and the numbers of DESIGN.md section 34.

    python scripts/bench_surface_shade.py --errors            the layered path's own error against float64 (the bound of the GPU test)
    python scripts/bench_surface_shade.py --kernel [--reps 9] nu_surface_shade_fwd against the layered composition, 131 072 / 640 000 rows
    python scripts/bench_surface_shade.py --frame [--hw 800]  an rgb frame of the parity network, part by part, against render_eval

--errors: nets.sdf + the network ops of shading_glue on the 4096 rows of tests/test_surface_shade_gpu.py::test_against_float64_end_to_end
against tests/surface_shade_oracle.py, largest error per output relative to max(1, |ref|): LAYERED_ERR of that test.
--kernel: the fused kernel against nu_s2_shade_encode_fwd + the four stacks + nu_shade_combine_fwd (stage2_ops.shade_encode,
nets.predictors, stage2_ops.shade_combine) in chunks of 65 536 rows (a fixed workspace), on the same rows with the same raw material
heads.  GPU events around each variant, one warm-up round, median of --reps, alternating order.  TFLOP/s against the fp32-MFMA peak
(157.3 TFLOP/s), algorithmic FLOP of the 21 hidden layers and 7 heads per row.
--frame: trace, SDF gradient, material bake and shade of one camera timed separately (GPU events, median of --reps), the whole
render_surface(aovs='rgb') call, and render_eval of the same rays; mean / max |surface rgb - volume-rendered rgb| over the hit pixels.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np   # noqa: E402
import torch   # noqa: E402

PEAK = 157.3e12
CHUNK = 65536


def parity_net(dev, sphere=False):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.renderer import NeROShapeRenderer
    arrays = randomize_for_parity(init_stage1_params(6033, sphere_direction=sphere), seed=1)
    net = NeROShapeRenderer({'name': 'parity', 'shader_config': {'sphere_direction': sphere}}, training=False)
    net.load_param_dict(arrays)
    return net.to(dev), arrays


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


def layered_terms(nets, scfg, lut, x, grads, v, feats):
    """The terms of shading_glue._shade_with_images WITHOUT its display clamps, on the same network ops."""
    import torch.nn.functional as F
    from nu_nerf_amd import torch_glue as G
    from nu_nerf_amd.shading_glue import lights, shade
    exp_max = scfg['light_exp_max']
    n, vv = F.normalize(grads, dim=-1), F.normalize(v, dim=-1)
    nov = torch.sum(n * vv, -1, keepdim=True)
    refl = nov * n * 2 - vv
    m = torch.sigmoid(nets.materials(feats, x))
    metallic, rough, albedo, trans = m[:, 0:1], m[:, 1:2], m[:, 2:5], m[:, 5:6]
    diffuse_light, light, light0, occ, indirect = lights(nets, exp_max, x, n, refl, rough, bool(scfg.get('sphere_direction', False)), detail=True)
    t = torch.clamp(1 - nov, 0.0, 1.0)
    fres = torch.clamp(0.04 + 0.96 * t * t * t * t * t, 0.0, 1.0)
    fg = G.lut_bilinear_clamp(lut[0], torch.cat([torch.clamp(nov, 0.0, 1.0), torch.clamp(rough, 0.0, 1.0)], -1))
    diffuse_color = (1 - metallic) * albedo * diffuse_light
    spec_color = ((0.04 * (1 - metallic) + metallic * albedo) * fg[:, 0:1] + fg[:, 1:2]) * light
    refrac = torch.exp(torch.clamp(nets.predictor('refrac_light', torch.cat([G.embed(x, 6), G.embed(vv, 6)], -1)), max=exp_max))
    color, _ = shade(nets, scfg, lut, x, grads, v, feats)
    return {'rgb': color, 'diffuse_color': G.linear_to_srgb(diffuse_color),
            'specular_color': G.linear_to_srgb(spec_color) * (1 - trans) + fres * light0 * trans,
            'diffuse_light': diffuse_light, 'specular_light': light0, 'occ_prob': occ[:, 0], 'indirect_light': indirect,
            'refraction_light': G.linear_to_srgb((1 - fres) * refrac * trans), 'reflection_weight': fres[:, 0]}


def errors(dev):
    import surface_shade_oracle as SO
    from test_surface_shade_gpu import rows
    from nu_nerf_amd.nets import Stage1Nets
    import test_environment_gpu as TE
    net, arrays = TE.stage1_net(dev, False)                     # the network of the test (occlusion head gain as there)
    nets = Stage1Nets(net.engine(), net._named())
    x_np, v_np, _ = rows(4096, 4096)
    cfg = {'light_exp_max': 3.0, 'sphere_direction': False, 'refrac_freq': 6}
    want = SO.shade64(arrays, cfg, x_np, v_np)
    x, v = torch.from_numpy(x_np).to(dev), torch.from_numpy(v_np).to(dev)
    with torch.no_grad():
        net.engine().pack()
        y, grads = nets.sdf(x)
        got = layered_terms(nets, net.color_network.cfg, net.color_network.FG_LUT, x, grads, v, y[:, 1:].contiguous())
    err = {k: float((np.abs(t.cpu().numpy().astype(np.float64) - want[k]) / np.maximum(1.0, np.abs(want[k]))).max()) for k, t in got.items()}
    print("layered path vs float64, 4096 rows, largest error relative to max(1, |ref|):")
    print("LAYERED_ERR = {" + ', '.join(f"'{k}': {e:.1e}" for k, e in err.items()) + "}")


def kernel(dev, reps):
    from nu_nerf_amd import stage2_ops as O
    from nu_nerf_amd.nets import Stage1Nets
    from nu_nerf_amd.surface_shade import shade_points
    from test_surface_shade_gpu import rows
    for sphere in (False, True):
        net, _ = parity_net(dev, sphere)
        eng = net.engine()
        nets = Stage1Nets(eng, net._named())
        scfg, lut = net.color_network.cfg, net.color_network.FG_LUT
        k_ol = 144 if sphere else 72
        flop = 2 * (3 * (k_ol * 256 + 2 * 65536 + 768) + 2 * (111 * 256 + 2 * 65536 + 768) + (78 * 256 + 2 * 65536 + 256) + (78 * 256 + 2 * 65536 + 768))
        print(f"sphere_direction {sphere}: {flop / 1e6:.3f} MFLOP per row")
        for n in (131072, 640000):
            x, v, nr = (torch.from_numpy(a).to(dev) for a in rows(n, 9))
            with torch.no_grad():
                eng.pack()
                mr = torch.zeros(n, 8, device=dev)
                for i in range(0, n, CHUNK):
                    y, _ = nets.sdf(x[i:i + CHUNK])
                    mr[i:i + CHUNK, :6] = nets.materials(y[:, 1:].contiguous(), x[i:i + CHUNK])
                    del y

                def fused():
                    return shade_points(net, x, v, nr, _mraw=mr)['rgb']

                def layered():
                    out = torch.empty(n, 3, device=dev)
                    for i in range(0, n, CHUNK):
                        s = slice(i, i + CHUNK)
                        OL, IL, IW, RL, nov, _ = O.shade_encode(eng, x[s], nr[s], v[s], mr[s, :6], sphere, 6, 6)
                        ol, il, iw, rl = nets.predictors(('outer_light', 'inner_light', 'inner_weight', 'refrac_light'), (OL, IL, IW, RL))
                        out[s] = O.shade_combine(eng, mr[s, :6], ol, il, iw, rl, nov[:, None], lut, eng.exp_max)[0]
                    return out
                res, ms, mem = {}, {}, {}
                for name, fn in (('fused', fused), ('layered', layered)):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    out = fn()
                    torch.cuda.synchronize()
                    mem[name] = torch.cuda.max_memory_allocated() - base - out.numel() * 4
                    del out
                    ms[name] = timed(fn, reps)
                    res[name] = ms[name][3]
                same = bool(torch.equal(res['fused'], res['layered']))
                for name in ('fused', 'layered'):
                    med, lo, hi, _ = ms[name]
                    per = min(n, CHUNK) if name == 'layered' else n
                    print(f"  {n:7d} rows  {name:8s} median {med:8.3f} ms (min {lo:8.3f}, max {hi:8.3f})  {n * flop / med * 1e3 / 1e12:6.1f} TFLOP/s = "
                          f"{n * flop / med * 1e3 / PEAK:5.3f} of peak   workspace {mem[name] / per:7.0f} B per row of a pass")
                print(f"  {n:7d} rows  layered / fused = {ms['layered'][0] / ms['fused'][0]:.2f}   same bits: {same}")
                del res, ms


def frame(dev, reps, hw):
    from nu_nerf_amd.mask_render import pinhole_rays
    from nu_nerf_amd.relight import intrinsics, relighting_poses
    from nu_nerf_amd.sdf_trace import trace_rays
    from nu_nerf_amd.validation import render_eval
    net, _ = parity_net(dev)
    eng = net.engine()
    K, pose = intrinsics(hw, hw), relighting_poses(8, 0.0, 45.0, 3.0)[0]
    rays = pinhole_rays(torch.as_tensor(K, dtype=torch.float32).reshape(3, 3), torch.as_tensor(pose, dtype=torch.float32).reshape(1, 3, 4), hw, hw, dev)
    with torch.no_grad():
        eng.pack()
        t_tr = timed(lambda: trace_rays(net, rays[:, :3], rays[:, 3:], entry_forward=True), reps)
        tr = t_tr[3]
        idx = tr['hit'].nonzero().reshape(-1)
        pts, view = tr['pos'][idx].contiguous(), -rays[idx, 3:6]
        P = pts.shape[0]
        g = torch.empty(P, 3, device=dev)
        t_gr = timed(lambda: eng.sdf_grad(pts.data_ptr(), 3, P, grad=g), reps)
        m = [torch.empty(P, device=dev), torch.empty(P, device=dev), torch.empty(P, 3, device=dev), torch.empty(P, device=dev)]
        t_bk = timed(lambda: eng.material_bake(pts.data_ptr(), 3, P, *m, raw=True), reps)
        mr = torch.zeros(P, 8, device=dev)
        mr[:, 0], mr[:, 1], mr[:, 2:5], mr[:, 5] = m
        col = torch.empty(P, 3, device=dev)
        t_sh = timed(lambda: eng.surface_shade(pts.data_ptr(), 3, view.data_ptr(), 3, g.data_ptr(), 3, mr.data_ptr(), 8, P, out={'color': col}), reps)
        t_all = timed(lambda: net.render_surface(K, pose, hw, hw, aovs=('rgb', 'mask')), reps)
        img = t_all[3]
        print(f"{hw} x {hw} frame of the parity network, {P} of {hw * hw} pixels hit")
        for name, t in (('trace', t_tr), ('SDF gradient', t_gr), ('material bake', t_bk), ('shade', t_sh), ('render_surface(rgb, mask)', t_all)):
            print(f"  {name:28s} median {t[0]:9.3f} ms (min {t[1]:9.3f}, max {t[2]:9.3f})")
        batch = {'rays_o': rays[:, :3].contiguous(), 'rays_d': rays[:, 3:6].contiguous()}
        t_ev = timed(lambda: render_eval(net, batch, 300000), 1)
        vol = t_ev[3]['ray_rgb'].reshape(hw, hw, 3)
        hit = img['mask'] > 0
        d = (img['rgb'][hit] - torch.clamp(vol[hit], 0.0, 1.0)).abs()
        print(f"  {'render_eval':28s} {t_ev[0]:9.1f} ms   = {t_ev[0] / t_all[0]:.0f} x render_surface")
        print(f"  |surface rgb - volume-rendered rgb| over the hit pixels: mean {float(d.mean()):.4f}, max {float(d.max()):.4f}")


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
