"""The fused NeRF++ background kernel (csrc/background.hip, nu_nerf_amd/background.py) on the GPU: per-sample bits against the layered
path, parity with the reference's recorded color_bkgr, float64 error against the layered composition's, independence of a ray from
its batch, stop semantics and the render_surface AOVs (the compile record needs no GPU: tests/test_background_host.py)."""
import os

import numpy as np
import pytest
import torch

import background_oracle as BO
import test_environment_gpu as TE
from helpers import exact_fp32_only, golden, parity_params
from test_stage1_gpu import make_net

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["step0_r48", "step20000_r48", "step500_r32_noperturb"]

# Test 3: the bound per output is 4 x the largest error (relative to max(1, |ref|), over every ray, against background_oracle in float64)
# of the EXISTING layered composition -- nodes -> nu_partition_* -> nerf_forward -> nu_composite_fwd's rgb_bg, stopped alphas zeroed in
# torch; its transmittance is torch's fp32 prod of (1 - alpha + 1e-7) over the same alphas -- on the same 512 rays x 96 default nodes,
# measured on an MI355X with scripts/bench_background.py --errors (profiles/r08/bench_background_errors.txt).
LAYERED_ERR = {'color': 1.3e-06, 'transmittance': 1.8e-06}
BOUND = {k: 4.0 * v for k, v in LAYERED_ERR.items()}


def _fixture_rays(tag, gpu):
    g, c = golden(f"train_{tag}.npz"), golden(f"core_{tag}.npz")
    o = torch.from_numpy(g['rays_o']).to(gpu)
    dn = torch.nn.functional.normalize(torch.from_numpy(g['rays_d']).to(gpu), dim=-1)
    return g, o, dn, torch.from_numpy(c['z_vals']).to(gpu)


def make_rays(R, S, seed, gpu):
    """R rays of three kinds in turn -- through the centre, missing the unit sphere, origin inside it -- with S ascending nodes that
    start in front of the sphere and end well behind it, unevenly spaced."""
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    v = torch.nn.functional.normalize(torch.cross(u, torch.randn(R, 3, generator=g), dim=-1), dim=-1)
    kind = torch.arange(R) % 3
    o = torch.where((kind == 2)[:, None], 0.5 * u, 3.0 * u)
    target = torch.where((kind == 1)[:, None], (1.2 + 0.6 * torch.rand(R, 1, generator=g)) * v, 0.3 * v * torch.rand(R, 1, generator=g))
    d = torch.nn.functional.normalize(target - o, dim=-1)
    t0 = torch.where(kind == 2, torch.full((R,), 0.05), torch.full((R,), 1.2)) + 0.3 * torch.rand(R, generator=g)
    span = 3.5 + torch.rand(R, generator=g)
    s = torch.linspace(0.0, 1.0, S)[None, :] ** 1.3 if S > 1 else torch.zeros(1, 1)
    z = t0[:, None] + span[:, None] * s
    return o.to(gpu), d.to(gpu), z.contiguous().to(gpu)


def mixed_stop(z, seed):
    """A stop per ray: most inside the ray's node range (cutting a tile in the middle), some +inf, some in front of everything."""
    R = z.shape[0]
    g = torch.Generator().manual_seed(seed)
    f = torch.rand(R, generator=g).to(z.device)
    t = z[:, 0] + (z[:, -1] - z[:, 0] + 0.1) * (0.15 + 0.8 * f)
    k = torch.arange(R, device=z.device) % 7
    t = torch.where(k == 5, torch.full_like(t, float('inf')), t)
    return torch.where(k == 6, torch.zeros_like(t), t).contiguous()


def torch_mid(z):
    if z.shape[1] >= 2:
        dist = z[:, 1:] - z[:, :-1]
        dist = torch.cat([dist, dist[:, -1:]], -1)
    else:
        dist = torch.zeros_like(z)
    return z + dist * 0.5


def layered(net, o, d, z, t_stop=None):
    """The existing layered path on the same rays: render_forward (nu_partition_*, nerf_forward = nu_nerf_embed + GEMMs + heads +
    nu_nerf_act_fwd), its per-sample buffers scattered to (ray, sample) order, and the background composite with stopped alphas zeroed."""
    from nu_nerf_amd.engine import addr
    eng = net.engine()
    eng.pack()
    R, S = z.shape
    with torch.no_grad():
        out, ctx = eng.render_forward(o.contiguous(), d.contiguous(), z, 1.0)
    inner = ctx['inner_rm'].view(R, S) != 0
    live = ~inner
    if t_stop is not None:
        live = live & (torch_mid(z) < t_stop[:, None])
    dev = z.device
    enc, raw = torch.zeros(R * S, 128, device=dev), torch.zeros(R * S, 4, device=dev)
    if ctx['P_out'] > 0:
        b, idx = ctx['nerf'], ctx['idx_out'][:ctx['P_out']].long()
        enc[idx] = torch.cat([b['H'][0][:ctx['P_out']], b['V'][:ctx['P_out'], 256:288]], -1)
        raw[idx] = torch.cat([b['sig'][:ctx['P_out'], None], b['rgb'][:ctx['P_out'], :3]], -1)
    act = torch.cat([ctx['alpha_rm'][:, None], ctx['color_rm'][:, :3]], -1)
    lv = live.reshape(-1, 1)
    enc, raw, act = (torch.where(lv, t, torch.zeros_like(t)) for t in (enc, raw, act))
    alpha = act[:, 0].contiguous()
    rgb, acc, rgb_bg, aux = (torch.empty(R, c, device=dev) for c in (3, 1, 3, 1))
    eng.lib.nu_composite_fwd(addr(alpha), addr(ctx['color_rm']), addr(ctx['inner_rm']), R, S, 0, addr(rgb), addr(acc), addr(rgb_bg),
                             addr(aux), eng.stream())
    trans = torch.prod(1.0 - alpha.view(R, S) + 1e-7, dim=1)
    return {'inner': inner, 'live': live, 'enc': enc, 'raw': raw, 'act': act, 'color': rgb_bg, 'transmittance': trans}


@pytest.fixture(scope="module")
def net(gpu):
    return make_net(gpu)


@pytest.fixture(scope="module")
def spread_net(gpu):
    """The parity network with alpha_linear and rgb_linear moved so that the raw heads straddle the two thresholds of the activation:
    sig ~ 20 +- 5 (softplus' identity branch above 20) and raw rgb ~ 5 +- 2 (the colour clamp at 5)."""
    from nu_nerf_amd.background import render_background
    n = make_net(gpu)
    o, d, z = make_rays(64, 48, 11, gpu)
    dbg = render_background(n, o, d, z=z, _dbg=True)
    rows = dbg['enc'][:, 3] != 0
    raw = dbg['raw'][rows]
    with torch.no_grad():
        for lin, cols, centre, width in ((n.outer_nerf.alpha_linear, [0], 20.0, 5.0), (n.outer_nerf.rgb_linear, [1, 2, 3], 5.0, 2.0)):
            for j, c in enumerate(cols):
                k = width / float(raw[:, c].std())
                m = float(raw[:, c].median())
                b = float(lin.bias[j])
                lin.weight[j] *= k
                lin.bias[j] = centre - (m - b) * k
    return n


SHAPES = [(1, 1), (1, 2), (3, 31), (5, 32), (4, 33), (48, 80), (7, 96), (2, 160), (600, 32)]


@exact_fp32_only
def test_per_sample_bits_against_the_layered_path(gpu, spread_net):
    """Test 1.  No allowance: every input column, raw head, alpha and colour of every live sample carries the bits of
    nu_partition_write -> nu_nerf_embed -> Engine.nerf_forward -> nu_nerf_act_fwd; rows that are not live are zero; the live mask is
    the partition's outer mask and-ed with the stop test."""
    from nu_nerf_amd.background import render_background
    n_all = n_inner = n_outer = n_live = n_stopped = 0
    sig_hi = sig_lo = raw_hi = raw_lo = 0
    for i, (R, S) in enumerate(SHAPES):
        if (R, S) == (48, 80):
            _, o, d, z = _fixture_rays("step20000_r48", gpu)
        else:
            o, d, z = make_rays(R, S, 100 + i, gpu)
        for stop in (None, mixed_stop(z, 200 + i)):
            ref = layered(spread_net, o, d, z, stop)
            got = render_background(spread_net, o, d, z=z, t_stop=stop, _dbg=True)
            what = f"R={R} S={S} stop={'mixed' if stop is not None else None}"
            assert torch.equal(got['enc'][:, 3] != 0, ref['live'].reshape(-1)), what
            assert torch.equal(got['enc'], ref['enc']), what
            assert torch.equal(got['raw'], ref['raw']), what
            assert torch.equal(got['act'], ref['act']), what
            lv = ref['live'].reshape(-1)
            n_all += R * S
            n_inner += int(ref['inner'].sum())
            if stop is not None:
                n_outer += int((~ref['inner']).sum())
                n_live += int(lv.sum())
                n_stopped += int((~ref['inner']).sum()) - int(lv.sum())
            sig, rgb = got['raw'][lv, 0], got['raw'][lv, 1:]
            sig_hi += int((sig > 20).sum()); sig_lo += int((sig <= 20).sum())
            raw_hi += int((rgb > 5).sum()); raw_lo += int((rgb <= 5).sum())
    assert 0.1 * n_all <= n_inner <= 0.9 * n_all, (n_inner, n_all)
    assert min(n_live, n_stopped) >= 0.1 * n_outer, (n_live, n_stopped, n_outer)
    assert min(sig_hi, sig_lo) >= 0.1 * (sig_hi + sig_lo), (sig_hi, sig_lo)
    assert min(raw_hi, raw_lo) >= 0.1 * (raw_hi + raw_lo), (raw_hi, raw_lo)


@pytest.mark.parametrize("tag", TAGS)
def test_reference_parity(gpu, net, tag):
    """Test 2.  The reference's recorded color_bkgr at its own z_vals, all rays, at the bound test_core_parity_gpu.py holds the layered
    path to."""
    g, o, dn, z = _fixture_rays(tag, gpu)
    out = net.render_background(o, dn, z=z)
    assert out['color'].shape == (o.shape[0], 3) and out['transmittance'].shape == (o.shape[0],)
    np.testing.assert_allclose(out['color'].cpu().numpy(), g['out_color_bkgr'], rtol=1e-4, atol=2e-6)


def _err(x, ref):
    ref = ref.double()
    return float(((x.double().cpu() - ref).abs() / torch.clamp(ref.abs(), min=1.0)).max())


def float64_case(net, gpu):
    """512 rays x 96 default nodes (64 + 32), half of the rays with a stop: (o, d, z, t_stop, oracle colour, oracle transmittance)."""
    from nu_nerf_amd.background import default_nodes
    o, d, _ = make_rays(512, 2, 31, gpu)
    z = default_nodes(net, o, d, n_samples=64, n_bg_samples=32)
    stop = mixed_stop(z, 32)
    stop = torch.where(torch.arange(512, device=gpu) % 2 == 0, stop, torch.full_like(stop, float('inf'))).contiguous()
    col, tr = BO.background(parity_params(), o.cpu(), d.cpu(), z.cpu(), stop.cpu())
    return o, d, z, stop, col, tr


@exact_fp32_only
def test_float64(gpu, net):
    """Test 3.  Measured on an MI355X (scripts/bench_background.py --errors): layered colour / transmittance error LAYERED_ERR, the
    kernel's own error in DESIGN 36."""
    o, d, z, stop, col, tr = float64_case(net, gpu)
    z_ref = BO.default_nodes(o, d, *net.near_far_from_sphere(o, d), 64, 32)
    assert torch.allclose(z, z_ref, rtol=1e-6, atol=0.0)
    out = net.render_background(o, d, z=z, t_stop=stop)
    errs = {'color': _err(out['color'], col), 'transmittance': _err(out['transmittance'], tr)}
    print("background kernel vs float64:", errs, "bounds:", BOUND)
    assert float(col.max()) > 0.3 and float(tr.min()) < 0.7
    for k in errs:
        assert errs[k] <= BOUND[k], (k, errs[k], BOUND[k])


@exact_fp32_only
def test_a_ray_does_not_depend_on_its_batch(gpu, net):
    """Test 4.  color / transmittance bits under a permutation, as a prefix, alone, with other leading dimensions, across two runs and
    in the second grid round (600 rays on 256 workgroups)."""
    from nu_nerf_amd.background import render_background
    o, d, z = make_rays(600, 32, 41, gpu)
    stop = mixed_stop(z, 42)
    base = render_background(net, o, d, z=z, t_stop=stop)
    again = render_background(net, o, d, z=z, t_stop=stop)
    perm = torch.randperm(600, generator=torch.Generator().manual_seed(43)).to(gpu)
    shuf = render_background(net, o[perm].contiguous(), d[perm].contiguous(), z=z[perm].contiguous(), t_stop=stop[perm].contiguous())
    pre = render_background(net, o[:100].contiguous(), d[:100].contiguous(), z=z[:100].contiguous(), t_stop=stop[:100].contiguous())
    wide = torch.randn(600, 11, device=gpu)
    wide[:, 2:5], wide[:, 6:9] = o, d
    sl = render_background(net, wide[:, 2:5], wide[:, 6:9], z=z, t_stop=stop)
    for k in ('color', 'transmittance'):
        assert torch.equal(again[k], base[k]), k
        assert torch.equal(shuf[k], base[k][perm]), k
        assert torch.equal(pre[k], base[k][:100]), k
        assert torch.equal(sl[k], base[k]), k
    for r in (0, 255, 256, 599):                       # first and second grid round
        one = render_background(net, o[r:r + 1], d[r:r + 1], z=z[r:r + 1], t_stop=stop[r:r + 1])
        for k in ('color', 'transmittance'):
            assert torch.equal(one[k], base[k][r:r + 1]), (k, r)
    assert float(base['color'].std()) > 1e-3


@exact_fp32_only
def test_stop_semantics(gpu, net):
    """Test 5."""
    from nu_nerf_amd.background import render_background
    o, d, z = make_rays(40, 70, 51, gpu)
    free = render_background(net, o, d, z=z)
    inf = render_background(net, o, d, z=z, t_stop=torch.full((40,), float('inf'), device=gpu))
    zero = render_background(net, o, d, z=z, t_stop=torch.zeros(40, device=gpu))
    for k in ('color', 'transmittance'):
        assert torch.equal(inf[k], free[k]), k
    assert bool((zero['color'] == 0).all())
    # rays whose samples are all inner: short rays through the centre
    S = 70
    oi = 0.2 * torch.nn.functional.normalize(o, dim=-1)
    zi = (torch.linspace(0.01, 0.6, S, device=gpu)[None, :] * torch.ones(40, 1, device=gpu)).contiguous()
    assert bool((torch.linalg.norm(oi[:, None, :] + d[:, None, :] * torch_mid(zi)[..., None], dim=-1) < 0.99).all())
    inner = render_background(net, oi, d, z=zi)
    assert bool((inner['color'] == 0).all())
    want = (1.0 + 1e-7) ** S
    err = float((inner['transmittance'].double() - want).abs().max() / max(1.0, want))
    print("all-inner transmittance error:", err, "bound:", BOUND['transmittance'])
    assert err <= BOUND['transmittance']
    for k in ('color', 'transmittance'):
        assert torch.equal(zero[k], render_background(net, o, d, z=z, t_stop=torch.full((40,), -1.0, device=gpu))[k])
    assert bool((zero['transmittance'] == inner['transmittance'][0]).all())      # the same S factors fl(1 + 1e-7)


def test_argument_errors(gpu, net):
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.background import render_background
    o, d, z = make_rays(6, 8, 61, gpu)
    for kw in (dict(z=z[:5]), dict(z=z.double()), dict(z=z.cpu()), dict(z=z, t_stop=torch.zeros(5, device=gpu)),
               dict(z=z[:, :0]), dict(n_samples=0)):
        with pytest.raises(NuNerfLibraryError):
            render_background(net, o, d, **kw)
    with pytest.raises(NuNerfLibraryError):
        render_background(net, o[:, :2], d, z=z)
    empty = render_background(net, o[:0], d[:0], z=z[:0])
    assert empty['color'].shape == (0, 3) and empty['transmittance'].shape == (0,)
    eng = net.engine()
    with pytest.raises(NuNerfLibraryError):            # the C entry's own checks
        eng.background(o.data_ptr(), 2, d.data_ptr(), 3, z, 6)
    with pytest.raises(NuNerfLibraryError):
        eng.lib.nu_background_fwd(None, o.data_ptr(), 3, d.data_ptr(), 3, z.data_ptr(), 8, None, 6, None, None, None, None, None, eng.stream())


@exact_fp32_only
def test_render_surface(gpu):
    """Test 6."""
    from nu_nerf_amd.relight import intrinsics, relighting_poses
    from nu_nerf_amd.sdf_trace import AOVS, BACKGROUND_AOVS, SHADING_AOVS
    net, _ = TE.stage1_net(gpu, False, gain=False)
    h, w = 40, 48
    K, pose = intrinsics(h, w), relighting_poses(4, 30.0, 35.0, 2.2)[1]
    old = AOVS + SHADING_AOVS
    base = net.render_surface(K, pose, h, w, aovs=old)
    both = net.render_surface(K, pose, h, w, aovs=old + BACKGROUND_AOVS)
    for a in old:
        assert torch.equal(both[a], base[a]), a
    mask = both['mask'] > 0
    assert 0.1 < float(mask.float().mean()) < 0.9
    bg, tr, rgb = both['background'], both['transmittance'], both['rgb']
    assert bg.shape == (h, w, 3) and tr.shape == (h, w) and both['frame'].shape == (h, w, 3)
    assert bool((bg[~mask].abs().sum(-1) > 0).all()) and float(bg[~mask].std()) > 1e-4
    m3 = mask[..., None]
    for white in (False, True):
        fr = net.render_surface(K, pose, h, w, aovs=('frame',), white_background=white)
        assert set(fr) == {'frame'}
        behind = torch.where(m3, tr[..., None] * rgb, tr[..., None].expand(h, w, 3) if white else torch.zeros_like(rgb))
        assert torch.equal(fr['frame'], torch.clamp(bg + behind, 0.0, 1.0)), white
    assert torch.equal(both['frame'], net.render_surface(K, pose, h, w, aovs='frame', white_background=bool(net.cfg['is_nerf']))['frame'])
    for chunk in (1, 97, 1000):
        part = net.render_surface(K, pose, h, w, aovs=('frame', 'background', 'transmittance', 'depth'), chunk=chunk)
        for a in part:
            assert torch.equal(part[a], both[a]), (a, chunk)
    # the stop is the hit's t: the background of a hit pixel is what lies in front of the surface
    from nu_nerf_amd.mask_render import pinhole_rays
    rays = pinhole_rays(torch.as_tensor(K, dtype=torch.float32).reshape(3, 3), torch.as_tensor(pose, dtype=torch.float32).reshape(1, 3, 4), h, w, gpu)
    stop = torch.where(mask.reshape(-1), both['depth'].reshape(-1), torch.full((h * w,), float('inf'), device=gpu))
    direct = net.render_background(rays[:, :3], rays[:, 3:], t_stop=stop)
    assert torch.equal(direct['color'].reshape(h, w, 3), bg) and torch.equal(direct['transmittance'].reshape(h, w), tr)


@exact_fp32_only
def test_stage2_renderer_evaluates_its_stage1_background(gpu):
    from nu_nerf_amd.background import render_background
    o, d, z = make_rays(50, 40, 71, gpu)
    for thick in (False, True):
        net2, _ = TE.stage2_net(gpu, thick=thick)
        a = net2.render_background(o, d, z=z)
        b = render_background(net2.stage1_network, o, d, z=z)
        for k in ('color', 'transmittance'):
            assert torch.equal(a[k], b[k]), (k, thick)
        assert float(a['color'].abs().sum()) > 0
