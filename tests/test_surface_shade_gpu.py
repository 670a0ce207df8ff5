"""The learned appearance at surface points on the GPU (csrc/surface_shade.hip, nu_nerf_amd/surface_shade.py, the shading AOVs of
render_surface): bit-identity with the layered path, the reference fixture, a float64 evaluation end to end, row independence, the
human-light rule, render_surface, the argument handling.

The bit contract as found on an MI355X: encoded rows, raw heads AND colour are the bits of the layered path
(nu_s2_shade_encode_fwd, the stacks, nu_shade_combine_fwd) -- no channel differs, so the colour is asserted exact too.

Bounds.  FIXTURE_RTOL / FIXTURE_ATOL: what tests/test_stage1_gpu.py asserts for the rows of the same fixture (ops.npz).  F64_BOUND (test 3):
four times the largest error of the EXISTING layered path (nets.sdf + shade) against tests/surface_shade_oracle.py on the test's own
4096 rows, relative to max(1, |ref|), per output; measured on an MI355X, never on the kernel under test.
"""
import functools

import numpy as np
import pytest
import torch

import surface_shade_oracle as SO
import test_environment_gpu as TE
from helpers import golden

pytestmark = pytest.mark.gpu

FIXTURE_RTOL, FIXTURE_ATOL = 1e-4, 2e-6
SIZES = (1, 31, 32, 33, 95, 2048)
# measured on the layered path (scripts/bench_surface_shade.py --errors prints them): largest error relative to max(1, |ref|) over the
# 4096 rows of test 3, and the asserted bound = 4 x that
LAYERED_ERR = {'rgb': 4.5e-06, 'diffuse_color': 8.2e-08, 'specular_color': 8.2e-06, 'diffuse_light': 4.7e-08, 'specular_light': 1.6e-05,
               'occ_prob': 5.8e-06, 'indirect_light': 2.9e-06, 'refraction_light': 5.8e-06, 'reflection_weight': 2.5e-06}
F64_BOUND = {k: 4.0 * v for k, v in LAYERED_ERR.items()}


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def rows(n, seed):
    """(points at radius 0.2 .. 0.95, view directions and normals of length 0.5 .. 2) float32 numpy [n,3] each."""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = (u * g.uniform(0.2, 0.95, (n, 1))).astype(np.float32)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)      # noqa: E731
    v = (unit(g.standard_normal((n, 3))) * g.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    nr = (unit(g.standard_normal((n, 3))) * g.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    return x, v, nr


class Case:
    """One network under test: the renderer, its network ops, shader config, FG table and the names of its parameters."""

    def __init__(self, gpu, kind, clamp=False):
        self.kind, self.which = kind, None
        self.sdf_prefix, self.prefix = 'sdf_network', 'color_network'
        over = None
        if kind in ('s1', 's1_sphere'):
            sphere = kind == 's1_sphere'
            base = TE.stage1_arrays(sphere)
            self.ocfg = {'light_exp_max': 3.0, 'sphere_direction': sphere, 'refrac_freq': 6}
            self.pos_freq, self.cap = 6, None
            if clamp:
                over = self._overrides(base)
            self.net, self.params = TE.stage1_net(gpu, sphere, over)
            from nu_nerf_amd.nets import Stage1Nets
            self.nets = Stage1Nets(self.net.engine(), self.net._named())
            self.scfg, self.lut = self.net.color_network.cfg, self.net.color_network.FG_LUT
        else:
            thick = kind == 's2_thick'
            self.which, self.sdf_prefix, self.prefix = 'inner', 'sdf_network_inner', 'color_network_inner'
            self.pos_freq, self.cap = (8, -0.2) if thick else (6, None)
            net0, base = TE.stage2_net(gpu, thick=thick)
            self.ocfg = {'light_exp_max': float(net0.color_network_inner.cfg['light_exp_max']), 'sphere_direction': False,
                         'refrac_freq': 2 if thick else 6}
            if clamp:
                over = self._overrides(base)
            self.net, self.params = TE.stage2_net(gpu, over, thick=thick)
            self.nets = self.net.nets()[1]
            self.scfg, self.lut = self.net.color_network_inner.cfg, self.net.color_network_inner.FG_LUT
        self.eng = self.nets.eng
        assert self.eng.light_pos_freq == self.pos_freq and self.eng.exp_max == self.ocfg['light_exp_max']
        assert self.eng.refrac_dim == 3 + 6 * self.ocfg['refrac_freq']
        assert float(self.scfg.get('refrac_exp_max', self.eng.exp_max)) == (self.cap if self.cap is not None else self.eng.exp_max)

    def _overrides(self, base):
        """Both sides of every clamp, from the float64 evaluation alone (surface_shade_oracle.clamp_overrides); the SpecInner network's
        refraction head straddles ITS cap (-0.2) instead of light_exp_max."""
        x, v, nr = rows(512, 77)
        feats, _ = SO.geometry64(base, x, self.sdf_prefix)
        over = SO.clamp_overrides(base, self.ocfg, x, nr, v, feats, self.prefix, self.pos_freq)
        if self.cap is not None:
            k = f'{self.prefix}.refrac_light.6.bias'
            over[k] = (over[k].astype(np.float64) - self.ocfg['light_exp_max'] + self.cap).astype(np.float32)
        return over

    def layered(self, x, v, nr):
        """The existing layered path on explicit rows: (encoded rows [P, 3 ld_ol + 352 + ld_rl], raw heads [P,20], colour [P,3], raw
        material heads [P,8]) in the kernel's test-output layouts."""
        from nu_nerf_amd import stage2_ops as O
        from nu_nerf_amd.shading_glue import shade
        n, nets, eng = x.shape[0], self.nets, self.eng
        with torch.no_grad():
            eng.pack()
            y, _ = nets.sdf(x)
            feats = y[:, 1:].contiguous()
            m_raw = nets.materials(feats, x)
            OL, IL, IW, RL, _, _ = O.shade_encode(eng, x, nr, v, m_raw, self.ocfg['sphere_direction'], self.pos_freq, self.ocfg['refrac_freq'])
            ol, il, iw, rl = nets.predictors(('outer_light', 'inner_light', 'inner_weight', 'refrac_light'), (OL, IL, IW, RL))
            col, _ = shade(nets, self.scfg, self.lut, x, nr, v, feats)
        enc = torch.cat([OL[:n], OL[n:2 * n], OL[2 * n:], IL[:n], IL[n:], IW, RL], 1)
        raw = torch.cat([ol[:n], ol[n:2 * n], ol[2 * n:], il[:n], il[n:], iw, rl, torch.zeros(n, 1, device=x.device)], 1)
        mr = torch.zeros(n, 8, device=x.device)
        mr[:, :6] = m_raw
        return enc, raw, col, mr


@functools.lru_cache(maxsize=None)
def case(gpu, kind, clamp=False):
    return Case(gpu, kind, clamp)


# ---- 1. the layered path, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ['s1', 's1_sphere', 's2_inner', 's2_thick'])
def test_bits_of_the_layered_path(gpu, kind):
    """sphere_direction off / on (stage 1), refrac_freq 6 / 2 with the SpecInner cap and light_pos_freq 6 / 8 (the inner networks of
    the two stage-2 models); heads moved so that the rows sit on both sides of every clamp."""
    from nu_nerf_amd.surface_shade import shade_points
    c = case(gpu, kind, True)
    for n in SIZES:
        x, v, nr = (dev(a, gpu) for a in rows(n, 100 + n))
        enc, raw, col, mr = c.layered(x, v, nr)
        out = shade_points(c.net, x, v, nr, which=c.which, _enc=True, _raw=True, _mraw=mr)
        assert torch.equal(out['enc'], enc), (kind, n)
        assert torch.equal(out['raw'], raw), (kind, n)
        assert torch.equal(out['rgb'], col), (kind, n, int((out['rgb'] != col).sum()))
        # the raw material heads of the fused bake are the layered ones, so the public call gives the same colour
        assert torch.equal(shade_points(c.net, x, v, nr, which=c.which)['rgb'], col), (kind, n)
        if n == 2048:
            r = raw.cpu().numpy()
            top, cap = c.eng.exp_max, (c.cap if c.cap is not None else c.eng.exp_max)
            sh = {'outer above': (r[:, 0:9] > top).any(1).mean(), 'outer below': (r[:, 0:9] < top).any(1).mean(),
                  'inner above': (r[:, 9:15] > top).any(1).mean(), 'inner below': (r[:, 9:15] < top).any(1).mean(),
                  'refraction above': (r[:, 16:19] > cap).any(1).mean(), 'refraction below': (r[:, 16:19] < cap).any(1).mean(),
                  'occ 0': (0.5 * r[:, 15] + 0.5 <= 0).mean(), 'occ 1': (0.5 * r[:, 15] + 0.5 >= 1).mean(),
                  'occ interior': ((0.5 * r[:, 15] + 0.5 > 0) & (0.5 * r[:, 15] + 0.5 < 1)).mean(),
                  'NoV < 0': float(((nr * v).sum(1) < 0).float().mean()), 'NoV > 0': float(((nr * v).sum(1) > 0).float().mean())}
            print(f"{kind}: shares of the rows on each side of the clamps: " + ', '.join(f'{k} {s:.2f}' for k, s in sh.items()))
            assert min(sh.values()) >= 0.1, sh
            lin = shade_points(c.net, x, v, nr, which=c.which, linear=True)['rgb']
            from nu_nerf_amd import torch_glue as G
            assert torch.allclose(G.linear_to_srgb(lin), col, rtol=1e-6, atol=1e-7) and not torch.equal(lin, col)


# ---- 2. the reference fixture -----------------------------------------------------------------------------------------------------
def test_reference_fixture(gpu):
    """The reference's own shading rows (ops.npz): raw material heads from the layered materials op on the fixture's features."""
    from nu_nerf_amd.surface_shade import shade_points
    from nu_nerf_amd.nets import Stage1Nets
    g = golden('ops.npz')
    net, _ = TE.stage1_net(gpu, False, gain=False)                   # the weights the fixture was recorded with
    eng = net.engine()
    x, nr, v, feats = (dev(g[k], gpu) for k in ('shade_pts', 'shade_nrm', 'shade_view', 'shade_feats'))
    P = x.shape[0]
    with torch.no_grad():
        eng.pack()
        mr = torch.zeros(P, 8, device=gpu)
        mr[:, :6] = Stage1Nets(eng, net._named()).materials(feats, x)
    out = shade_points(net, x, v, nr, terms=('occ_prob',), _enc=True, _mraw=mr)
    np.testing.assert_allclose(out['rgb'].cpu().numpy(), g['shade_color'], rtol=FIXTURE_RTOL, atol=FIXTURE_ATOL)
    np.testing.assert_allclose(out['occ_prob'].cpu().numpy().reshape(-1, 1), g['shade_occ_prob'].reshape(-1, 1), rtol=FIXTURE_RTOL, atol=FIXTURE_ATOL)
    # the reflective direction: the raw columns of the occlusion row's direction code (IWin = [pos_enc(x) 39 | embed(r, 6)])
    off = 3 * eng.ld_ol + 256 + 39
    np.testing.assert_allclose(out['enc'][:, off:off + 3].cpu().numpy(), g['shade_reflective'], rtol=FIXTURE_RTOL, atol=FIXTURE_ATOL)


# ---- 3. float64, end to end -------------------------------------------------------------------------------------------------------
def test_against_float64_end_to_end(gpu):
    """shade_points(renderer, x, v) with normals and materials from the fused kernels against the float64 wrapper on 4096 points; no
    row is left out.  Errors relative to max(1, |ref|), bounds F64_BOUND (four times the layered path's own error on these rows)."""
    from nu_nerf_amd.surface_shade import TERMS, shade_points
    c = case(gpu, 's1')
    x_np, v_np, _ = rows(4096, 4096)
    want = SO.shade64(c.params, c.ocfg, x_np, v_np)
    out = shade_points(c.net, dev(x_np, gpu), dev(v_np, gpu), terms=tuple(TERMS))
    worst = {}
    for k in F64_BOUND:
        mine = out[k].cpu().numpy().astype(np.float64)
        worst[k] = float((np.abs(mine - want[k]) / np.maximum(1.0, np.abs(want[k]))).max())
    print("shade_points vs float64 (4096 rows), largest error relative to max(1, |ref|): " + ', '.join(f'{k} {e:.3e}' for k, e in worst.items()))
    print("bounds (4 x the layered path): " + ', '.join(f'{k} {e:.3e}' for k, e in F64_BOUND.items()))
    for k, e in worst.items():
        assert e <= F64_BOUND[k], (k, e, F64_BOUND[k])


# ---- 4. independence --------------------------------------------------------------------------------------------------------------
def test_row_independence_bits(gpu):
    from nu_nerf_amd.surface_shade import TERMS, shade_points
    c = case(gpu, 's1_sphere', True)
    n = 95
    x, v, nr = (dev(a, gpu) for a in rows(n, 2031))
    cat = lambda o: torch.cat([o[k].reshape(o[k].shape[0], -1) for k in ('rgb',) + tuple(TERMS)], 1)      # noqa: E731
    run = lambda x, v, nr: cat(shade_points(c.net, x, v, nr, terms=tuple(TERMS)))      # noqa: E731
    full = run(x, v, nr)
    assert full.shape == (n, 23) and bool(torch.isfinite(full).all())
    assert torch.equal(run(x, v, nr), full)                                          # two runs
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).permutation(n)).to(gpu)
    assert torch.equal(run(x[perm].contiguous(), v[perm].contiguous(), nr[perm].contiguous()), full[perm])
    for k in (1, 31, 32, 33):                                                         # prefixes
        assert torch.equal(run(x[:k], v[:k], nr[:k]), full[:k]), k
    for i in (0, 31, 32, 94):                                                         # a row alone
        assert torch.equal(run(x[i:i + 1].contiguous(), v[i:i + 1].contiguous(), nr[i:i + 1].contiguous()), full[i:i + 1]), i
    wide = torch.full((n, 11), 7.0, device=gpu)                                       # other leading dimensions: 11, 5 and 4 floats
    wide[:, 0:3], wide[:, 4:7] = x, v
    five = torch.full((n, 5), -3.0, device=gpu)
    five[:, 1:4] = nr
    assert torch.equal(run(wide[:, 0:3], wide[:, 4:7], five[:, 1:4]), full)
    four = torch.zeros(n, 4, device=gpu)
    four[:, :3] = x
    assert torch.equal(run(four, v, nr), full)                                        # columns past the third are not read
    # more tiles than workgroups: the grid-stride tail (258 tiles on at most 256 workgroups) repeats the rows' bits
    reps = 87
    big = run(x.repeat(reps, 1), v.repeat(reps, 1), nr.repeat(reps, 1))
    assert big.shape[0] == 8265 and torch.equal(big, full.repeat(reps, 1))


# ---- 5. the human light -----------------------------------------------------------------------------------------------------------
def test_human_light_model_is_shaded_without_the_photographer(gpu):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.surface_shade import TERMS, shade_points
    arrays = randomize_for_parity(init_stage1_params(6033, human_light=True), seed=1)
    on = NeROShapeRenderer({'name': 'hl', 'shader_config': {'human_light': True}}, training=False)
    on.load_param_dict(arrays)
    off = NeROShapeRenderer({'name': 'hl', 'shader_config': {'human_light': False}}, training=False)
    off.load_param_dict({k: a for k, a in arrays.items() if 'human_light_predictor' not in k})
    on, off = on.to(gpu), off.to(gpu)
    assert on.engine().human_light and not off.engine().human_light
    x, v, nr = (dev(a, gpu) for a in rows(97, 2032))
    a, b = shade_points(on, x, v, terms=tuple(TERMS)), shade_points(off, x, v, terms=tuple(TERMS))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(on.shade_points(x, v, nr)['rgb'], shade_points(off, x, v, nr)['rgb'])


# ---- 6. render_surface ------------------------------------------------------------------------------------------------------------
def test_render_surface_rgb(gpu):
    from nu_nerf_amd import torch_glue as G
    from nu_nerf_amd.relight import intrinsics, relighting_poses
    from nu_nerf_amd.sdf_trace import AOVS, SHADING_AOVS
    from nu_nerf_amd.surface_shade import TERMS, shade_points
    net, _ = TE.stage1_net(gpu, False, gain=False)
    h, w = 40, 48
    K, pose = intrinsics(h, w), relighting_poses(4, 30.0, 35.0, 2.2)[1]
    base = net.render_surface(K, pose, h, w, aovs=AOVS)
    both = net.render_surface(K, pose, h, w, aovs=AOVS + SHADING_AOVS)
    for a in AOVS:                                                       # existing AOVs: the same bits next to the shading AOVs
        assert torch.equal(both[a], base[a]), a
    mask = both['mask'] > 0
    assert 0.1 < float(mask.float().mean()) < 0.9
    from nu_nerf_amd.mask_render import pinhole_rays
    rays = pinhole_rays(torch.as_tensor(K, dtype=torch.float32).reshape(3, 3), torch.as_tensor(pose, dtype=torch.float32).reshape(1, 3, 4), h, w, gpu)
    idx = mask.reshape(-1).nonzero().reshape(-1)
    sh = shade_points(net, both['position'].reshape(-1, 3)[idx].contiguous(), -rays[idx, 3:6], terms=tuple(TERMS))
    for a in SHADING_AOVS:
        img = both[a]
        assert img.shape == ((h, w, 3) if a == 'rgb' or TERMS.get(a) == 3 else (h, w)) and img.dtype == torch.float32
        assert bool((img[~mask] == 0).all()), a
        want = sh['rgb' if a == 'rgb' else a]
        want = torch.clamp(G.linear_to_srgb(want) if a in ('diffuse_light', 'specular_light') else want, 0.0, 1.0)
        assert torch.equal(img[mask].reshape(want.shape), want), a
        assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    assert float(both['rgb'][mask].std()) > 1e-3
    for chunk in (1, 97, 1000):
        part = net.render_surface(K, pose, h, w, aovs=('rgb', 'occ_prob', 'depth'), chunk=chunk)
        for a in part:
            assert torch.equal(part[a], both[a]), (a, chunk)
    only = net.render_surface(K, pose, h, w, aovs='rgb')
    assert set(only) == {'rgb'} and torch.equal(only['rgb'], both['rgb'])


def test_render_surface_command_writes_rgb(gpu, tmp_path, monkeypatch, capsys):
    import json
    import os
    import yaml
    from nu_nerf_amd import render_surface as R
    from nu_nerf_amd.mask_render import _pillow
    net, _ = TE.stage1_net(gpu, False, gain=False)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    torch.save({'step': 77, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 'data/model/tiny/model.pth')
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = R.main(['--cfg', 'tiny.yaml', '--hw', '24', '--num', '1', '--cam_dist', '2.2', '--aovs', 'rgb', 'specular_light', 'occ_prob'])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['aovs'] == ['rgb', 'specular_light', 'occ_prob'] and line['hit'][0] > 0
    assert sorted(os.listdir(out)) == ['0_occ_prob.png', '0_rgb.png', '0_specular_light.png']
    rgb = np.asarray(_pillow().open(os.path.join(out, '0_rgb.png')))
    assert rgb.shape == (24, 24, 4) and int((rgb[..., 3] == 255).sum()) == line['hit'][0] and rgb[..., :3][rgb[..., 3] == 0].max(initial=0) == 0
    assert np.asarray(_pillow().open(os.path.join(out, '0_specular_light.png'))).shape == (24, 24, 3)
    assert np.asarray(_pillow().open(os.path.join(out, '0_occ_prob.png'))).shape == (24, 24)


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    import ctypes
    from nu_nerf_amd._lib import NU_SHADE_LINEAR, NuNerfLibraryError
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.surface_shade import shade_points
    c = case(gpu, 's1')
    net, eng = c.net, c.eng
    n = 33
    x, v, nr = (dev(a, gpu) for a in rows(n, 2033))
    ref = shade_points(net, x, v, nr, terms=('occ_prob',))
    # empty input: empty tensors of the right shapes, no launch
    empty = shade_points(net, x[:0], v[:0], nr[:0], terms=('occ_prob', 'diffuse_color'), _enc=True, _raw=True)
    assert {k: tuple(t.shape) for k, t in empty.items()} == {'rgb': (0, 3), 'occ_prob': (0,), 'diffuse_color': (0, 3), 'enc': (0, 736), 'raw': (0, 20)}
    assert tuple(shade_points(net, x[:0], v[:0])['rgb'].shape) == (0, 3)
    # wrong type, dtype, shape, device, strides or row count raise before the call
    for bad in (x.cpu().numpy(), x.double(), x.half(), x[:, :2].contiguous(), x.reshape(-1), x.t().contiguous().t(), x.cpu(), x[:-1].contiguous()):
        with pytest.raises(NuNerfLibraryError, match=r"nu_surface_shade_fwd failed with code -1"):
            shade_points(net, x, bad, nr)
        with pytest.raises(NuNerfLibraryError, match=r"nu_surface_shade_fwd failed with code -1"):
            shade_points(net, x, v, bad)
    for bad in (x.double(), x[:, :2].contiguous(), x.cpu(), x.t().contiguous().t()):
        with pytest.raises(NuNerfLibraryError, match=r"nu_surface_shade_fwd failed with code -1"):
            shade_points(net, bad, v, nr)
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        shade_points(net, x, v, nr, _mraw=torch.zeros(n, 5, device=gpu))
    with pytest.raises(ValueError):
        shade_points(net, x, v, nr, terms=('rgb',))
    with pytest.raises(ValueError):
        shade_points(net, x, v, nr, terms=('human_light',))
    with pytest.raises(ValueError):
        shade_points(net, x, v, nr, which='inner')
    with pytest.raises(ValueError):
        shade_points(net, x, v, nr, which='middle')
    # the C entry: every NU_ERR_ARG case
    eng.pack()
    lib, sn, S = eng.lib, ctypes.byref(eng._shade_net), eng.stream()
    mr = c.layered(x, v, nr)[3]
    color = torch.full((n, 3), -7.0, device=gpu)
    ok = dict(net=sn, X=addr(x), x_ld=3, V=addr(v), v_ld=3, N=addr(nr), n_ld=3, M=addr(mr), ldm=8, P=n, pf=6, cap=eng.exp_max, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nu_surface_shade_fwd(a['net'], a['X'], a['x_ld'], a['V'], a['v_ld'], a['N'], a['n_ld'], a['M'], a['ldm'], a['P'], a['pf'],
                                        a['cap'], a['flags'], addr(color), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, S)
    for kw in (dict(net=None), dict(X=0), dict(V=0), dict(N=0), dict(M=0), dict(P=-1), dict(x_ld=2), dict(v_ld=2), dict(n_ld=0), dict(ldm=5),
               dict(flags=2), dict(flags=NU_SHADE_LINEAR | 4), dict(pf=9), dict(pf=-1), dict(pf=8), dict(pf=5)):
        with pytest.raises(NuNerfLibraryError, match=r"nu_surface_shade_fwd failed with code -1"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((color == -7.0).all())                                     # nothing was launched
    assert call(P=0) == 0
    torch.cuda.synchronize()
    assert bool((color == -7.0).all())                                     # P = 0 returns at once
    assert call() == 0                                                     # every other output may be NULL
    torch.cuda.synchronize()
    assert torch.equal(color, ref['rgb'])
    # a shading table that is not the network's: refused, not read
    broken = type(eng._shade_net).from_buffer_copy(eng._shade_net)
    broken.ld_rl = 64
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        call(net=ctypes.byref(broken))
    broken = type(eng._shade_net).from_buffer_copy(eng._shade_net)
    broken.lut = None
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        call(net=ctypes.byref(broken))


def test_every_renderer_class_and_which(gpu):
    from nu_nerf_amd.renderer_std import NeROShapeRenderer as StdRenderer
    from nu_nerf_amd.surface_shade import shade_points
    x, v, nr = (dev(a, gpu) for a in rows(97, 2034))
    net1, _ = TE.stage1_net(gpu, False, gain=False)
    ref = net1.shade_points(x, v)['rgb']
    for thick in (False, True):
        net2, _ = TE.stage2_net(gpu, thick=thick)
        assert torch.equal(net2.shade_points(x, v, which='outer')['rgb'], ref)
        inner = net2.shade_points(x, v)['rgb']                                  # the default of a stage-2 renderer: its inner networks
        assert torch.equal(inner, shade_points(net2, x, v, which='inner')['rgb'])
        assert not torch.equal(inner, ref) and bool(torch.isfinite(inner).all())
    std, _ = TE.stage1_net(gpu, False, gain=False, cls=StdRenderer, cfg={'is_nerf': False})
    assert torch.equal(std.shade_points(x, v)['rgb'], ref)
    for md in ('bf16', 'bf16x6'):                                               # the kernel reads the fp32 tables in every mlp_dtype
        net16, _ = TE.stage1_net(gpu, False, gain=False, cfg={'mlp_dtype': md})
        assert torch.equal(net16.shade_points(x, v)['rgb'], ref), md
