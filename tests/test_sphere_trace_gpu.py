"""Fused SDF sphere tracing on the GPU (csrc/sdf_trace.hip, nu_nerf_amd/sdf_trace.py): the bits of the composition a user could build
from sdf_forward + torch, independence of slot / neighbours / order / count, a float64 oracle (tests/sphere_trace_oracle.py), a plane
with a closed form, the edges of the C entry, the mesh pipeline, and render_surface.

Ray set: the 2048 standard rays of tests/sphere_trace_oracle.py (origins at radius 3, aimed at targets of radius <= 1.1), bounding radius 1,
threshold 1e-5, 200 iterations.  On it the float64 oracle gives, init / parity network: 1989 / 1989 rays enter the sphere, 1100 / 1080 hit,
1 / 1 reach max_iter, a hit takes 4 .. 175 / 4 .. 128 evaluations (median 11 / 10).

Bounds (test 3, also used by test 4).  Each is four times the largest error measured on an MI355X against the float64 oracle (never
against the kernel itself; run to run there is no spread, the kernel returns the composition's bits), over the rays that hit in both, on
the init network, the parity network and the stage-2 inner network, capped at 1e-4.  Measured (init / parity / inner) / bound / cap:
    pos        8.013e-6 / 6.556e-6 / 5.697e-6   3.21e-5   1e-4       max |pos - pos64|
    residual   9.770e-6 / 9.763e-6 / 9.736e-6   3.91e-5   1e-4       max |f64(pos)| at the kernel's hit points (the threshold is 1e-5)
Hit flags differed from the oracle's on 0 / 0 / 0 rays (allowed: 0.5 % of the 1989 rays that entered); iteration counts were equal on
99.64 / 99.44 / 99.17 % of the common hits and never more than 1 apart (required: 95 %, 1).
Test 6: against the 64^3 marching-cubes mesh of the init network, 1059 rays hit both with |n.d| >= 0.3 and differ by at most 2.644e-3 in t
(allowed: one voxel, 2 / 63 = 3.17e-2); the masks of the SDF trace and of the mesh differed on 0.05 % of the 2048 rays, those of the
float64 oracle and the mesh on 0.05 % (allowed: 3 %)."""
import ctypes

import numpy as np
import pytest
import torch

import curvature_oracle as CO
import sphere_trace_oracle as SO

pytestmark = pytest.mark.gpu

TM = 64                                              # ray slots per workgroup of sdf_trace_kernel
BOUND = {'pos': 3.21e-5, 'residual': 3.91e-5}
CAP = {'pos': 1e-4, 'residual': 1e-4}
assert all(BOUND[k] <= CAP[k] for k in CAP)
KEYS = ('pos', 't', 'sdf', 'iters', 'hit')
MAX_ITERS = (1, 2, 7, 200)


# ---- the networks of tests/test_curvature_gpu.py ---------------------------------------------------------------------------------
def stage1_arrays(init_only=False):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = init_stage1_params(6033)
    return arrays if init_only else randomize_for_parity(arrays, seed=1)


def stage1_net(gpu, overrides=None, init_only=False):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    arrays = stage1_arrays(init_only)
    arrays.update(overrides or {})
    net = NeROShapeRenderer({'name': 'golden'}, training=False)
    net.load_param_dict(arrays)
    return net.to(gpu), arrays


def stage2_net(gpu):
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, randomize_for_parity
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.stage2 import Stage2Renderer
    s1 = randomize_for_parity(init_stage1_params(6033), seed=1)
    s1cfg = {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000}
    cfg = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'shader_config': {'sphere_direction': False, 'human_light': False},
           'stage1_cfg': s1cfg, 'stage1_mesh_arrays': icosphere(3, 0.5)}
    net = Stage2Renderer(cfg, training=False)
    p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
    sd = net.state_dict()
    for k in [k for k in p2 if k.startswith('stage1_network.')]:      # the aliases of the same tensors, where the model has them
        if 'color_network.' + k in sd:
            p2['color_network.' + k] = p2[k]
    net.load_param_dict(p2)
    return net.to(gpu), p2


def trace(net, o, d, **kw):
    from nu_nerf_amd.sdf_trace import trace_rays
    return trace_rays(net, o, d, **kw)


def rows(out, idx):
    """The rows idx (an index tensor or a slice) of every output."""
    return {k: out[k][idx] for k in KEYS}


def same(a, b):
    """Equal bits of every output."""
    bits = lambda v: v.contiguous().view(torch.int32) if v.dtype == torch.float32 else v      # noqa: E731
    return all(a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])) for k in KEYS)


@pytest.fixture(scope='module')
def rays(gpu):
    o, d = SO.standard_rays()
    return torch.from_numpy(o).to(gpu), torch.from_numpy(d).to(gpu)


@pytest.fixture(scope='module')
def models(gpu):
    """name -> (net, `which`, arrays, the oracle's parameter prefix): built once."""
    init, init_arrays = stage1_net(gpu, init_only=True)
    parity, parity_arrays = stage1_net(gpu)
    s2, p2 = stage2_net(gpu)
    return {'init': (init, None, init_arrays, 'sdf_network'), 'parity': (parity, None, parity_arrays, 'sdf_network'),
            'inner': (s2, 'inner', p2, 'sdf_network_inner')}


@pytest.fixture(scope='module')
def full(gpu, rays, models):
    """name -> the kernel's outputs on the standard rays (200 iterations): computed once, never modified."""
    return {name: trace(net, *rays, which=which) for name, (net, which, _, _) in models.items()}


@pytest.fixture(scope='module')
def oracle64(gpu, rays, models):
    """name -> the float64 oracle on the standard rays: computed once, never modified."""
    o, d = rays
    return {name: SO.trace(SO.sdf_fn(arrays, prefix, device=gpu), o.cpu().numpy(), d.cpu().numpy(), device=gpu)
            for name, (_, _, arrays, prefix) in models.items()}


# ---- 1. the bits of the composition ----------------------------------------------------------------------------------------------------
def f32(v):
    return np.float32(v)


def entry_np(o, d, rb, entry_forward=False):
    """(x, t0, bounded) of the bounding-sphere entry in numpy float32, one rounding per operation, in the stated order."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]      # noqa: E731
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        a = dot(d, d)
        b = f32(2) * dot(d, o)
        c = dot(o, o) - f32(rb) * f32(rb)
        disc = b * b - (f32(4) * a) * c
        bounded = disc >= 0
        t0 = (-b - np.sqrt(disc)) / (f32(2) * a)
        if entry_forward:
            t0 = np.maximum(t0, f32(0))
        x = o + d * t0[:, None]
    assert all(v.dtype == np.float32 for v in (a, b, c, disc, t0, x))
    return x, t0, bounded


def composition(eng, o, d, *, max_iter, threshold=1e-5, rb=1.0, entry_forward=False, fg=None):
    """What a user could build without the kernel: the entry in numpy float32, then a device loop of the fused forward on ALL rays
    (eng.sdf_forward(keep=False, want_feat=False)) and the update in separate torch mul / add ops under per-ray masks."""
    from nu_nerf_amd.engine import addr
    dev, R = o.device, o.shape[0]
    on, dn = o.cpu().numpy(), d.cpu().numpy()
    fgr = np.isfinite(on).all(1)
    if fg is not None:
        fgr &= fg.cpu().numpy().astype(bool)
    x, t = on.copy(), np.zeros(R, np.float32)
    if rb > 0:
        xe, t0, bounded = entry_np(on, dn, rb, entry_forward)
        fgr &= bounded
        x, t = np.where(fgr[:, None], xe, on), np.where(fgr, t0, f32(0))
    x, t = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
    fgr = torch.from_numpy(fgr).to(dev)
    live = fgr.clone()
    iters = torch.zeros(R, dtype=torch.int32, device=dev)
    last = torch.zeros(R, device=dev)
    conv = torch.zeros(R, dtype=torch.bool, device=dev)
    thr, rbt = torch.tensor(threshold, dtype=torch.float32, device=dev), torch.tensor(rb, dtype=torch.float32, device=dev)
    for i in range(max_iter):
        if not bool(live.any()):
            break
        x = x.contiguous()
        s = eng.sdf_forward(addr(x), 3, R, keep=False, want_feat=False)['sdf']
        s = torch.nan_to_num(torch.clamp(s, -10.0, 10.0), nan=10.0)
        xn = torch.add(x, torch.mul(d, s[:, None]))
        tn = torch.add(t, s)
        if rb > 0:
            q = torch.mul(xn, xn)
            inside = torch.sqrt(torch.add(torch.add(q[:, 0], q[:, 1]), q[:, 2])) < rbt
        else:
            inside = torch.ones_like(live)
        c = s.abs() < thr
        x = torch.where(live[:, None], xn, x)
        t = torch.where(live, tn, t)
        last = torch.where(live, s, last)
        iters = torch.where(live, torch.full_like(iters, i + 1), iters)
        fgr = torch.where(live, inside, fgr)
        conv = torch.where(live, c, conv)
        live = live & inside & ~c
    return {'pos': x, 't': t, 'sdf': last, 'iters': iters, 'hit': (conv & fgr).to(torch.uint8)}


@pytest.mark.parametrize('name', ['init', 'parity', 'inner'])
def test_bits_against_the_composition(gpu, rays, models, full, name):
    from nu_nerf_amd.materials import bake_engine
    net, which, _, _ = models[name]
    eng = bake_engine(net, which)
    eng.pack()
    o, d = rays
    for max_iter in MAX_ITERS:
        want = composition(eng, o, d, max_iter=max_iter)
        got = full[name] if max_iter == 200 else trace(net, o, d, which=which, max_iter=max_iter)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (max_iter, k)
            ne = (got[k] != want[k]) & ~((got[k] != got[k]) & (want[k] != want[k]))
            assert not bool(ne.any()), (name, max_iter, k, int(ne.sum()))
        assert same(got, want), (name, max_iter)
        n_hit, n_it = int(got['hit'].sum()), int(got['iters'].sum())
        print(f"{name} max_iter {max_iter}: hit {n_hit}  traced {int((got['iters'] > 0).sum())}  evaluations {n_it}")
        assert int(got['iters'].max()) == max_iter or max_iter == 200
    # the ray set exercises hits and misses alike (a quarter to three quarters of the rays hit), and rays that never enter the sphere
    assert 512 < int(full[name]['hit'].sum()) < 1536 and int((full[name]['iters'] == 0).sum()) > 20


# ---- 2. independence -------------------------------------------------------------------------------------------------------------------
def test_independence_bits(gpu, rays, models, full):
    net, which, _, _ = models['parity']
    ref = full['parity']
    o, d = rays
    R = o.shape[0]
    assert same(trace(net, o, d), ref)                                   # two runs, equal bits
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(R)).to(gpu)
    assert same(trace(net, o[perm].contiguous(), d[perm].contiguous()), rows(ref, perm))
    rolled = torch.roll(torch.arange(R, device=gpu), 1)                  # every ray in the next workgroup (rays go round-robin), the last in the first
    assert same(trace(net, o[rolled].contiguous(), d[rolled].contiguous()), rows(ref, rolled))
    for n in (1, TM - 1, TM, TM + 1, 2 * TM + 1):                        # a prefix of the batch is the batch's prefix
        assert same(trace(net, o[:n].contiguous(), d[:n].contiguous()), rows(ref, slice(0, n))), n
    hit, it = ref['hit'].bool(), ref['iters']
    a_hit = int(hit.nonzero()[0])
    a_miss = int((~hit & (it > 0)).nonzero()[0])
    slowest = int(it.argmax())
    never = int((it == 0).nonzero()[0])
    assert int(it[slowest]) > 100
    for i in (a_hit, a_miss, slowest, never):                           # a ray alone against the same ray inside 2048
        assert same(trace(net, o[i:i + 1].contiguous(), d[i:i + 1].contiguous()), rows(ref, slice(i, i + 1))), i
    for pos in (0, 1, TM - 1, TM):                                       # the slowest ray in other slots, among other neighbours
        oo, dd = o[100:100 + TM + 1].clone(), d[100:100 + TM + 1].clone()
        oo[pos], dd[pos] = o[slowest], d[slowest]
        out = trace(net, oo, dd)
        assert all(torch.equal(out[k][pos], ref[k][slowest]) for k in KEYS), pos
    wide = torch.full((R, 8), float('nan'), device=gpu)                  # leading dimension 8, both in one matrix: the other columns are never read
    wide[:, :3], wide[:, 3:6] = o, d
    assert same(trace(net, wide[:, :3], wide[:, 3:6]), ref)
    ones = torch.ones(R, dtype=torch.bool, device=gpu)
    assert same(trace(net, o, d, mask=ones), ref) and same(trace(net, o, d, mask=ones.to(torch.uint8)), ref)


def test_refill_bits_on_a_large_batch(gpu, models):
    """The grid is min(ceil(R / 64), 256) workgroups and ray q G + b is the q-th of workgroup b, so up to 16 384 rays every workgroup loads its
    whole sequence in its first pass.  49 999 rays give each of the 256 workgroups 195 or 196 rays for its 64 slots: slots are retired and
    refilled while their neighbours march (partly free tiles, the sequence running out in mid-march).  Bits against the composition,
    against a permuted run and against prefixes whose rays meet other workgroups, slots and neighbours."""
    from nu_nerf_amd.materials import bake_engine
    net, which, _, _ = models['parity']
    eng = bake_engine(net, which)
    eng.pack()
    R = 49999
    o, d = (torch.from_numpy(v).to(gpu) for v in SO.standard_rays(R, seed=21))
    ref = trace(net, o, d)
    it = ref['iters']
    assert int((it > 0).sum()) > 2 * TM * 256                            # the traced rays exceed the launch's 256 x 64 slots more than twice over
    assert int(it.max()) == 200 and int((it == 0).sum()) > 500 and 0.25 * R < int(ref['hit'].sum()) < 0.75 * R
    assert same(ref, composition(eng, o, d, max_iter=200))
    assert same(trace(net, o, d), ref)
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).permutation(R)).to(gpu)
    assert same(trace(net, o[perm].contiguous(), d[perm].contiguous()), rows(ref, perm))
    for n in (TM * 256 + 1, 30011):                                     # other grids / sequences: 65 and 118 rays per workgroup
        assert same(trace(net, o[:n].contiguous(), d[:n].contiguous()), rows(ref, slice(0, n))), n
    short = trace(net, o, d, max_iter=7)                                 # every slot retires at once at pass 7, 14, ..: whole-tile refills
    assert same(short, composition(eng, o, d, max_iter=7))
    fg = torch.from_numpy(np.random.Generator(np.random.PCG64(6)).random(R) < 0.5).to(gpu)
    assert same(trace(net, o, d, mask=fg), composition(eng, o, d, max_iter=200, fg=fg))     # half the sequence is retired inside the refill loop


# ---- 3. float64 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['init', 'parity', 'inner'])
def test_float64_oracle(gpu, models, full, oracle64, name):
    _, _, arrays, prefix = models[name]
    got, ref = full[name], oracle64[name]
    hit, hit64 = got['hit'].cpu().numpy().astype(bool), ref['hit']
    entered = ref['entered']
    mism = int((hit != hit64).sum())
    both = hit & hit64
    pos = got['pos'].cpu().numpy().astype(np.float64)
    e_pos = float(np.abs(pos[both] - ref['pos'][both]).max())
    f64 = SO.sdf_fn(arrays, prefix, device=gpu)
    e_res = float(f64(torch.from_numpy(pos[hit]).to(gpu)).abs().max())
    di = np.abs(got['iters'].cpu().numpy()[both].astype(np.int64) - ref['iters'][both])
    print(f"sphere trace vs float64 ({name}): entered {int(entered.sum())} (kernel {int((got['iters'] > 0).sum())})  hit {int(hit.sum())} (oracle {int(hit64.sum())})  flag mismatches {mism}"
          f"  pos {e_pos:.3e}  residual {e_res:.3e}  iters equal {float((di == 0).mean()):.4f} max diff {int(di.max())}"
          f"  max_iter rays {int((ref['iters'] == 200).sum())}  iters of a hit {int(ref['iters'][hit64].min())} .. {int(ref['iters'][hit64].max())}")
    assert mism <= 0.005 * entered.sum()
    assert e_pos <= BOUND['pos'] and e_res <= BOUND['residual']
    assert (di == 0).mean() >= 0.95 and di.max() <= 1


# ---- 4. closed form: a plane -------------------------------------------------------------------------------------------------------------
PLANE_A = np.array([0.6, -0.48, 0.64])
PLANE_B = 0.15


def plane_net(gpu):
    """The pass-through network of tests/curvature_oracle.py with head weights on the three linear embedding columns only: f = a.x + b."""
    A, B = np.zeros(39, np.float32), np.zeros(39, np.float32)
    A[:3] = PLANE_A
    template = stage1_arrays()
    over = CO.analytic_overrides(A, B, template)
    over['sdf_network.lin8.bias'] = over['sdf_network.lin8.bias'].copy()
    over['sdf_network.lin8.bias'].reshape(-1)[0] += np.float32(PLANE_B)
    return stage1_net(gpu, over)[0]


def plane_rays(n, seed, lo, hi):
    """n rays from origins of radius <= 0.1 (so that f0 = a.o + b lies in 0.05 .. 0.25) whose a.d is uniform in [lo, hi] (float64; a = PLANE_A / |PLANE_A|)."""
    g = np.random.Generator(np.random.PCG64(seed))
    a = PLANE_A / np.linalg.norm(PLANE_A)
    o = g.standard_normal((n, 3))
    o *= g.uniform(0.0, 0.1, (n, 1)) / np.linalg.norm(o, axis=1, keepdims=True)
    c = g.uniform(lo, hi, n)
    p = g.standard_normal((n, 3))
    p -= (p @ a)[:, None] * a
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    d = c[:, None] * a + np.sqrt(1.0 - c * c)[:, None] * p
    return o.astype(np.float32), d.astype(np.float32)


def test_closed_form_plane(gpu):
    net = plane_net(gpu)
    a = PLANE_A.astype(np.float32).astype(np.float64)                   # the head's weights (|a| = 1 up to float32 rounding)
    o, d = plane_rays(64, 11, -1.0, -0.6)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    ad, f0 = d64 @ a, o64 @ a + PLANE_B
    assert (f0 > 0).all() and (ad <= -0.59).all()
    ot, dt = torch.from_numpy(o).to(gpu), torch.from_numpy(d).to(gpu)
    out = trace(net, ot, dt, bound_radius=0.0)
    assert bool(out['hit'].all())
    want = o64 - d64 * (f0 / ad)[:, None]
    # the march stops with |s| < 1e-5 and then steps by s: it ends |s (1 + a.d) / (a.d)| <= 1e-5 * 0.4 / 0.6 from the plane along the ray
    err = float(np.abs(out['pos'].cpu().numpy() - want).max())
    print(f"plane: max |pos - closed form| {err:.3e}  iters {int(out['iters'].min())} .. {int(out['iters'].max())}")
    assert err <= BOUND['pos']
    assert float(np.abs(out['t'].cpu().numpy() - (-f0 / ad)).max()) <= BOUND['pos']
    for k in (1, 2, 3):                                                  # sdf_last = f0 (1 + a.d)^(k - 1) at the k-th evaluation
        part = trace(net, ot, dt, bound_radius=0.0, max_iter=k)
        at_k = (part['iters'] == k).cpu().numpy()
        assert at_k.sum() >= 32
        s_err = float(np.abs(part['sdf'].cpu().numpy() - f0 * (1.0 + ad) ** (k - 1))[at_k].max())
        print(f"plane: max |sdf_last - f0 (1 + a.d)^{k - 1}| {s_err:.3e} on {int(at_k.sum())} rays")
        assert s_err <= BOUND['residual']
    # a.d >= 0: the ray moves away from (or along) the plane, never hits and stops at max_iter (three steps of at most 0.25 * 1.5^i keep
    # every point where the pass-through layers are exact: no coordinate below -1.8)
    o2, d2 = plane_rays(64, 12, 0.0, 0.5)
    out = trace(net, torch.from_numpy(o2).to(gpu), torch.from_numpy(d2).to(gpu), bound_radius=0.0, max_iter=3)
    assert not bool(out['hit'].any()) and bool((out['iters'] == 3).all())
    assert bool((out['sdf'] > 0).all())


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges(gpu, rays, models, full):
    from nu_nerf_amd._lib import NU_TRACE_ENTRY_FORWARD, NuNerfLibraryError
    from nu_nerf_amd.engine import addr
    net, _, _, _ = models['parity']
    ref = full['parity']
    eng = net.engine()
    eng.pack()
    o, d = rays
    n = 200
    # never foreground: a NaN origin, an fg entry of 0, a ray that misses the sphere
    oo, dd = o[:n].clone(), d[:n].clone()
    fg = torch.ones(n, dtype=torch.bool, device=gpu)
    hits = ref['hit'][:n].bool().nonzero().reshape(-1)
    i_nan, i_fg, i_miss = int(hits[0]), int(hits[1]), int(hits[2])
    oo[i_nan, 1] = float('nan')
    fg[i_fg] = False
    side = torch.linalg.cross(o[i_miss], torch.tensor([0.0, 0.0, 1.0], device=gpu))
    dd[i_miss] = side / side.norm()                                      # at right angles to the origin's direction: passes the sphere at distance 3
    out = trace(net, oo, dd, mask=fg)
    for i in (i_nan, i_fg, i_miss):
        assert torch.equal(out['pos'][i].view(torch.int32), oo[i].view(torch.int32)), i
        assert int(out['iters'][i]) == 0 and int(out['hit'][i]) == 0 and float(out['t'][i]) == 0 and float(out['sdf'][i]) == 0, i
    others = torch.ones(n, dtype=torch.bool, device=gpu)
    others[[i_nan, i_fg, i_miss]] = False
    keep = others.nonzero().reshape(-1)
    assert same(rows(out, keep), rows(ref, keep))                        # the others do not notice
    assert same(out, composition(eng, oo, dd, max_iter=200, fg=fg))
    # no bounding sphere: every finite ray is traced from its origin
    free = trace(net, o[:n], d[:n], bound_radius=0.0, max_iter=20)
    assert same(free, composition(eng, o[:n], d[:n], max_iter=20, rb=0.0)) and bool((free['iters'] > 0).all())
    assert same(free, trace(net, o[:n], d[:n], bound_radius=None, max_iter=20))
    # an origin inside the sphere: with NU_TRACE_ENTRY_FORWARD it starts there, without it steps back to the sphere's entry point
    oi = (0.4 * o[:n] / 3.0).contiguous()
    fwd = trace(net, oi, d[:n], entry_forward=True, max_iter=1)
    back = trace(net, oi, d[:n], entry_forward=False, max_iter=1)
    assert same(fwd, composition(eng, oi, d[:n], max_iter=1, entry_forward=True))
    assert same(back, composition(eng, oi, d[:n], max_iter=1, entry_forward=False))
    first = eng.sdf_forward(addr(oi), 3, n, keep=False, want_feat=False)['sdf']
    assert torch.equal(fwd['sdf'], first) and torch.equal(fwd['t'], first)          # t = 0 + f(o)
    assert torch.equal(fwd['pos'], oi + d[:n] * first[:, None])
    assert bool((back['t'] - back['sdf'] < -0.5).all())                  # t0 < 0: behind the origin, on the sphere
    outside = trace(net, o[:n], d[:n], entry_forward=True)                # an origin outside: the flag changes nothing
    assert same(outside, rows(ref, slice(0, n)))
    # R == 0, nullable outputs, the C entry's own argument checks
    only_hit, only_pos = torch.full((n,), 249, dtype=torch.uint8, device=gpu), torch.full((n, 3), -7.0, device=gpu)
    A = (addr(o), 3, addr(d), 3)
    eng.sdf_trace(*A, 0, hit=only_hit, pos=only_pos)                     # nothing launched, nothing written
    assert bool((only_hit == 249).all()) and bool((only_pos == -7).all())
    eng.sdf_trace(*A, n, hit=only_hit)                                    # any subset of the outputs, same bits
    eng.sdf_trace(*A, n, pos=only_pos)
    eng.sdf_trace(*A, n)                                                  # nothing asked for: still a valid call
    assert torch.equal(only_hit, ref['hit'][:n]) and torch.equal(only_pos, ref['pos'][:n])
    empty = trace(net, o[:0], d[:0])
    assert {k: tuple(v.shape) for k, v in empty.items()} == {'pos': (0, 3), 't': (0,), 'sdf': (0,), 'iters': (0,), 'hit': (0,)}
    assert empty['iters'].dtype == torch.int32 and empty['hit'].dtype == torch.uint8
    lib, net_ref, S = eng.lib, ctypes.byref(eng._sdf_net), eng.stream()
    good = dict(net=net_ref, O=addr(o), o_ld=3, D=addr(d), d_ld=3, R=n, fg=None, max_iter=200, threshold=1e-5, rb=1.0, flags=0)
    assert NU_TRACE_ENTRY_FORWARD == 1
    for bad in (dict(net=None), dict(O=None), dict(D=None), dict(R=-1), dict(o_ld=2), dict(d_ld=2), dict(max_iter=0), dict(threshold=0.0),
                dict(threshold=-1e-5), dict(threshold=float('nan')), dict(net=None, R=0)):
        a = {**good, **bad}
        with pytest.raises(NuNerfLibraryError, match=r"nu_sdf_trace failed with code -1"):
            lib.nu_sdf_trace(a['net'], a['O'], a['o_ld'], a['D'], a['d_ld'], a['R'], a['fg'], a['max_iter'], a['threshold'], a['rb'],
                             a['flags'], addr(only_pos), None, None, None, addr(only_hit), S)
    torch.cuda.synchronize()
    assert torch.equal(only_hit, ref['hit'][:n]) and torch.equal(only_pos, ref['pos'][:n])
    for bad in (dict(rays_o=o.cpu()), dict(rays_d=d.cpu()), dict(mask=torch.ones(o.shape[0], dtype=torch.bool))):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            kw = {'rays_o': o, 'rays_d': d, **bad}
            trace(net, kw.pop('rays_o'), kw.pop('rays_d'), **kw)
    with pytest.raises(ValueError):
        trace(net, o, d, which='inner')


# ---- 6. against the mesh pipeline ----------------------------------------------------------------------------------------------------------
def test_against_the_mesh_pipeline(gpu, rays, models, full, oracle64):
    from nu_nerf_amd.curvature import bake_curvature
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.lbvh import LBVH
    from nu_nerf_amd.mesh import extract_geometry
    net, _, _, _ = models['init']
    eng = net.engine()
    eng.pack()

    def query(p):
        p = p.contiguous()
        return eng.sdf_forward(addr(p), 3, p.shape[0], keep=False, want_feat=False)['sdf']
    V, F = extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), 64, 0.0, query)
    o, d = rays
    bvh = LBVH(torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(gpu), torch.from_numpy(np.ascontiguousarray(F).astype(np.int32)).to(gpu))
    m_hit, _, m_t = bvh.intersect(torch.cat([o, d], 1), return_t=True)
    m_hit = m_hit > 0
    got = full['init']
    hit = got['hit'].bool()
    voxel = 2.0 / 63.0
    n = bake_curvature(net, got['pos'].contiguous())['normal']
    steep = (n * d).sum(1).abs() >= 0.3
    both = hit & m_hit & steep
    dt = float((got['t'] - m_t)[both].abs().max())
    mism = float((hit != m_hit).float().mean())
    mism64 = float((torch.from_numpy(oracle64['init']['hit']).to(gpu) != m_hit).float().mean())
    print(f"SDF trace vs 64^3 mesh: both hit {int((hit & m_hit).sum())} ({int(both.sum())} with |n.d| >= 0.3)  max |dt| {dt:.3e} (voxel {voxel:.3e})"
          f"  mask mismatch {mism:.4f}  float64 oracle vs mesh {mism64:.4f}")
    assert int(both.sum()) > 800
    assert dt <= voxel
    assert mism64 <= 0.03 and mism <= 0.03


# ---- 7. render_surface -----------------------------------------------------------------------------------------------------------------
def test_render_surface(gpu, models):
    from nu_nerf_amd import relight
    from nu_nerf_amd.curvature import bake_curvature
    from nu_nerf_amd.mask_render import pinhole_rays
    from nu_nerf_amd.materials import bake_materials
    from nu_nerf_amd.sdf_trace import AOVS, render_surface
    net, _, _, _ = models['parity']
    h = w = 48
    K = relight.intrinsics(h, w)
    pose = relight.relighting_poses(8, 0.0, 45.0, 3.0)[2]
    img = net.render_surface(K, pose, h, w, aovs=AOVS)
    assert set(img) == set(AOVS)
    r = pinhole_rays(torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(pose, dtype=torch.float32)[None], h, w, gpu)
    tr = trace(net, r[:, :3], r[:, 3:], entry_forward=True)
    hit = tr['hit'].bool()
    assert 200 < int(hit.sum()) < h * w - 200
    pts = tr['pos'][hit].contiguous()
    curv, mat = bake_curvature(net, pts), bake_materials(net, pts)

    def image(values, channels=None):
        out = torch.zeros((h * w, channels) if channels else (h * w,), device=gpu)
        out[hit] = values.reshape(out[hit].shape)
        return out.reshape((h, w, channels) if channels else (h, w))
    assert img['mask'].dtype == torch.uint8 and torch.equal(img['mask'], (tr['hit'] * 255).reshape(h, w))
    assert torch.equal(img['depth'], image(tr['t'][hit])) and torch.equal(img['position'], image(pts, 3))
    assert torch.equal(img['normal'], image(curv['normal'], 3))
    assert torch.equal(img['mean_curvature'], image(curv['mean'])) and torch.equal(img['gaussian_curvature'], image(curv['gaussian']))
    assert torch.equal(img['albedo'], image(mat['albedo'], 3)) and torch.equal(img['roughness'], image(mat['roughness']))
    assert torch.equal(img['metallic'], image(mat['metallic']))
    assert bool((img['depth'][img['mask'] > 0] > 1.5).all()) and not bool(img['depth'][img['mask'] == 0].any())
    assert float((img['normal'][img['mask'] > 0].norm(dim=1) - 1).abs().max()) < 1e-5
    default = render_surface(net, K, pose, h, w)
    assert set(default) == {'depth', 'normal', 'mask'} and all(torch.equal(default[k], img[k]) for k in default)
    for chunk in (1000, 64, h * w + 5):                                  # a chunked run: the same bits
        part = render_surface(net, K, pose, h, w, aovs=AOVS, chunk=chunk)
        assert all(torch.equal(part[k], img[k]) for k in AOVS), chunk
    few = render_surface(net, K, pose, h, w, aovs=('depth',), max_iter=3)
    assert int((few['depth'] > 0).sum()) < int(hit.sum())


def test_command_renders_a_frame_set(gpu, tmp_path, monkeypatch, capsys):
    import json
    import os
    import yaml
    from nu_nerf_amd import relight, render_surface as RS
    from nu_nerf_amd.mask_render import _pillow
    monkeypatch.chdir(tmp_path)
    with open('golden.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'golden', 'network': 'shape'}, fh)
    torch.manual_seed(0)
    out = RS.main(['--cfg', 'golden.yaml', '--ckpt', 'none', '--hw', '40', '--num', '2', '--aovs', 'depth', 'normal', 'mask', 'albedo'])
    assert out == os.path.join('data', 'surface', 'golden-0')
    assert sorted(os.listdir(out)) == sorted(f'{k}_{a}' for k in (0, 1) for a in ('albedo.png', 'depth.npy', 'depth.png', 'mask.png', 'normal.png'))
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep['frames'] == 2 and rep['step'] == 0 and rep['out'] == out and len(rep['hit']) == 2 and all(50 < n < 1600 for n in rep['hit'])
    depth = np.load(os.path.join(out, '0_depth.npy'))
    mask = np.asarray(_pillow().open(os.path.join(out, '0_mask.png')))
    assert depth.dtype == np.float32 and depth.shape == (40, 40) and mask.shape == (40, 40, 4)
    assert int((depth > 0).sum()) == rep['hit'][0] == int((mask[:, :, 0] > 0).sum())
    assert 2.2 < float(depth[depth > 0].min()) < 2.8                     # the initialised SDF is roughly a sphere of radius 0.5 seen from distance 3
