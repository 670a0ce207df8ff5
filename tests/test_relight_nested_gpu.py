"""Relighting of the nested object on the GPU: every traced ray of the interior chain and of the light paths against
nu_lbvh_trace bit for bit, the interface maths, the inner rows and the linear image against the float64 oracle, the index-matched
shell, the Fresnel bookkeeping under a constant environment, determinism and chunk invariance, argument handling, predict_ior, the
command.

fp32-against-float64 bounds are four times the largest deviation measured on the first GPU run (each test prints its figure before it
asserts; DESIGN.md 21 records both); all stay under the project's fp32 parity bar of 1e-4.  Pixels whose refract / reflect decision
lies within 1e-4 of the threshold eta^2 sin^2 = 0.999 are left out of the float64 comparisons, at most 2 % of the hit pixels of a scene
(test_relight_nested_host.py measures the share on the CPU: 0 of every scene used here)."""
import functools
import os

import numpy as np
import pytest
import torch

import nested_relight_oracle as NO
import relight_oracle as O
from test_relight_gpu import _cams_of, _env, _ico, _orbit, _rows64

pytestmark = pytest.mark.gpu

# measured on the first GPU run -> bound = 4 x measured (DESIGN.md 21 records both)
TOL_IFACE = 4 * 1.966e-6        # next ray (origin, direction), Fresnel factors and T, absolute
TOL_ATTR = 4 * 1.734e-6         # inner G-buffer rows, relative to max(1, |oracle|)
TOL_LINEAR = 4 * 3.053e-6       # linear radiance, relative to max(|oracle|, 1e-2)
assert max(TOL_IFACE, TOL_ATTR, TOL_LINEAR) < 1e-4
# index-matched shell against the opaque path, relative to max(|opaque|, 1e-2).  Exit pixels: rounding only.  Inner pixels: a FINDING, not
# rounding -- the interior ray starts ORIGIN_EPS = 1e-4 off the shell along the facet normal, which moves it sideways by up to 1e-4; on
# the inner sphere (radius 0.2) the hit point moves by up to 2.7e-4 and the normal by 1.5e-3, and a pixel whose samples straddle the
# step of the test environment changes by 1.6 %.  It is the price of the eps offsets of the transport, not of the kernels.
TOL_MATCHED_EXIT = 4 * 1.277e-6
TOL_MATCHED_INNER = 4 * 1.607e-2
# ... and the sharp companion: the opaque passes (nu_relight_visibility + nu_relight_resolve) fed the DEVICE's inner rows, so that only
# the light's way out through the index-matched shell differs
TOL_MATCHED_ROWS = 4 * 2.333e-7
MARGIN, MARGIN_CAP = 1e-4, 0.02
INNER_C = np.array([0.1, 0.0, 0.05], np.float32)
SCENES = {'ico2': (24, 24), 'ico3': (48, 48), 'box': (40, 40), 'ico7': (32, 32)}


def _meshes(name):
    if name == 'box':
        Vo, Fo = NO.box(0.4)
        ior = np.full(len(Vo), 1.5, np.float32)
        Vi, Fi = _ico(1, 0.2)
    else:
        Vo, Fo = _ico(int(name[3:]))
        ior = (1.45 + 0.25 * Vo[:, 0] + 0.1 * Vo[:, 2]).astype(np.float32)            # 1.27 .. 1.63 over the sphere
        Vi, Fi = _ico(1 if name == 'ico2' else 2, 0.2)
    g = np.random.Generator(np.random.PCG64(5))
    return Vo, Fo, ior, (Vi + INNER_C).astype(np.float32), Fi, g.uniform(0.05, 0.95, (len(Vi), 5)).astype(np.float32)


def _poses(name):
    return _orbit(3, az=20.0, el=45.0 if name == 'box' else 30.0, dist=2.2)[1:2]


@functools.lru_cache(maxsize=None)
def _case(name, S=16, seed=7):
    """Everything the tests of one scene share: the scene, the outer G-buffer, the dumped chain and the dumped light paths."""
    from nu_nerf_amd import relight as R
    gpu = torch.device('cuda', torch.cuda.current_device())
    h, w = SCENES[name]
    Vo, Fo, ior, Vi, Fi, mat = _meshes(name)
    ns = R.NestedScene(Vo, Fo, ior, Vi, Fi, mat, device=gpu)
    poses = _poses(name)
    face, gbuf = R.gbuffer(ns.outer, _cams_of(gpu, R.intrinsics(h, w), poses), h, w, img0=3)
    pix = R.hit_pixels(face)
    kind, chain, irow, seg, aux = R.nested_chain(ns, gbuf, pix, dump=True)
    sel = (kind == R.INNER).nonzero().flatten().to(torch.int32)
    rec, ldump = R.nested_light(ns, irow, sel, S, 0, S, seed, dump=True)
    return dict(ns=ns, h=h, w=w, poses=poses, face=face, gbuf=gbuf, pix=pix, kind=kind, chain=chain, irow=irow, seg=seg, aux=aux, sel=sel,
                rec=rec, ldump=ldump, S=S, seed=seed, meshes=(Vo, Fo, ior, Vi, Fi, mat))


def _i(t):
    return t.contiguous().view(torch.int32)


def _trace(bvh, rays):
    hit, idx, t = bvh.intersect(rays, return_t=True)
    return (hit > 0).to(torch.int32), idx, t


# ---- 1. hits are the tracer's -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['ico2', 'ico3', 'box', 'ico7'])
def test_every_traced_ray_meets_what_lbvh_trace_finds(gpu, name):
    from nu_nerf_amd import relight as R
    c = _case(name)
    ns, seg, aux, kind = c['ns'], c['seg'], c['aux'], c['kind']
    assert c['pix'].numel() > 100 and int((kind == R.INNER).sum()) > 10 and int((kind == R.EXIT).sum()) > 50
    # the entries without dump outputs give the same bits
    k2, ch2, ir2 = R.nested_chain(ns, c['gbuf'], c['pix'])
    assert torch.equal(k2, kind) and torch.equal(_i(ch2), _i(c['chain'])) and torch.equal(_i(ir2), _i(c['irow']))
    assert torch.equal(_i(R.nested_light(ns, c['irow'], c['sel'], c['S'], 0, c['S'], c['seed'])), _i(c['rec']))
    s = seg.reshape(-1, R.SEG)
    s = s[_i(s[:, 15]) == 1]
    assert s.shape[0] >= c['pix'].numel() - 5
    fi, ii, ti = _trace(ns.inner.bvh, s[:, :6])
    fo, io, to = _trace(ns.outer.bvh, s[:, :6])
    assert torch.equal(_i(s[:, 9]), fi) and torch.equal(_i(s[:, 10]), ii) and torch.equal(_i(s[:, 11]), _i(ti))
    assert torch.equal(_i(s[:, 12]), fo) and torch.equal(_i(s[:, 13]), io) and torch.equal(_i(s[:, 14]), _i(to))
    ends_inner = (fi == 1) & ((fo == 0) | (ti <= to))
    which = torch.where(ends_inner, 1, torch.where(fo == 1, 2, 0)).to(torch.int32)
    assert torch.equal(_i(s[:, 6]), which)
    assert torch.equal(_i(s[:, 7]), torch.where(ends_inner, ii, io)) and torch.equal(_i(s[:, 8]), _i(torch.where(ends_inner, ti, to)))
    for k in range(2):                                      # reflection ray, exit ray: any hit = the closest-hit predicate
        a = aux[:, k]
        tr = a[:, 6] == 1
        assert bool(tr.any()) and torch.equal((a[tr, 7] == 1).to(torch.int32), _trace(ns.outer.bvh, a[tr, :6])[0])
        assert not bool(a[~tr, 7].any())
    assert torch.equal(c['chain'][:, 9], ((aux[:, 0, 6] == 1) & (aux[:, 0, 7] == 0)).float())
    ex = kind == R.EXIT
    assert torch.equal(c['chain'][ex, 4], ((aux[ex, 1, 6] == 0) | (aux[ex, 1, 7] == 0)).float())
    # light paths
    d = c['ldump']
    tr = d[:, 6] == 1
    assert 0.3 < float(tr.float().mean()) < 1.0
    assert torch.equal((d[tr, 7] == 1).to(torch.int32), _trace(ns.inner.bvh, d[tr, :6])[0]) and not bool(d[~tr, 7:].any())
    b = tr & (d[:, 7] == 0)
    fo, io, to = _trace(ns.outer.bvh, d[b, :6])
    assert torch.equal((d[b, 8] == 1).to(torch.int32), fo) and torch.equal(_i(d[b, 9]), io) and torch.equal(_i(d[b, 10]), _i(to))
    e = b & (d[:, 8] == 1) & (d[:, 11] == 1)
    assert bool(e.any()) and torch.equal((d[e, 18] == 1).to(torch.int32), _trace(ns.outer.bvh, d[e, 12:18])[0])
    lit = e & (d[:, 18] == 0)
    rec = c['rec'].reshape(-1, 4)
    assert torch.equal(_i(rec[lit]), _i(torch.cat([d[lit, 15:18], d[lit, 19:20]], 1))) and not bool(rec[~lit & ~(b & (d[:, 8] == 0))].any())
    if name == 'box':
        assert int((_i(c['chain'][:, 10]) > 1).sum()) > 10          # total internal reflection inside the box: more than one segment


# ---- 2. interface maths ---------------------------------------------------------------------------------------------------------------
def _outer64(c):
    Vo, Fo, ior = c['meshes'][:3]
    return Vo.astype(np.float64), Fo.astype(np.int64), c['ns'].outer.normals.cpu().numpy().astype(np.float64), ior.astype(np.float64)


@pytest.mark.parametrize("name", ['ico2', 'ico3', 'box'])
def test_interface_maths_matches_the_float64_oracle(gpu, name):
    from nu_nerf_amd import relight as R
    c = _case(name)
    Vo, Fo, VNo, ior = _outer64(c)
    rows, _, _ = _rows64(c['gbuf'], c['pix'])
    n = len(rows)
    seg = c['seg'].cpu().numpy()
    segi = seg.view(np.int32)
    aux, chain, kind = c['aux'].cpu().numpy().astype(np.float64), c['chain'].cpu().numpy(), c['kind'].cpu().numpy()
    walked = chain.view(np.int32)[:, 10]
    ev = NO.entry(rows)
    near = np.abs(ev['k2'] - NO.TIR_K2) <= MARGIN
    bad = near.copy()
    assert np.array_equal((walked >= 1)[~near], ev['refr'][~near])
    err = 0.0
    ok = ev['refr'] & (walked >= 1)
    err = max(err, np.abs(chain[ok, 8] - ev['F'][ok]).max(), np.abs(chain[ok, 5:8] - ev['r'][ok]).max())
    err = max(err, np.abs(seg[ok, 0, :3] - (rows[ok, 1:4] - R.ORIGIN_EPS * rows[ok, 4:7])).max(), np.abs(seg[ok, 0, 3:6] - ev['dn'][ok]).max())
    T = np.where(ok, 1.0 - ev['F'], 0.0)
    f_exit = np.zeros(n)
    K = seg.shape[1]
    for k in range(K):
        at = np.flatnonzero((walked > k) & (segi[:, k, 6] == 2))
        if not len(at):
            continue
        o, d = seg[at, k, :3].astype(np.float64), seg[at, k, 3:6].astype(np.float64)
        lv = NO.leave(Vo, Fo, VNo, ior, o, d, segi[at, k, 7].astype(np.int64), R.ORIGIN_EPS)
        dev_refr = (walked[at] == k + 1) & (kind[at] == R.EXIT)
        nr = np.abs(lv['k2'] - NO.TIR_K2) <= MARGIN
        bad[at[nr]] = True
        assert np.array_equal(dev_refr[~nr], lv['refr'][~nr])
        same = dev_refr == lv['refr']
        out = same & dev_refr
        if out.any():
            j = at[out]
            err = max(err, np.abs(aux[j, 1, :3] - lv['o2'][out]).max(), np.abs(aux[j, 1, 3:6] - lv['dn'][out]).max())
            T[j] *= 1.0 - lv['F'][out]
            f_exit[j] = lv['F'][out]
        tir = same & ~dev_refr & (k + 1 < K) & (walked[at] > k + 1)
        if tir.any():
            j = at[tir]
            err = max(err, np.abs(seg[j, k + 1, :3] - lv['o2'][tir]).max(), np.abs(seg[j, k + 1, 3:6] - lv['dn'][tir]).max())
    good = ~bad & (kind != R.DARK)
    err = max(err, np.abs(chain[good, 0] - T[good]).max())
    share = bad.mean()
    print(f"{name}: interface maths max deviation {err:.3e} over {n} pixels (bound {TOL_IFACE:.3e}); {bad.sum()} pixels ({share:.2%}) within "
          f"{MARGIN} of the threshold left out")
    assert share <= MARGIN_CAP and err <= TOL_IFACE
    assert not chain[kind == R.DARK, 0].any()
    if name == 'box':
        assert ((walked > 1) & (kind != R.DARK)).sum() > 10


# ---- 3. inner rows ---------------------------------------------------------------------------------------------------------------------
def test_inner_rows_match_the_float64_oracle(gpu):
    from nu_nerf_amd import relight as R
    c = _case('ico3')
    Vi, Fi, mat = c['meshes'][3:]
    kind = c['kind'].cpu().numpy()
    sel = np.flatnonzero(kind == R.INNER)
    seg = c['seg'].cpu().numpy()
    last = c['chain'].cpu().numpy().view(np.int32)[sel, 10] - 1
    s = seg[sel, last]
    assert (s.view(np.int32)[:, 6] == 1).all()
    rows = c['irow'].cpu().numpy()[sel]
    outer_ids = c['gbuf'].reshape(-1, O.ROW)[c['pix'].long()].cpu().numpy().view(np.int32)[sel, 18:20]
    assert np.array_equal(rows.view(np.int32)[:, 18:20], outer_ids) and (outer_ids[:, 0] == 3).all()
    VN = c['ns'].inner.normals.cpu().numpy().astype(np.float64)
    ref = O.gbuffer_rows(Vi.astype(np.float64), Fi.astype(np.int64), VN, mat.astype(np.float64), s[:, :3].astype(np.float64),
                         s[:, 3:6].astype(np.float64), s.view(np.int32)[:, 7].astype(np.int64), 0, 0)
    rows = rows.astype(np.float64)
    err = (np.abs(rows[:, :18] - ref[:, :18]) / np.maximum(1.0, np.abs(ref[:, :18]))).max()
    print(f"inner rows: max deviation {err:.3e} over {len(sel)} pixels (bound {TOL_ATTR:.3e})")
    assert len(sel) > 100 and err <= TOL_ATTR
    assert np.abs(np.linalg.norm(rows[:, 4:7], axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(rows[:, 7:10], axis=1) - 1).max() < 1e-6
    assert (np.sum(rows[:, 4:7] * rows[:, 15:18], 1) >= 0).all() and (np.sum(rows[:, 4:7] * rows[:, 7:10], 1) >= 0).all()
    assert not c['irow'][c['kind'] != R.INNER].any()


# ---- 4. linear image ---------------------------------------------------------------------------------------------------------------------
def _image_vs_oracle(c, env, S, seed):
    from nu_nerf_amd import relight as R
    ns, h, w = c['ns'], c['h'], c['w']
    lin = R.relight_nested_linear(ns, env, c['poses'], h, w, S, seed, chunk=S, img0=3)
    rec = torch.zeros(c['pix'].numel(), S, 4, device=lin.device)
    rec[c['sel'].long()] = R.nested_light(ns, c['irow'], c['sel'], S, 0, S, seed)
    rows, img, pixel = _rows64(c['gbuf'], c['pix'])
    ref = NO.resolve(c['kind'].cpu().numpy(), c['chain'].cpu().numpy().astype(np.float64), c['irow'].cpu().numpy().astype(np.float64), img,
                     pixel, rec.cpu().numpy().astype(np.float64), S, seed, env.astype(np.float64))
    got = lin.reshape(-1, 4)[c['pix'].long()].cpu().numpy().astype(np.float64)
    return lin, got, ref


@pytest.mark.parametrize("name,S", [('ico3', 64), ('box', 16)])
def test_linear_image_matches_the_oracle_fed_the_device_records(gpu, name, S):
    from nu_nerf_amd import relight as R
    c = _case(name)
    env = _env()
    lin, got, ref = _image_vs_oracle(c, env, S, 11)
    err = (np.abs(got[:, :3] - ref) / np.maximum(np.abs(ref), 1e-2)).max()
    print(f"{name}: linear image max relative deviation {err:.3e} over {len(ref)} pixels (bound {TOL_LINEAR:.3e})")
    assert err <= TOL_LINEAR
    alpha = lin[..., 3].reshape(-1)
    assert torch.equal(alpha, (c['face'].reshape(-1) != O.MISS).float()) and not bool(lin.reshape(-1, 4)[alpha == 0].any())
    img8 = R.to_srgb8(lin).reshape(-1, 4)
    assert torch.equal(img8, R.relight_nested(c['ns'], env, c['poses'], c['h'], c['w'], S, 11, chunk=S, img0=3).reshape(-1, 4))
    d8 = np.abs(img8[c['pix'].long(), :3].cpu().numpy().astype(np.int64) - O.to_srgb8(ref))
    print(f"{name}: 8-bit image max difference {d8.max()} levels")
    assert d8.max() <= 1 and set(np.unique(img8[:, 3].cpu().numpy())) == {0, 255}
    inner = (c['kind'] == R.INNER).cpu().numpy()
    assert got[inner, :3].sum(1).min() > 0 and ref[~inner].max() > 0


# ---- 5. index-matched shell ----------------------------------------------------------------------------------------------------------------
def test_index_matched_shell_disappears(gpu):
    from nu_nerf_amd import relight as R
    Vo, Fo, _, Vi, Fi, mat = _meshes('ico3')
    h, w, S, seed = 48, 48, 16, 4
    env, poses = _env(), _poses('ico3')
    ns = R.NestedScene(Vo, Fo, 1.0, Vi, Fi, mat, device=gpu)
    lin = R.relight_nested_linear(ns, env, poses, h, w, S, seed).reshape(-1, 4)
    face, gbuf = R.gbuffer(ns.outer, _cams_of(gpu, R.intrinsics(h, w), poses), h, w)
    pix = R.hit_pixels(face)
    kind, chain, irow = R.nested_chain(ns, gbuf, pix)
    assert not bool(chain[:, 8].any())                                          # F_entry: the reflection term is exactly 0
    assert float(chain[kind != R.DARK, 0].min()) == 1.0 and float(chain[:, 0].max()) == 1.0
    opaque = R.relight_linear(ns.inner, None, None, env, poses, h, w, S, seed).reshape(-1, 4)
    inner = pix[kind == R.INNER].long()
    n_nested, n_opaque = inner.numel(), int((opaque[:, 3] == 1).sum())
    inner = inner[opaque[inner, 3] == 1]                                        # but for silhouette pixels the same set
    assert inner.numel() > 100 and inner.numel() >= 0.98 * max(n_nested, n_opaque)
    a, b = lin[inner, :3].cpu().numpy().astype(np.float64), opaque[inner, :3].cpu().numpy().astype(np.float64)
    err_in = (np.abs(a - b) / np.maximum(np.abs(b), 1e-2)).max()
    # the trained rule reflects totally where eta^2 sin^2 > 0.999 whatever the index: at ior = 1 the few rays that leave within 1.8 degrees
    # of grazing bounce inside and leave elsewhere.  Every other exit pixel -- one interior segment -- goes straight through.
    n_exit = int((kind == R.EXIT).sum())
    ex = (kind == R.EXIT) & (_i(chain[:, 10]) == 1)
    assert int(ex.sum()) >= (1 - MARGIN_CAP) * n_exit
    d0 = -gbuf.reshape(-1, O.ROW)[pix[ex].long(), 15:18]
    want = R.env_lookup(torch.from_numpy(R.pack_env(env)).to(gpu), d0).cpu().numpy().astype(np.float64)
    got = lin[pix[ex].long(), :3].cpu().numpy().astype(np.float64)
    err_ex = (np.abs(got - want) / np.maximum(np.abs(want), 1e-2)).max()
    print(f"index-matched shell: inner pixels {err_in:.3e} ({inner.numel()}), exit pixels {err_ex:.3e} ({int(ex.sum())}) relative to the "
          f"opaque path (bounds {TOL_MATCHED_INNER:.3e}, {TOL_MATCHED_EXIT:.3e})")
    assert int(ex.sum()) > 500 and bool((chain[ex, 4] == 1).all())
    assert err_in <= TOL_MATCHED_INNER and err_ex <= TOL_MATCHED_EXIT
    sel = (kind == R.INNER).nonzero().flatten().to(torch.int32)
    vis = R.visibility(ns.inner, irow, sel, S, 0, S, seed)
    rec = R.nested_light(ns, irow, sel, S, 0, S, seed)
    assert torch.equal(vis != 0, rec[..., 3] == 1) and bool(((rec[..., 3] == 0) | (rec[..., 3] == 1)).all())    # same verdicts, keep = 1
    same = torch.zeros(pix.numel(), 4, device=gpu)
    R.resolve(irow, sel, S, 0, S, seed, torch.from_numpy(R.pack_env(env)).to(gpu), vis, same)
    a = lin[pix[sel.long()].long(), :3].cpu().numpy().astype(np.float64)
    b = same[sel.long(), :3].cpu().numpy().astype(np.float64)
    err_rows = (np.abs(a - b) / np.maximum(np.abs(b), 1e-2)).max()
    print(f"index-matched shell: inner pixels against the opaque passes on the same rows {err_rows:.3e} ({sel.numel()}) "
          f"(bound {TOL_MATCHED_ROWS:.3e})")
    assert err_rows <= TOL_MATCHED_ROWS


# ---- 6. Fresnel bookkeeping under a constant environment ----------------------------------------------------------------------------------
def test_constant_environment_shows_the_fresnel_bookkeeping(gpu):
    from nu_nerf_amd import relight as R
    c = _case('ico3')
    env = np.ones((16, 32, 3), np.float32)
    lin, got, ref = _image_vs_oracle(c, env, 16, 11)
    err = (np.abs(got[:, :3] - ref) / np.maximum(np.abs(ref), 1e-2)).max()
    Vo, Fo, VNo, ior = _outer64(c)
    rows, _, _ = _rows64(c['gbuf'], c['pix'])
    kind, chain = c['kind'].cpu().numpy(), c['chain'].cpu().numpy()
    one = np.flatnonzero((kind == R.EXIT) & (chain.view(np.int32)[:, 10] == 1))  # straight through: one interior segment
    seg = c['seg'].cpu().numpy()[one, 0]
    ev = NO.entry(rows[one])
    lv = NO.leave(Vo, Fo, VNo, ior, seg[:, :3].astype(np.float64), seg[:, 3:6].astype(np.float64), seg.view(np.int32)[:, 7].astype(np.int64),
                  R.ORIGIN_EPS)
    far = (np.abs(ev['k2'] - NO.TIR_K2) > MARGIN) & (np.abs(lv['k2'] - NO.TIR_K2) > MARGIN)
    # (a faceted sphere: at the silhouette the mirrored or the refracted ray can meet the shell again, and that term is dark -- the
    # visibility bits are the tracer's, test 1; nearly every pixel has both)
    vis_r, vis_e = chain[one, 9].astype(np.float64), chain[one, 4].astype(np.float64)
    assert (vis_r * vis_e).mean() > 0.9
    want = ev['F'] * vis_r + (1.0 - ev['F']) * (1.0 - lv['F']) * vis_e
    dev = np.abs(got[one, 0] - want)[far].max()
    print(f"constant environment: image vs oracle {err:.3e}, exit pixels vs F + (1 - F)(1 - F_exit) {dev:.3e} over {far.sum()} pixels "
          f"(bound {TOL_LINEAR:.3e})")
    assert far.sum() > 500 and far.mean() >= 1 - MARGIN_CAP
    assert err <= TOL_LINEAR and dev <= TOL_LINEAR
    both = vis_r * vis_e == 1
    assert np.array_equal(got[one, 0], got[one, 1]) and 0.5 < want[both].min() and want.max() <= 1.0 + 1e-12


# ---- 7. determinism and chunk invariance ----------------------------------------------------------------------------------------------------
def test_runs_and_chunkings_are_bit_identical(gpu):
    from nu_nerf_amd import relight as R
    Vo, Fo, ior, Vi, Fi, mat = _meshes('ico2')
    ns = R.NestedScene(Vo, Fo, ior, Vi, Fi, mat, device=gpu)
    h, w, S, seed = 30, 38, 48, 2
    env, poses = _env(), _orbit(3, el=30.0, dist=2.2)
    one = R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=S, images=3)
    assert bool((one[..., 3] == 1).any()) and bool((one[..., :3] > 0).any())
    assert torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=S, images=3))
    assert torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=S, images=3, rows=7))
    assert torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=S, images=1, rows=11))
    assert torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=10, images=2, rows=11))
    assert torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed, chunk=48, images=2, rows=7))
    assert torch.equal(one[1:], R.relight_nested_linear(ns, env, poses[1:], h, w, S, seed, img0=1))
    assert not torch.equal(one, R.relight_nested_linear(ns, env, poses, h, w, S, seed + 1))
    fresh = R.NestedScene(Vo, Fo, ior, Vi, Fi, mat, device=gpu)                   # a second build of both trees and the normals
    assert torch.equal(one, R.relight_nested_linear(fresh, env, poses, h, w, S, seed))


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(gpu):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd import relight as R
    c = _case('ico2')
    ns, irow, sel, chain, kind, pix = c['ns'], c['irow'], c['sel'], c['chain'], c['kind'], c['pix']
    env = torch.from_numpy(R.pack_env(_env())).to(gpu)
    out = torch.zeros(c['h'] * c['w'], 4, device=gpu)
    with pytest.raises(RuntimeError, match="nu_relight_nested_light"):
        R.nested_light(ns, irow, sel, 15, 0, 4, 0)
    with pytest.raises(RuntimeError, match="nu_relight_nested_light"):
        R.nested_light(ns, irow, sel, 16, 10, 7, 0)
    with pytest.raises(RuntimeError, match="nu_relight_nested_resolve"):
        R.nested_resolve(irow, chain, kind, pix, sel, 16, 10, 7, 0, env, c['rec'], True, out)
    with pytest.raises(RuntimeError, match="nu_relight_nested_resolve"):
        R.nested_resolve(irow, chain, kind, pix, sel, 15, 0, 4, 0, env, c['rec'], True, out)
    with pytest.raises(RuntimeError, match="nu_relight_nested_resolve"):
        R.nested_resolve(irow, chain, kind, pix, sel, 16, 0, 4, 0, env, None, True, out)
    lib, a = L.load(), list(ns._args())
    tail = (L.ptr(c['gbuf']), L.ptr(pix), int(pix.numel()), 1e-4, 4, L.ptr(kind.clone()), L.ptr(chain.clone()), L.ptr(irow.clone()), L.stream())
    for k in (0, 2, 5, 6, 11):
        with pytest.raises(RuntimeError, match="nu_relight_nested_chain"):
            lib.nu_relight_nested_chain(*(a[:k] + [None] + a[k + 1:]), *tail)
    with pytest.raises(RuntimeError, match="nu_relight_nested_chain"):
        lib.nu_relight_nested_chain(*a, *tail[:4], 0, *tail[5:])
    with pytest.raises(RuntimeError, match="nu_relight_nested_chain"):
        lib.nu_relight_nested_chain(*a, None, *tail[1:])
    # a zero pixel count is fine and touches nothing
    empty = pix[:0]
    k0, ch0, ir0 = R.nested_chain(ns, c['gbuf'], empty)
    assert k0.numel() == 0 and R.nested_light(ns, irow, empty, 16, 0, 16, 0).shape == (0, 16, 4)
    R.nested_resolve(irow, chain, kind, pix, empty, 16, 0, 16, 0, env, c['rec'], True, out)
    assert not bool(out.any())
    with pytest.raises(ValueError):
        R.NestedScene(*c['meshes'][:2], 0.9, *c['meshes'][3:], device=gpu)
    with pytest.raises(ValueError):
        R.relight_nested_linear(ns, _env(), c['poses'], 8, 8, 7)


# ---- 9. predict_ior ----------------------------------------------------------------------------------------------------------------------
def test_predict_ior_is_the_index_the_refraction_kernel_uses(gpu):
    from nu_nerf_amd import materials as M
    from nu_nerf_amd import stage2_ops as S2
    from nu_nerf_amd import torch_glue as G
    from test_materials_gpu import stage1_net, stage2_net
    net, _ = stage2_net(gpu)
    V, F = _ico(2)
    got = M.predict_ior(net, (V, F))
    assert got.shape == (len(V), 1) and got.dtype == np.float32
    n1, n2 = net.nets()
    x = torch.from_numpy(V).to(gpu)
    raw = torch.sigmoid(n2.ior(G.embed(x, 6))).detach()
    nrm = torch.nn.functional.normalize(x, dim=-1)
    _, eta, _, _ = S2.refract(n1.eng, -nrm, nrm, raw, x, True)
    want = (1.0 / eta.double()).cpu().numpy()
    err = (np.abs(got[:, 0].astype(np.float64) - want) / want).max()
    print(f"predict_ior: max relative deviation from 1 / eta {err:.3e}")
    assert err <= 1e-6
    assert (got > 1.0).all() and (got < 2.0).all() and got.std() > 0
    with pytest.raises(ValueError):
        M.predict_ior(stage1_net(gpu)[0], (V, F))


# ---- 11. the command ---------------------------------------------------------------------------------------------------------------------
def test_command_end_to_end(gpu, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from nu_nerf_amd import mesh as M
    from nu_nerf_amd import relight as R
    Vo, Fo, ior, Vi, Fi, mat = _meshes('ico2')
    M.write_ply(str(tmp_path / 'outer.ply'), Vo, Fo)
    M.write_ply(str(tmp_path / 'inner.ply'), Vi, Fi)
    os.makedirs(tmp_path / 'mat')
    np.save(tmp_path / 'mat' / 'albedo.npy', mat[:, :3])
    np.save(tmp_path / 'mat' / 'metallic.npy', mat[:, 3:4])
    np.save(tmp_path / 'mat' / 'roughness.npy', mat[:, 4:5])
    np.save(tmp_path / 'mat' / 'ior.npy', ior[:, None])
    np.save(tmp_path / 'env.npy', _env())
    monkeypatch.chdir(tmp_path)
    argv = ['--mesh', 'outer.ply', '--inner', 'inner.ply', '--inner-material', 'mat', '--ior', 'mat', '--hdr', 'env.npy', '--name', 'glass',
            '--num', '2', '--width', '32', '--height', '32', '--samples', '16', '--cam_dist', '2.2']
    out = R.main(argv)
    assert out == os.path.join('data', 'relight', 'glass')
    frames = []
    for k in range(2):
        with Image.open(os.path.join(out, f'{k}.png')) as im:
            assert im.mode == 'RGBA' and im.size == (32, 32)
            frames.append(np.asarray(im).copy())
    ns = R.NestedScene(Vo, Fo, ior, Vi, Fi, mat, device=gpu)
    poses = R.camera_in_mesh_frame(R.relighting_poses(2, 0.0, 45.0, 2.2))
    for k in range(2):
        face, _ = R.gbuffer(ns.outer, _cams_of(gpu, R.intrinsics(32, 32), poses[k:k + 1]), 32, 32)
        miss = (face[0] == O.MISS).cpu().numpy()
        assert miss.any() and (~miss).any() and np.array_equal(frames[k][..., 3] == 0, miss) and not frames[k][miss].any()
        assert set(np.unique(frames[k][..., 3])) == {0, 255}
        want = R.relight_nested(ns, _env(), poses[k:k + 1], 32, 32, 16, 0, img0=k)
        assert np.array_equal(want[0].cpu().numpy(), frames[k])
    stamp = {k: os.stat(os.path.join(out, f'{k}.png')).st_mtime_ns for k in range(2)}
    capsys.readouterr()
    R.main(argv)
    assert 'all 2 frames exist' in capsys.readouterr().out
    assert {k: os.stat(os.path.join(out, f'{k}.png')).st_mtime_ns for k in range(2)} == stamp
    # a scalar index gives another picture
    R.main(argv[:7] + ['1.2'] + argv[8:] + ['--output', 'other'])
    with Image.open(os.path.join('other', '1.png')) as im:
        assert not np.array_equal(np.asarray(im), frames[1])
