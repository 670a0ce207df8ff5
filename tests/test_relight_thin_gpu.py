"""Relighting through the thin shell on the GPU: the wall crossing against oracle/stage2_oracle.shell_refraction in float64
and against nu_s2_shell_fwd, every traced ray against nu_lbvh_trace bit for bit, the chain / inner / light records and the linear image
against the float64 oracle, the energy bookkeeping under a constant environment, determinism and chunk invariance, predict_shell, the
two commands.

fp32-against-float64 bounds are four times the largest deviation measured on the first GPU run (each test prints its figure before it
asserts; DESIGN.md 22 records both); all stay under the project's fp32 parity bar of 1e-4, and all are ABSOLUTE unless they say otherwise.
One bound cannot have the 4 x margin.  The trained chord length R cos - sqrt((R cos)^2 -+ 2 R th + th^2) is a difference of two
quantities of size R = 1 / sqrt(max(|curvature|, 1e-6)), so its fp32 rounding is about an ulp(R) whatever the arithmetic: on a flat row
(|curvature| < 1e-6, R = 1000, ulp 6.1e-5) the positions behind the crossing measured 4.5e-5 / 5.6e-5 from float64, and four times that
is past 1e-4.  Those rows get the explicit bound TOL_CROSS_POS_FLAT = 1.5 ulp(1000) = 9.2e-5 < 1e-4 (half an ulp each for R cos and the
root, a quarter propagated from the square, a quarter to spare); rows with |curvature| >= 1e-6 get 4 x their own measured deviation.
Rows / pixels with a decision within 1e-4 of its branch point (the 0.999 tests, the 1e-4 clamps of 1 - sin^2_t and of the chord
discriminants) are left out of the float64 comparisons, at most 2 % (test_relight_thin_host.py measures the share on the CPU)."""
import functools
import os

import numpy as np
import pytest
import torch

import nested_relight_oracle as NO
import relight_oracle as O
import thin_relight_oracle as TO
from test_relight_gpu import _cams_of, _env, _ico, _orbit, _rows64

pytestmark = pytest.mark.gpu

# measured on the first GPU run -> bound = 4 x measured (DESIGN.md 22 records both)
TOL_CROSS_POS = 4 * 7.571e-7     # crossing op: end point and next origin on rows with |curvature| >= 1e-6
TOL_CROSS_POS_FLAT = 1.5 * 2.0 ** -14   # ... on rows with |curvature| < 1e-6: 1.5 ulp(R = 1000) = 9.2e-5 (module docstring; measured 5.6e-5)
TOL_CROSS_DIR = 4 * 3.820e-6     # crossing op: oriented normal and next direction
TOL_CROSS_F = 4 * 2.123e-5       # crossing op: the two Fresnel factors
TOL_CHAIN = 4 * 4.478e-6         # chain records: cavity and exit rays, mirror direction, Fresnel factor, T
TOL_LIGHT = 4 * 5.419e-7         # light records: exit ray and keep
TOL_ATTR = 4 * 1.166e-6          # inner G-buffer rows, relative to max(1, |oracle|)
TOL_LINEAR = 4 * 1.827e-6        # linear radiance, relative to max(|oracle|, 1e-2)
TOL_BAKE = 4 * 1.604e-7          # predict_shell against the float64 evaluation of the two modules, relative
assert max(TOL_CROSS_POS, TOL_CROSS_POS_FLAT, TOL_CROSS_DIR, TOL_CROSS_F, TOL_CHAIN, TOL_LIGHT, TOL_ATTR, TOL_LINEAR, TOL_BAKE) < 1e-4
MARGIN, MARGIN_CAP, N_ROWS, N_FLAT, SCENES, _meshes, _poses = TO.MARGIN, TO.MARGIN_CAP, TO.N_ROWS, TO.N_FLAT, TO.SCENES, TO.meshes, TO.poses


def _radius(gk):
    return 1.0 / np.sqrt(np.maximum(np.abs(gk), 1e-6))


@functools.lru_cache(maxsize=None)
def _case(name, S=16, seed=7):
    """Everything the tests of one scene share: the scene, the outer G-buffer, the dumped chain and the dumped light paths."""
    from nu_nerf_amd import relight as R
    gpu = torch.device('cuda', torch.cuda.current_device())
    h, w = SCENES[name]
    Vo, Fo, ior, th, Vi, Fi, mat = _meshes(name)
    ts = R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, device=gpu)
    poses = _poses(name)
    face, gbuf = R.gbuffer(ts.outer, _cams_of(gpu, R.intrinsics(h, w), poses), h, w, img0=3)
    pix = R.hit_pixels(face)
    kind, chain, irow, seg, aux = R.thin_chain(ts, gbuf, pix, dump=True)
    sel = (kind == R.INNER).nonzero().flatten().to(torch.int32)
    rec, ldump = R.thin_light(ts, irow, sel, S, 0, S, seed, dump=True)
    return dict(ts=ts, h=h, w=w, poses=poses, face=face, gbuf=gbuf, pix=pix, kind=kind, chain=chain, irow=irow, seg=seg, aux=aux, sel=sel,
                rec=rec, ldump=ldump, S=S, seed=seed, meshes=(Vo, Fo, ior, th, Vi, Fi, mat))


def _i(t):
    return t.contiguous().view(torch.int32)


def _trace(bvh, rays):
    hit, idx, t = bvh.intersect(rays, return_t=True)
    return (hit > 0).to(torch.int32), idx, t


def _outer64(c):
    Vo, Fo, ior, th = c['meshes'][:4]
    ts = c['ts']
    return (Vo.astype(np.float64), Fo.astype(np.int64), ts.outer.normals.cpu().numpy().astype(np.float64), ior.astype(np.float64),
            th.astype(np.float64), ts.curvature.cpu().numpy().astype(np.float64))


# ---- 1. / 2. the crossing ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crossing(inside):
    """The rows of one direction, the device's crossing, the float64 oracle's (with margins) and shell_refraction's."""
    from nu_nerf_amd import relight as R
    gpu = torch.device('cuda', torch.cuda.current_device())
    rows = TO.random_rows(N_ROWS + N_FLAT, inside, 21 + int(inside), flat=N_FLAT)
    dev = R.thin_cross(*[torch.from_numpy(a).to(gpu) for a in rows], inside)
    dev = {k: v.cpu().numpy() for k, v in dev.items()}
    rows64 = [a.astype(np.float64) for a in rows]
    return rows, dev, TO.cross(*rows64, inside), TO.cross_ref(*rows64, inside)


def _crossing_errors(got, ref, sel, gk):
    """Largest absolute deviation of the positions on the rows with |gk| >= 1e-6, on the flat rows, and of normal and direction."""
    flat = np.abs(gk) < 1e-6
    curved, flats = (max(np.abs(got[k][sel & m] - ref[k][sel & m]).max() for k in ('end', 'next_start')) for m in (~flat, flat))
    dirs = max(np.abs(got[k][sel] - ref[k][sel]).max() for k in ('normal', 'next_dir'))
    return curved, flats, dirs


@pytest.mark.parametrize("inside", [False, True])
def test_crossing_matches_shell_refraction_in_float64(gpu, inside):
    rows, dev, ora, ref = _crossing(inside)
    n = len(rows[0])
    assert np.array_equal(ora['refracts'], ref['refracts']) and np.array_equal(ora['tir_ok'], ref['tir_ok'])
    near = ora['margin'] <= MARGIN
    flips = (dev['refracts'] != ref['refracts']) | (dev['tir_ok'] != ref['tir_ok'])
    sel = ~near & ref['refracts']
    pos, pos_flat, dirs = _crossing_errors(dev, ref, sel, rows[5])
    flat = np.abs(rows[5]) < 1e-6
    fres = max(np.abs(dev['fresnel'][~near, 0] - ora['F_a'][~near]).max(), np.abs(dev['fresnel'][~near, 1] - ora['F_b'][~near]).max())
    print(f"crossing {'leaving' if inside else 'entering'}: {n} rows, refracts {ref['refracts'].mean():.1%}, tir_ok {ref['tir_ok'].mean():.1%}; "
          f"left out {near.sum()} ({near.mean():.3%}; first face {(ora['margin1'] <= MARGIN).mean():.3%}), device flags differ on {flips.sum()} rows "
          f"({flips.mean():.3%}); positions {pos:.3e} on rows with |gk| >= 1e-6 (bound {TOL_CROSS_POS:.3e}), {pos_flat:.3e} on the "
          f"{(flat & sel).sum()} flat rows (bound {TOL_CROSS_POS_FLAT:.3e}), normal and direction {dirs:.3e} (bound {TOL_CROSS_DIR:.3e}), Fresnel "
          f"{fres:.3e} (bound {TOL_CROSS_F:.3e})")
    assert near.mean() <= MARGIN_CAP and not flips[~near].any()
    assert 0.5 < ref['refracts'].mean() < 0.95 and (ref['refracts'] & ~ref['tir_ok']).sum() > 50
    assert (flat & sel).sum() >= N_FLAT // 2 and ((rows[5] < 0) & sel).sum() > 1000 and ((rows[5] > 0) & sel).sum() > 1000
    assert pos <= TOL_CROSS_POS and pos_flat <= TOL_CROSS_POS_FLAT and dirs <= TOL_CROSS_DIR and fres <= TOL_CROSS_F
    lost = ~near & ~ref['refracts']                                # a row that does not refract: end = x, zeros, F = 1 (0 index-matched), 0
    assert np.array_equal(dev['end'][lost], rows[2][lost]) and not dev['next_start'][lost].any() and not dev['next_dir'][lost].any()
    assert np.array_equal(dev['fresnel'][lost], np.stack([ora['F_a'][lost], ora['F_b'][lost]], 1).astype(np.float32))
    assert (dev['fresnel'] >= 0).all() and (dev['fresnel'] <= 1).all()


@pytest.mark.parametrize("inside", [False, True])
def test_crossing_matches_nu_s2_shell_fwd(gpu, inside):
    """The same rows through the trained kernel (fed the fp32 logits of the baked values): equal flags outside the exclusions, values within
    the bounds of the float64 comparison -- the two differ by FMA contraction and by the rounding of sigmoid(logit)."""
    from nu_nerf_amd import _lib as L
    rows, dev, ora, _ = _crossing(inside)
    n = len(rows[0])
    ior_raw, th_raw = (a.astype(np.float32) for a in TO.logits(rows[3], rows[4]))
    d, nrm, x, _, _, gk = (torch.from_numpy(a).to(gpu) for a in rows)
    ior_raw, th_raw = torch.from_numpy(ior_raw).to(gpu), torch.from_numpy(th_raw).to(gpu)
    refr, ok = (torch.empty(n, dtype=torch.uint8, device=gpu) for _ in range(2))
    eta = torch.empty(n, device=gpu)
    on, oe, os_, od = (torch.empty(n, 3, device=gpu) for _ in range(4))
    L.load().nu_s2_shell_fwd(L.ptr(d), L.ptr(nrm), L.ptr(x), L.ptr(ior_raw), L.ptr(gk), L.ptr(th_raw), n, 1 if inside else 0, L.ptr(refr),
                             L.ptr(ok), L.ptr(eta), L.ptr(on), L.ptr(oe), L.ptr(os_), L.ptr(od), L.stream())
    s2 = dict(refracts=refr.cpu().numpy() != 0, tir_ok=ok.cpu().numpy() != 0, normal=on.cpu().numpy(), end=oe.cpu().numpy(),
              next_start=os_.cpu().numpy(), next_dir=od.cpu().numpy())
    near = ora['margin'] <= MARGIN
    flips = (dev['refracts'] != s2['refracts']) | (dev['tir_ok'] != s2['tir_ok'])
    sel = ~near & s2['refracts']
    pos, pos_flat, dirs = _crossing_errors({k: v.astype(np.float64) for k, v in dev.items()}, {k: v.astype(np.float64) for k, v in s2.items()},
                                           sel, rows[5])
    print(f"crossing {'leaving' if inside else 'entering'} vs nu_s2_shell_fwd: flags differ on {flips.sum()} rows ({flips.mean():.3%}), positions "
          f"{pos:.3e} on rows with |gk| >= 1e-6 (bound {TOL_CROSS_POS:.3e}), {pos_flat:.3e} on the flat rows (bound {TOL_CROSS_POS_FLAT:.3e}), "
          f"normal and direction {dirs:.3e} (bound {TOL_CROSS_DIR:.3e})")
    assert not flips[~near].any() and pos <= TOL_CROSS_POS and pos_flat <= TOL_CROSS_POS_FLAT and dirs <= TOL_CROSS_DIR


# ---- 3. hits are the tracer's ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['ico2', 'ico3', 'torus', 'ico7'])
def test_every_traced_ray_meets_what_lbvh_trace_finds(gpu, name):
    from nu_nerf_amd import relight as R
    c = _case(name)
    ts, seg, aux, kind = c['ts'], c['seg'], c['aux'], c['kind']
    assert c['pix'].numel() > 100 and int((kind == R.INNER).sum()) > 10 and int((kind == R.EXIT).sum()) > 50 and int((kind == R.DARK).sum()) > 10
    # the entries without dump outputs give the same bits
    k2, ch2, ir2 = R.thin_chain(ts, c['gbuf'], c['pix'])
    assert torch.equal(k2, kind) and torch.equal(_i(ch2), _i(c['chain'])) and torch.equal(_i(ir2), _i(c['irow']))
    assert torch.equal(_i(R.thin_light(ts, c['irow'], c['sel'], c['S'], 0, c['S'], c['seed'])), _i(c['rec']))
    walked = _i(seg[:, 15]) == 1
    assert torch.equal(walked, _i(c['chain'][:, 10]) == 1) and not bool(seg[~walked].any())
    s = seg[walked]
    fi, ii, ti = _trace(ts.inner.bvh, s[:, :6])
    fo, io, to = _trace(ts.outer.bvh, s[:, :6])
    assert torch.equal(_i(s[:, 9]), fi) and torch.equal(_i(s[:, 10]), ii) and torch.equal(_i(s[:, 11]), _i(ti))
    assert torch.equal(_i(s[:, 12]), fo) and torch.equal(_i(s[:, 13]), io) and torch.equal(_i(s[:, 14]), _i(to))
    ends_inner = (fi == 1) & ((fo == 0) | (ti <= to))
    which = torch.where(ends_inner, 1, torch.where(fo == 1, 2, 0)).to(torch.int32)
    assert torch.equal(_i(s[:, 6]), which)
    assert torch.equal(_i(s[:, 7]), torch.where(ends_inner, ii, io)) and torch.equal(_i(s[:, 8]), _i(torch.where(ends_inner, ti, to)))
    assert torch.equal(kind[walked] == R.INNER, ends_inner)
    for k in range(2):                                      # reflection ray, exit ray: any hit = the closest-hit predicate
        a = aux[:, k]
        tr = a[:, 6] == 1
        assert bool(tr.any()) and torch.equal((a[tr, 7] == 1).to(torch.int32), _trace(ts.outer.bvh, a[tr, :6])[0])
        assert not bool(a[~tr, 7].any())
    assert torch.equal(c['chain'][:, 9], ((aux[:, 0, 6] == 1) & (aux[:, 0, 7] == 0)).float())
    ex = kind == R.EXIT
    assert torch.equal(c['chain'][ex, 4], ((aux[ex, 1, 6] == 0) | (aux[ex, 1, 7] == 0)).float())
    # light paths
    d = c['ldump']
    tr = d[:, 6] == 1
    assert 0.3 < float(tr.float().mean()) < 1.0
    assert torch.equal((d[tr, 7] == 1).to(torch.int32), _trace(ts.inner.bvh, d[tr, :6])[0]) and not bool(d[~tr, 7:].any())
    b = tr & (d[:, 7] == 0)
    fo, io, to = _trace(ts.outer.bvh, d[b, :6])
    assert torch.equal((d[b, 8] == 1).to(torch.int32), fo) and torch.equal(_i(d[b, 9]), io) and torch.equal(_i(d[b, 10]), _i(to))
    e = b & (d[:, 8] == 1) & (d[:, 11] == 1)
    assert bool(e.any()) and torch.equal((d[e, 18] == 1).to(torch.int32), _trace(ts.outer.bvh, d[e, 12:18])[0])
    lit = e & (d[:, 18] == 0)
    rec = c['rec'].reshape(-1, 4)
    assert torch.equal(_i(rec[lit]), _i(torch.cat([d[lit, 15:18], d[lit, 19:20]], 1))) and not bool(rec[~lit & ~(b & (d[:, 8] == 0))].any())
    if name == 'torus':                                     # hits that carry negative curvature: the `positive = false` branch, both ways
        g12 = c['gbuf'].reshape(-1, O.ROW)[c['pix'].long(), 12]
        assert int(((g12 < 0) & walked).sum()) > 50 and int(((g12 > 0) & walked).sum()) > 50


# ---- 4. records and image against the float64 oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['ico2', 'ico3', 'torus'])
def test_chain_records_match_the_float64_oracle(gpu, name):
    from nu_nerf_amd import relight as R
    c = _case(name)
    Vo, Fo, VNo, ior, th, gk = _outer64(c)
    rows, _, _ = _rows64(c['gbuf'], c['pix'])
    n = len(rows)
    seg = c['seg'].cpu().numpy()
    segi = seg.view(np.int32)
    aux, chain, kind = c['aux'].cpu().numpy().astype(np.float64), c['chain'].cpu().numpy(), c['kind'].cpu().numpy()
    walked = chain.view(np.int32)[:, 10] == 1
    ev = TO.entry(rows)
    bad = ev['margin'] <= MARGIN
    assert np.array_equal(walked[~bad], ev['enters'][~bad])
    ok = ev['enters'] & walked & ~bad
    good = ~bad
    err = max(np.abs(chain[good, 8] - ev['F_a'][good]).max(), np.abs(chain[good, 5:8] - ev['r'][good]).max())
    err_o = np.abs(seg[ok, :3] - ev['next_start'][ok]).max()
    err = max(err, np.abs(seg[ok, 3:6] - ev['next_dir'][ok]).max())
    T = np.where(ev['enters'], ev['keep'], 0.0)
    at = np.flatnonzero(walked & (segi[:, 6] == 2))
    lv = TO.leave(Vo, Fo, VNo, ior, th, gk, seg[at, :3].astype(np.float64), seg[at, 3:6].astype(np.float64), segi[at, 7].astype(np.int64),
                  R.ORIGIN_EPS)
    nr = lv['margin'] <= MARGIN
    bad[at[nr]] = True
    dev_out = kind[at] == R.EXIT
    assert np.array_equal(dev_out[~nr], lv['out'][~nr])
    out = ~nr & lv['out']
    j = at[out]
    err_o = max(err_o, np.abs(aux[j, 1, :3] - lv['o2'][out]).max())
    err = max(err, np.abs(aux[j, 1, 3:6] - lv['next_dir'][out]).max(), np.abs(chain[j, 1:4] - lv['next_dir'][out]).max())
    T[at] = np.where(lv['out'], T[at] * lv['keep'], 0.0)
    good = ~bad
    err = max(err, err_o, np.abs(chain[good, 0] - np.where(kind[good] == R.DARK, 0.0, T[good])).max())
    r_max = max(_radius(rows[ok, 12]).max(), _radius(lv['gk'][out]).max())
    share = bad.mean()
    kinds = [int((kind == k).sum()) for k in (R.DARK, R.INNER, R.EXIT)]
    print(f"{name}: chain records max deviation {err:.3e} (cavity and exit origins {err_o:.3e}, largest wall radius {r_max:.2f}) over {n} pixels, dark / inner / exit {kinds} (bound {TOL_CHAIN:.3e}); {bad.sum()} pixels "
          f"({share:.2%}) within {MARGIN} of a branch point left out; {int(out.sum())} leaving crossings, {int((lv['gk'] < 0).sum())} at negative curvature")
    assert share <= MARGIN_CAP and err <= TOL_CHAIN
    assert not chain[kind == R.DARK, 0].any() and (chain[:, 0] <= 1).all() and out.sum() > 50
    if name == 'torus':
        assert (lv['gk'][out] < 0).sum() > 20 and (rows[ok, 12] < 0).sum() > 20


def test_inner_rows_match_the_float64_oracle(gpu):
    from nu_nerf_amd import relight as R
    c = _case('ico3')
    Vi, Fi, mat = c['meshes'][4:]
    kind = c['kind'].cpu().numpy()
    sel = np.flatnonzero(kind == R.INNER)
    s = c['seg'].cpu().numpy()[sel]
    assert (s.view(np.int32)[:, 6] == 1).all()
    rows = c['irow'].cpu().numpy()[sel]
    outer_ids = c['gbuf'].reshape(-1, O.ROW)[c['pix'].long()].cpu().numpy().view(np.int32)[sel, 18:20]
    assert np.array_equal(rows.view(np.int32)[:, 18:20], outer_ids) and (outer_ids[:, 0] == 3).all()
    VN = c['ts'].inner.normals.cpu().numpy().astype(np.float64)
    ref = O.gbuffer_rows(Vi.astype(np.float64), Fi.astype(np.int64), VN, mat.astype(np.float64), s[:, :3].astype(np.float64),
                         s[:, 3:6].astype(np.float64), s.view(np.int32)[:, 7].astype(np.int64), 0, 0)
    rows = rows.astype(np.float64)
    err = (np.abs(rows[:, :18] - ref[:, :18]) / np.maximum(1.0, np.abs(ref[:, :18]))).max()
    print(f"inner rows: max deviation {err:.3e} over {len(sel)} pixels (bound {TOL_ATTR:.3e})")
    assert len(sel) > 100 and err <= TOL_ATTR
    assert np.array_equal(rows[:, 15:18].astype(np.float32), -s[:, 3:6])                   # the view vector is minus the cavity direction
    assert not c['irow'][c['kind'] != R.INNER].any()


@pytest.mark.parametrize("name", ['ico3', 'torus'])
def test_light_records_match_the_float64_oracle(gpu, name):
    from nu_nerf_amd import relight as R
    c = _case(name)
    Vo, Fo, VNo, ior, th, gk = _outer64(c)
    d = c['ldump'].cpu().numpy()
    at = np.flatnonzero((d[:, 6] == 1) & (d[:, 7] == 0) & (d[:, 8] == 1))
    lv = TO.leave(Vo, Fo, VNo, ior, th, gk, d[at, :3].astype(np.float64), d[at, 3:6].astype(np.float64), d.view(np.int32)[at, 9].astype(np.int64),
                  R.ORIGIN_EPS)
    nr = lv['margin'] <= MARGIN
    assert np.array_equal((d[at, 11] == 1)[~nr], lv['out'][~nr])
    out = ~nr & lv['out']
    j = at[out]
    err_o = np.abs(d[j, 12:15] - lv['o2'][out]).max()
    err = max(err_o, np.abs(d[j, 15:18] - lv['next_dir'][out]).max(), np.abs(d[j, 19] - lv['keep'][out]).max())
    print(f"{name}: light records max deviation {err:.3e} (exit origins {err_o:.3e}, largest wall radius {_radius(lv['gk'][out]).max():.2f}) over "
          f"{out.sum()} leaving crossings, {int((lv['gk'][out] < 0).sum())} at negative curvature (bound {TOL_LIGHT:.3e}); {nr.sum()} ({nr.mean():.2%}) within {MARGIN} of a branch point left out")
    assert out.sum() > (1000 if name == 'ico3' else 200) and nr.mean() <= MARGIN_CAP and err <= TOL_LIGHT
    assert (d[j, 19] > 0).all() and (d[j, 19] <= 1).all()
    if name == 'torus':
        assert (lv['gk'][out] < 0).sum() > 50


def _image_vs_oracle(c, env, S, seed):
    from nu_nerf_amd import relight as R
    ts, h, w = c['ts'], c['h'], c['w']
    lin = R.relight_nested_linear(ts, env, c['poses'], h, w, S, seed, chunk=S, img0=3)
    rec = torch.zeros(c['pix'].numel(), S, 4, device=lin.device)
    rec[c['sel'].long()] = R.thin_light(ts, c['irow'], c['sel'], S, 0, S, seed)
    rows, img, pixel = _rows64(c['gbuf'], c['pix'])
    ref = NO.resolve(c['kind'].cpu().numpy(), c['chain'].cpu().numpy().astype(np.float64), c['irow'].cpu().numpy().astype(np.float64), img,
                     pixel, rec.cpu().numpy().astype(np.float64), S, seed, env.astype(np.float64))
    got = lin.reshape(-1, 4)[c['pix'].long()].cpu().numpy().astype(np.float64)
    return lin, got, ref


@pytest.mark.parametrize("name,S", [('ico3', 64), ('torus', 16)])
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
    assert torch.equal(img8, R.relight_nested(c['ts'], env, c['poses'], c['h'], c['w'], S, 11, chunk=S, img0=3).reshape(-1, 4))
    d8 = np.abs(img8[c['pix'].long(), :3].cpu().numpy().astype(np.int64) - O.to_srgb8(ref))
    print(f"{name}: 8-bit image max difference {d8.max()} levels")
    assert d8.max() <= 1 and set(np.unique(img8[:, 3].cpu().numpy())) == {0, 255}
    inner = (c['kind'] == R.INNER).cpu().numpy()
    assert got[inner, :3].sum(1).min() > 0 and ref[~inner].max() > 0


# ---- 5. energy under a constant environment ------------------------------------------------------------------------------------------------
def test_constant_environment_never_gains_energy(gpu):
    from nu_nerf_amd import relight as R
    c = _case('ico3')
    env = np.ones((16, 32, 3), np.float32)
    lin, got, ref = _image_vs_oracle(c, env, 16, 11)
    kind, chain = c['kind'].cpu().numpy(), c['chain'].cpu().numpy().astype(np.float64)
    other = kind != R.INNER
    top = got[other, :3].max()
    dark = kind == R.DARK
    refl = chain[:, 8] * chain[:, 9]
    dev = np.abs(got[dark, :3] - refl[dark, None]).max()
    ex = kind == R.EXIT
    want = refl + chain[:, 0] * chain[:, 4]
    dev_ex = np.abs(got[ex, :3] - want[ex, None]).max()
    print(f"constant environment: brightest non-inner pixel {top:.8f} over {other.sum()} pixels; dark pixels vs F vis {dev:.3e} ({dark.sum()}), "
          f"exit pixels vs F vis + T vis {dev_ex:.3e} ({ex.sum()})")
    assert other.sum() > 1000 and dark.sum() > 10 and top <= 1.0 + 1e-6
    assert dev <= 1e-6 and dev_ex <= 1e-6 and (chain[:, 8] + chain[:, 0] <= 1.0 + 1e-6).all()
    assert np.array_equal(got[other, 0], got[other, 1]) and got[ex, 0].mean() > 0.5
    assert (np.abs(got[:, :3] - ref) / np.maximum(np.abs(ref), 1e-2)).max() <= TOL_LINEAR


# ---- 6. determinism and chunk invariance ----------------------------------------------------------------------------------------------------
def test_runs_and_chunkings_are_bit_identical(gpu):
    from nu_nerf_amd import relight as R
    Vo, Fo, ior, th, Vi, Fi, mat = _meshes('ico2')
    ts = R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, device=gpu)
    h, w, S, seed = 30, 38, 48, 2
    env, poses = _env(), _orbit(3, el=30.0, dist=2.2)
    one = R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=S, images=3)
    assert bool((one[..., 3] == 1).any()) and bool((one[..., :3] > 0).any())
    assert torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=S, images=3))
    assert torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=S, images=3, rows=7))
    assert torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=S, images=1, rows=11))
    assert torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=10, images=2, rows=11))
    assert torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed, chunk=48, images=2, rows=7))
    assert torch.equal(one[1:], R.relight_nested_linear(ts, env, poses[1:], h, w, S, seed, img0=1))
    assert not torch.equal(one, R.relight_nested_linear(ts, env, poses, h, w, S, seed + 1))
    fresh = R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, device=gpu)              # a second build of both trees, normals and curvature
    assert torch.equal(one, R.relight_nested_linear(fresh, env, poses, h, w, S, seed))
    # the solid shell of the same meshes is another picture, and still the one it was
    solid = R.NestedScene(Vo, Fo, np.maximum(ior, 1.0), Vi, Fi, mat, device=gpu)
    assert not torch.equal(one, R.relight_nested_linear(solid, env, poses, h, w, S, seed))
    # an explicit curvature is used as given
    assert torch.equal(one, R.relight_nested_linear(R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, curvature=ts.curvature, device=gpu), env,
                                                    poses, h, w, S, seed))
    assert not torch.equal(one, R.relight_nested_linear(R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, curvature=-4.0, device=gpu), env,
                                                        poses, h, w, S, seed))


def test_bad_arguments_are_refused(gpu):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd import relight as R
    c = _case('ico2')
    ts, irow, sel, chain, kind, pix = c['ts'], c['irow'], c['sel'], c['chain'], c['kind'], c['pix']
    with pytest.raises(RuntimeError, match="nu_relight_thin_light"):
        R.thin_light(ts, irow, sel, 15, 0, 4, 0)
    with pytest.raises(RuntimeError, match="nu_relight_thin_light"):
        R.thin_light(ts, irow, sel, 16, 10, 7, 0)
    lib, a = L.load(), list(ts._args())
    tail = (L.ptr(c['gbuf']), L.ptr(pix), int(pix.numel()), 1e-4, L.ptr(kind.clone()), L.ptr(chain.clone()), L.ptr(irow.clone()), L.stream())
    for k in (0, 2, 5, 6, 11, 12, 13):
        with pytest.raises(RuntimeError, match="nu_relight_thin_chain"):
            lib.nu_relight_thin_chain(*(a[:k] + [None] + a[k + 1:]), *tail)
    with pytest.raises(RuntimeError, match="nu_relight_thin_chain"):
        lib.nu_relight_thin_chain(*a, None, *tail[1:])
    empty = pix[:0]
    k0, ch0, ir0 = R.thin_chain(ts, c['gbuf'], empty)
    assert k0.numel() == 0 and R.thin_light(ts, irow, empty, 16, 0, 16, 0).shape == (0, 16, 4)
    z = torch.zeros(0, 3, device=gpu)
    assert R.thin_cross(z, z, z, z[:, 0], z[:, 0], z[:, 0], True)['next_dir'].shape == (0, 3)
    with pytest.raises(ValueError):
        R.relight_nested_linear(ts, _env(), c['poses'], 8, 8, 7)
    assert np.allclose(ts.curvature.cpu().numpy(), 4.0, atol=0.7)                  # the angle-defect curvature of a sphere of radius 0.5


# ---- 7. bake ------------------------------------------------------------------------------------------------------------------------------
def _ior_module64(holder, X):
    """float64 evaluation of an IoRNetwork parameter holder on encoded points X [P,39]: weight-normed linear layers 0, 2, 4, 5 with a
    ReLU after the first two, then the sigmoid."""
    y = X
    for k in (0, 2, 4, 5):
        lay = holder.module0[k]
        g, v, b = (p.detach().double().cpu() for p in (lay.weight_g, lay.weight_v, lay.bias))
        y = y @ (g * v / v.norm(dim=1, keepdim=True)).t() + b
        if k in (0, 2):
            y = torch.relu(y)
    return torch.sigmoid(y)


def test_predict_shell_is_the_shell_the_model_trains(gpu):
    from nu_nerf_amd import materials as M
    from nu_nerf_amd import torch_glue as G
    from test_materials_gpu import stage1_net, stage2_net
    net, _ = stage2_net(gpu, thick=True)
    V, F = _ico(2)
    got = M.predict_shell(net, (V, F))
    assert sorted(got) == ['ior', 'thickness'] and all(v.shape == (len(V), 1) and v.dtype == np.float32 for v in got.values())
    x = torch.from_numpy(V).to(gpu)
    with torch.no_grad():
        ior_raw, th_raw = net.nets()[1].ior_and_thickness(G.embed(x, 6))
        want_i = (torch.sigmoid(ior_raw).reshape(-1, 1) * 1.0 + 0.6).cpu().numpy()
        want_t = (torch.sigmoid(th_raw).reshape(-1, 1) * 0.01).cpu().numpy()
    assert np.array_equal(got['ior'], want_i) and np.array_equal(got['thickness'], want_t)
    x64 = torch.from_numpy(V).double()
    X = torch.cat([x64] + [f(x64 * 2.0 ** k) for k in range(6) for f in (torch.sin, torch.cos)], -1)
    ref_i = (_ior_module64(net.IORs_pred, X) + 0.6).numpy()
    ref_t = (_ior_module64(net.thickness_pred, X) * 0.01).numpy()
    err = max((np.abs(got['ior'] - ref_i) / ref_i).max(), (np.abs(got['thickness'] - ref_t) / ref_t).max())
    print(f"predict_shell: max relative deviation from the float64 evaluation {err:.3e} (bound {TOL_BAKE:.3e})")
    assert err <= TOL_BAKE
    assert (got['ior'] > 0.6).all() and (got['ior'] < 1.6).all() and (got['thickness'] > 0).all() and (got['thickness'] < 0.01).all()
    assert got['ior'].std() > 0 and got['thickness'].std() > 0
    # predict_ior keeps the zero-thickness formula on the same model
    assert np.allclose(M.predict_ior(net, (V, F)), got['ior'] + 0.4, atol=1e-6)
    for other in (stage1_net(gpu)[0], stage2_net(gpu)[0]):
        with pytest.raises(ValueError):
            M.predict_shell(other, (V, F))


def test_extract_materials_writes_the_shell_of_a_thick_checkpoint(gpu, tmp_path, monkeypatch):
    import yaml
    from nu_nerf_amd import extract_materials
    from nu_nerf_amd import materials as M
    from nu_nerf_amd.mesh import write_ply
    from test_materials_gpu import stage2_net
    net, _ = stage2_net(gpu, thick=True)
    Vo, Fo = net._mesh
    Vi, Fi = _ico(1, 0.2)
    monkeypatch.chdir(tmp_path)
    write_ply('outer.ply', Vo, Fo)
    write_ply('inner.ply', np.asarray(Vi, np.float32), Fi)
    cfg = {k: v for k, v in net.cfg.items() if k in ('name', 'network', 'is_nerf', 'get_mask', 'shader_config', 'stage1_cfg')}
    cfg.update(zero_thickness=False, stage1_mesh_dir='outer.ply')
    with open('s2.yaml', 'w') as fh:
        yaml.safe_dump(cfg, fh)
    torch.save({'step': 55, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 's2.pth')
    out = extract_materials.main(['--cfg', 's2.yaml', '--stage2', '--ckpt', 's2.pth', '--mesh', 'inner.ply', '--out', 'baked'])
    assert sorted(os.listdir(out)) == ['albedo.npy', 'ior.npy', 'metallic.npy', 'roughness.npy', 'shell_ior.npy', 'shell_thickness.npy']
    shell = M.predict_shell(net, (Vo, Fo))
    assert np.array_equal(np.load('baked/shell_ior.npy'), shell['ior']) and np.array_equal(np.load('baked/shell_thickness.npy'), shell['thickness'])
    assert np.array_equal(np.load('baked/ior.npy'), M.predict_ior(net, (Vo, Fo)))              # as before: the zero-thickness formula


# ---- 8. the command -----------------------------------------------------------------------------------------------------------------------
def test_command_end_to_end(gpu, tmp_path, monkeypatch):
    from PIL import Image
    from nu_nerf_amd import mesh as M
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.extract_materials import save_shell
    Vo, Fo, ior, th, Vi, Fi, mat = _meshes('ico2')
    M.write_ply(str(tmp_path / 'outer.ply'), Vo, Fo)
    M.write_ply(str(tmp_path / 'inner.ply'), Vi, Fi)
    os.makedirs(tmp_path / 'mat')
    np.save(tmp_path / 'mat' / 'albedo.npy', mat[:, :3])
    np.save(tmp_path / 'mat' / 'metallic.npy', mat[:, 3:4])
    np.save(tmp_path / 'mat' / 'roughness.npy', mat[:, 4:5])
    save_shell(str(tmp_path / 'mat'), {'ior': ior, 'thickness': th})
    np.save(tmp_path / 'env.npy', _env())
    monkeypatch.chdir(tmp_path)
    argv = ['--mesh', 'outer.ply', '--inner', 'inner.ply', '--inner-material', 'mat', '--shell', 'mat', '--hdr', 'env.npy', '--name', 'bottle',
            '--num', '2', '--width', '32', '--height', '32', '--samples', '16', '--cam_dist', '2.2']
    out = R.main(argv)
    assert out == os.path.join('data', 'relight', 'bottle')
    ts = R.ThinShellScene(Vo, Fo, ior, th, Vi, Fi, mat, device=gpu)
    poses = R.camera_in_mesh_frame(R.relighting_poses(2, 0.0, 45.0, 2.2))
    frames = []
    for k in range(2):
        with Image.open(os.path.join(out, f'{k}.png')) as im:
            assert im.mode == 'RGBA' and im.size == (32, 32)
            frames.append(np.asarray(im).copy())
        want = R.relight_nested(ts, _env(), poses[k:k + 1], 32, 32, 16, 0, img0=k)
        assert np.array_equal(want[0].cpu().numpy(), frames[k]) and set(np.unique(frames[k][..., 3])) == {0, 255}
    # two numbers give a uniform shell: another picture, the one ThinShellScene renders for them
    R.main(argv[:7] + ['1.45,0.005'] + argv[8:] + ['--output', 'uniform'])
    with Image.open(os.path.join('uniform', '1.png')) as im:
        uni = np.asarray(im).copy()
    want = R.relight_nested(R.ThinShellScene(Vo, Fo, 1.45, 0.005, Vi, Fi, mat, device=gpu), _env(), poses[1:2], 32, 32, 16, 0, img0=1)
    assert np.array_equal(want[0].cpu().numpy(), uni) and not np.array_equal(uni, frames[1])
    # without --shell the command is the solid shell it was
    R.main(argv[:6] + ['--ior', '1.45'] + argv[8:] + ['--output', 'solid'])
    with Image.open(os.path.join('solid', '1.png')) as im:
        solid = np.asarray(im).copy()
    want = R.relight_nested(R.NestedScene(Vo, Fo, 1.45, Vi, Fi, mat, device=gpu), _env(), poses[1:2], 32, 32, 16, 0, img0=1)
    assert np.array_equal(want[0].cpu().numpy(), solid) and not np.array_equal(solid, uni)
