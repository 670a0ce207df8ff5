"""Every entry of csrc/sampler.hip alone, through the C ABI, against the float64 oracle of tests/sampler_oracle.py (anchored on the
stage-1 oracle by tests/test_sampler_oracle_host.py): nu_upsample and nu_probe_weights judged in CDF space, EVERY sample of every ray
against its own bound B (no percentile, nothing left out); nu_sample_coarse, nu_merge_sorted and nu_concat_cols bit for bit; and the
loop of engine.sample_ray with an analytic SDF between the kernels.

Every output buffer starts filled with NaN and has one guard row past R.  The cases (families of rays, sn across every change of the
intervals-per-lane count, n_new, R, the three inv_s rules, quantiles with 0 and 1.0) are sampler_oracle.CASES; the bound, the
derivation of each of its terms and the measured constants are in that module's docstring.

Measured on an MI355X (each check prints its figure, run with -s): largest residual / bound 0.32 for nu_upsample (through-sn3), 0.22
for nu_probe_weights (through-sn3), 0.13 in the chain; wsum error / bound 0.24 (ties-sn2); the file takes 5 s, 2.6 s of them the first
import.  DESIGN.md section 33 lists which of these tests fails for each of seven mutants of the kernels."""
import pytest
import torch

import sampler_oracle as S

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope="module")
def K(gpu):
    from nu_nerf_amd import _lib as L

    class Ctx:
        lib = L.load()
        err = L.NuNerfLibraryError
        live = []                          # device copies made by dev(): kept until the call that reads them has finished

        @staticmethod
        def ptr(t):
            return L.ptr(t)

        @staticmethod
        def nan(*shape):
            return torch.full(shape, NAN, device=gpu)

        @classmethod
        def dev(cls, t):
            cls.live.append(t.float().to(gpu).contiguous())
            return cls.live[-1]

        @classmethod
        def call(cls, name, *args):
            try:
                L.check(getattr(cls.lib, name)(*args, L.stream()), name)
            finally:
                torch.cuda.synchronize()
                cls.live.clear()
    return Ctx


def _untouched(t):
    return t is None or bool(torch.isnan(t).all())


def _run_round(K, mode, o, d, z, sdf, var, cap, use_var, u, with_wsum=True, with_samples=True):
    """One launch of nu_upsample (mode 0) or nu_probe_weights (mode 1) on CPU fp32 inputs -> (z_new [R, n], Xn [R, n, 3], wsum [R]) on
    the CPU; checks that the guard rows past R stay untouched."""
    R, sn = z.shape
    n = u.shape[0] if with_samples else 0
    zn = K.nan(R + 1, n) if n else None
    Xn = K.nan((R + 1) * n, 3) if n else None
    ws = K.nan(R + 1) if (mode == 1 and with_wsum) else None
    p, dv = K.ptr, K.dev
    head = (p(dv(o)), p(dv(d)), p(dv(z)), p(dv(sdf)), R, sn, p(dv(torch.tensor([var]))))
    tail = (p(dv(u)) if n else p(None), n, p(zn), p(Xn))
    if mode == 0:
        K.call('nu_upsample', *head, float(cap), int(use_var), *tail)
    else:
        K.call('nu_probe_weights', *head, *tail, p(ws))
    if n:
        assert _untouched(zn[R:]) and _untouched(Xn[R * n:])
        zn, Xn = zn[:R].cpu(), Xn[:R * n].cpu().view(R, n, 3)
    if ws is not None:
        assert _untouched(ws[R:])
        ws = ws[:R].cpu()
    return zn, Xn, ws


def _judge_round(mode, o, d, z, sdf, inv_s, u, zn, Xn, ends, tag):
    """The checks of one round's new depths; returns the largest residual / bound."""
    R, sn = z.shape
    assert bool(torch.isfinite(zn).all()) and bool(torch.isfinite(Xn).all())                        # every slot written
    raw64 = S.weights64(o, d, z, sdf, inv_s, mode)
    j = S.cdf_residual(z, raw64, zn, u)
    B = S.bound(z, j, S.arg_term64(o, d, z, sdf, inv_s, mode))
    frac = float((j.res / B).max())
    print(f"{tag}: largest residual {float(j.res.max()):.2e}, largest residual / bound {frac:.3f}")
    worst = int((j.res / B).argmax())
    assert bool((j.res <= B).all()), (tag, divmod(worst, zn.shape[1]), float(j.res.flatten()[worst]), float(B.flatten()[worst]))
    assert bool((zn[:, 1:] >= zn[:, :-1]).all())                                                      # the quantiles ascend: so do the depths
    assert bool((zn >= z[:, :1]).all()) and bool((zn <= z[:, -1:]).all())
    if ends:
        assert float(u[0]) == 0.0 and float(u[-1]) == 1.0
        assert torch.equal(zn[:, 0], z[:, 0]) and torch.equal(zn[:, -1], z[:, -1])
    # the points handed to the next SDF evaluation: o + d * z_new in separately rounded fp32 operations, of the z this launch wrote
    assert torch.equal(Xn, o[:, None, :] + d[:, None, :] * zn[..., None])
    return frac


@pytest.mark.parametrize("c", [c for c in S.CASES if c.mode == 0], ids=lambda c: c.id)
def test_upsample_every_sample_within_its_cdf_bound(K, c):
    o, d, z, sdf, u = S.make_case(c)
    cap, use_var = 64.0 * 2 ** c.rnd, c.kind != 'cap'
    zn, Xn, _ = _run_round(K, 0, o, d, z, sdf, c.var, cap, use_var, u)
    _judge_round(0, o, d, z, sdf, S.inv_s64(c.var, cap, use_var, 0), u, zn, Xn, c.ends and c.n_new >= 3, c.id)


@pytest.mark.parametrize("c", [c for c in S.CASES if c.mode == 1], ids=lambda c: c.id)
def test_probe_weights_every_sample_and_wsum_within_bound(K, c):
    o, d, z, sdf, u = S.make_case(c)
    if c.fam in ('probe', 'inside'):
        assert bool((z[:, 0] == 0).any())                                                             # rows that start at the probe's own point
    inv_s = S.inv_s64(c.var, 0.0, False, 1)
    zn, Xn, ws = _run_round(K, 1, o, d, z, sdf, c.var, 0.0, False, u)                                 # everything at once
    _judge_round(1, o, d, z, sdf, inv_s, u, zn, Xn, c.ends and c.n_new >= 3, c.id)
    raw64 = S.weights64(o, d, z, sdf, inv_s, 1)
    err = (ws.double() - S.wsum64(raw64)).abs()
    tol = S.KW * S.U24 * (c.sn - 1)
    print(f"{c.id}: wsum error / bound {float(err.max()) / tol:.3f}")
    assert bool((err <= tol).all()), (float(err.max()), tol)
    if c.fam == 'rising':                                                                             # no interval has cos < 0: every alpha is masked
        assert bool((raw64 == 0).all()) and bool((ws == 0).all())
    # the two forms the occlusion probe uses: samples without wsum, then wsum alone (n_new = 0, uvals / z_new / Xn NULL)
    zn2, Xn2, none = _run_round(K, 1, o, d, z, sdf, c.var, 0.0, False, u, with_wsum=False)
    assert none is None and torch.equal(zn2, zn) and torch.equal(Xn2, Xn)
    none_z, none_x, ws2 = _run_round(K, 1, o, d, z, sdf, c.var, 0.0, False, u, with_samples=False)
    assert none_z is None and none_x is None and torch.equal(ws2, ws)


@pytest.mark.parametrize("entry", ['nu_upsample', 'nu_probe_weights'])
@pytest.mark.parametrize("sn", [1, 257])
def test_rounds_reject_sn_outside_2_to_256_and_write_nothing(K, entry, sn):
    R, n = 5, 8
    g = torch.Generator().manual_seed(sn)
    o, d = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    z = torch.sort(torch.rand(R, sn, generator=g), dim=-1).values
    zn, Xn, ws = K.nan(R, n), K.nan(R * n, 3), K.nan(R)
    p, dv = K.ptr, K.dev
    head = (p(dv(o)), p(dv(d)), p(dv(z)), p(dv(z)), R, sn, p(dv(torch.tensor([0.3]))))
    tail = (p(dv(S.quantiles(n, False))), n, p(zn), p(Xn))
    with pytest.raises(K.err, match=f"{entry} failed with code -1"):
        K.call(entry, *head, *((64.0, 0) if entry == 'nu_upsample' else ()), *tail, *((p(ws),) if entry == 'nu_probe_weights' else ()))
    assert _untouched(zn) and _untouched(Xn) and _untouched(ws)


@pytest.mark.parametrize("R,Nc,Nbg,form", [
    (37, 64, 32, 'jitter'), (5, 24, 8, 'jitter'), (400, 16, 8, 'plain'), (1, 64, 32, 'plain'), (37, 64, 0, 'probe'), (400, 16, 0, 'probe')])
def test_sample_coarse_bit_for_bit(K, R, Nc, Nbg, form):
    """zc, zbg (stored reversed) and X equal sample_ray's expressions (renderer_zerothick.py:572-592) evaluated in fp32 torch on the
    CPU: each is a chain of separately rounded fp32 operations in the reference's order, the file compiles with contraction off."""
    g = torch.Generator().manual_seed(R + Nc)
    o = torch.randn(R, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    near = torch.zeros(R) if form == 'probe' else 0.5 + torch.rand(R, generator=g)
    far = near + 1.0 + 2.0 * torch.rand(R, generator=g)
    lin = torch.linspace(0.0, 1.0, Nc)
    u1 = torch.rand(R, generator=g) if form == 'jitter' else None
    u2 = torch.rand(R, Nbg, generator=g) if form == 'jitter' else None
    zc, X = K.nan(R + 1, Nc), K.nan((R + 1) * Nc, 3)
    zbg = K.nan(R + 1, Nbg) if Nbg else None
    p, dv = K.ptr, K.dev
    if form == 'probe':                                   # engine.occ_probe: Nbg = 0, the four optional inputs and zbg NULL
        bins = (p(None), p(None), p(None), p(None))
    else:
        lin_bg, lower, upper = S.bg_bins(Nbg)
        bins = (p(dv(lower if u2 is not None else lin_bg)), p(dv(upper)), p(dv(u1)) if u1 is not None else p(None),
                p(dv(u2)) if u2 is not None else p(None))
    K.call('nu_sample_coarse', p(dv(o)), p(dv(d)), p(dv(near)), p(dv(far)), p(dv(lin)), *bins, R, Nc, Nbg, p(zc), p(zbg), p(X))
    want = S.coarse_depths(near, far, lin, u1, Nc)
    assert torch.equal(zc[:R].cpu(), want)
    assert torch.equal(X[:R * Nc].cpu().view(R, Nc, 3), o[:, None, :] + d[:, None, :] * want[..., None])
    assert _untouched(zc[R:]) and _untouched(X[R * Nc:])                                              # nothing beyond R * Nc rows
    if Nbg:
        assert torch.equal(zbg[:R].cpu(), S.bg_depths(far, lower if u2 is not None else lin_bg, upper, u2, Nbg))
        assert _untouched(zbg[R:])
    if form == 'probe':
        assert bool((zc[:R, 0] == 0).all())


def _tied_rows(R, n, g):
    """Sorted rows on the lattice k / 8: equal depths within a row and across two such rows are the rule."""
    return torch.sort(torch.randint(0, max(n // 2, 3), (R, n), generator=g).float() / 8.0, dim=-1).values.contiguous()


@pytest.mark.parametrize("R,sn,nn,last", [(37, 64, 64, False), (5, 192, 64, False), (1, 3, 2, False), (130, 40, 8, False), (37, 192, 64, True)])
def test_merge_sorted_ties_old_before_new(K, R, sn, nn, last):
    g = torch.Generator().manual_seed(R + sn)
    z, zn = _tied_rows(R, sn, g), _tied_rows(R, nn, g)
    s, s_n = torch.randn(R, sn, generator=g), torch.randn(R, nn, generator=g)
    assert bool((z[:, :, None] == zn[:, None, :]).any()) and (nn < 8 or bool((zn[:, 1:] == zn[:, :-1]).any()))
    want_z, want_s = S.merge(z, s, zn, s_n)
    zo, so = K.nan(R + 1, sn + nn), K.nan(R + 1, sn + nn)
    p, dv = K.ptr, K.dev
    K.call('nu_merge_sorted', p(dv(z)), p(dv(s)), sn, p(dv(zn)), p(None if last else dv(s_n)), nn, R, p(zo), p(None if last else so))
    assert torch.equal(zo[:R].cpu(), want_z) and _untouched(zo[R:])
    if last:
        assert _untouched(so)                             # the last round carries no SDF
    else:
        assert torch.equal(so[:R].cpu(), want_s) and _untouched(so[R:])


def test_merge_sorted_rejects_65_new_samples(K):
    R, sn, nn = 3, 16, 65
    g = torch.Generator().manual_seed(0)
    z, zn = _tied_rows(R, sn, g), _tied_rows(R, nn, g)
    zo, so = K.nan(R, sn + nn), K.nan(R, sn + nn)
    p, dv = K.ptr, K.dev
    with pytest.raises(K.err, match="nu_merge_sorted failed with code -1"):
        K.call('nu_merge_sorted', p(dv(z)), p(dv(z)), sn, p(dv(zn)), p(dv(zn)), nn, R, p(zo), p(so))
    assert _untouched(zo) and _untouched(so)


@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("a,b", [(1, 1), (128, 16), (160, 32)])
def test_concat_cols_exact(K, a, b, R):
    g = torch.Generator().manual_seed(a + R)
    A, B = torch.randn(R, a, generator=g), torch.randn(R, b, generator=g)
    out = K.nan(R + 1, a + b)
    K.call('nu_concat_cols', K.ptr(K.dev(A)), a, K.ptr(K.dev(B)), b, R, K.ptr(out))
    assert torch.equal(out[:R].cpu(), torch.cat([A, B], -1)) and _untouched(out[R:])


@pytest.mark.parametrize("R,Nc,Nbg,n_new,jitter,clip,seed", [(37, 64, 32, 16, True, False, 5), (6, 32, 8, 8, False, True, 6)])
def test_chain_with_an_analytic_sdf(K, R, Nc, Nbg, n_new, jitter, clip, seed):
    """coarse -> four rounds of upsample / merge -> concat, the loop of engine.sample_ray, with the analytic SDF of the families
    (float64 at the X / Xn the kernels emit, rounded to fp32) where the engine runs the network.  Each round is judged in CDF space on
    the inputs that round received, so no difference of an earlier round enters a later one."""
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5
    d = torch.nn.functional.normalize(-o + 0.35 * torch.randn(R, 3, generator=g), dim=-1)
    mid = -(o * d).sum(-1)
    near, far = mid - 1.0, mid + 1.0
    lin = torch.linspace(0.0, 1.0, Nc)
    lin_bg, lower, upper = S.bg_bins(Nbg)
    u1 = torch.rand(R, generator=g) if jitter else None
    u2 = torch.rand(R, Nbg, generator=g) if jitter else None
    var = 0.3
    p, dv = K.ptr, K.dev
    zc, zbg, X = K.nan(R, Nc), K.nan(R, Nbg), K.nan(R * Nc, 3)
    K.call('nu_sample_coarse', p(dv(o)), p(dv(d)), p(dv(near)), p(dv(far)), p(dv(lin)), p(dv(lower if jitter else lin_bg)), p(dv(upper)),
           p(dv(u1)) if jitter else p(None), p(dv(u2)) if jitter else p(None), R, Nc, Nbg, p(zc), p(zbg), p(X))
    zc, zbg = zc.cpu(), zbg.cpu()
    z, sdf = zc, S.sdf_analytic(X.cpu().double()).float().view(R, Nc)
    u = S.quantiles(n_new, False)
    for i in range(4):
        cap = 64.0 * 2 ** i
        d_radius, d_clip = S.input_conditions(None, o, d, z, sdf)
        assert d_radius > 4e-6 and d_clip > 1e-3, "this seed puts a sample on a threshold an fp32 kernel may decide differently"
        zn, Xn, _ = _run_round(K, 0, o, d, z, sdf, var, cap, clip, u)
        _judge_round(0, o, d, z, sdf, S.inv_s64(var, cap, clip, 0), u, zn, Xn, False, f"chain R{R} round {i}")
        last = i == 3
        s_n = None if last else S.sdf_analytic(Xn.double()).float()
        sn = z.shape[1]
        zo, so = K.nan(R, sn + n_new), (None if last else K.nan(R, sn + n_new))
        K.call('nu_merge_sorted', p(dv(z)), p(dv(sdf)), sn, p(dv(zn)), p(None if last else dv(s_n)), n_new, R, p(zo), p(so))
        want_z, want_s = S.merge(z, None if last else sdf, zn, s_n)
        assert torch.equal(zo.cpu(), want_z)
        if not last:
            assert torch.equal(so.cpu(), want_s)
        z, sdf = zo.cpu(), (None if last else so.cpu())
    sn = z.shape[1]
    out = K.nan(R, sn + Nbg)
    K.call('nu_concat_cols', p(dv(z)), sn, p(dv(zbg)), Nbg, R, p(out))
    out = out.cpu()
    assert sn == Nc + 4 * n_new and bool((out[:, 1:] >= out[:, :-1]).all())                          # sorted, the background tail included
    assert bool((out[:, :sn, None] == zc[:, None, :]).any(1).all())                                   # every coarse depth is still there
    assert torch.equal(out[:, sn:], zbg)
