"""tests/sampler_oracle.py on the CPU, before tests/test_sampler_cdf_gpu.py judges a kernel with it:
  * its float64 formulas equal oracle/stage1_oracle.py's upsample / sample_pdf / get_weights run in float64 on the same data (1e-12),
    and in fp32 they ARE that oracle (the same bits), so "the fp32 CPU oracle" below is the repository's one;
  * every case of the GPU file keeps clear of the two thresholds an fp32 kernel may decide differently (no exclusions: seeds);
  * the constants K and KW of the bound are re-derived: the fp32 CPU oracle, judged in CDF space, stays within K / 4 and KW / 4;
  * the bound can fail: three wrong results break it.

K_ref = max over the samples of (residual - flat - slope term - A)+ total / (ni 2^-24) of the fp32 CPU oracle, K_w = max over the rows
of |wsum32 - wsum64| / (ni 2^-24); largest value per family over its cases (every case prints its own, run with -s); "no A" is K_ref
with the derived argument term A (sampler_oracle.arg_term64) left out of the bound, "max A" the largest A of a row:

                        through   miss    graze   inside   ties    second   probe   rising
  mode 0  K_ref         0.067     0.000   0.239   0.000    0.034   0.073
          no A          0.405     0.000   6.419   0.073    9.947   0.144
          max A         9.2e-5    1.0e-7  5.6e-5  4.1e-3   3.6e-5  2.7e-4
  mode 1  K_ref         0.145                     0.000    0.055   0.055    0.140   0.000
          no A          0.230                     0.059    0.115   0.110    0.192   0.000
          K_w           0.792                     0.212    1.661   0.794    0.510   0 (exactly)
          max A         7.7e-5                    5.8e-4   5.5e-4  3.6e-5   5.9e-4  0

K_REF_MAX = 0.25 and KW_REF_MAX = 1.75 are these maxima rounded up to a multiple of 0.05 (the fp32 results of another CPU's vector
units may differ in last bits), K = 1.0 and KW = 7.0.  The two large "no A" values are rows of
ni = 2 with total ~ 1 (graze-sn3 row 10, ties-sn3 row 1): mid + cos dz / 2 cancels to 2e-3 from two terms of 0.35, its rounding (4e-8)
is multiplied by inv_s = 256 and by sigmoid' = 0.24, 2.5e-6 in one weight of the two -- the conditioning of the formula in fp32, which
u24 ni / total undercounts when ni is 2; A bounds exactly that operation, so K stays the constant of the remaining roundings."""
import functools

import pytest
import torch

import sampler_oracle as S
from oracle import stage1_oracle as O

IDS = [c.id for c in S.CASES]


@functools.lru_cache(maxsize=None)
def _evaluated(cid):
    """(case, inputs, float64 weights, fp32 weights, fp32 new depths, their judgement, the argument term of the bound)."""
    c = S.CASES[IDS.index(cid)]
    o, d, z, sdf, u = S.make_case(c)
    cap, use_var = 64.0 * 2 ** c.rnd, c.kind != 'cap'
    raw64 = S.weights64(o, d, z, sdf, S.inv_s64(c.var, cap, use_var, c.mode), c.mode)
    arg = S.arg_term64(o, d, z, sdf, S.inv_s64(c.var, cap, use_var, c.mode), c.mode)
    raw32 = S.weights(o, d, z, sdf, S.inv_s32(c.var, cap, use_var, c.mode), c.mode)
    zq32 = S.sample_pdf(z, raw32, u)
    return c, (o, d, z, sdf, u), raw64, raw32, zq32, S.cdf_residual(z, raw64, zq32, u), arg


@pytest.fixture
def float64_default():
    """Lets a test run the stage-1 oracle in float64 (its linspace / zeros follow the default dtype); the cases are made before."""
    for cid in IDS:
        _evaluated(cid)
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def test_case_table_covers_what_the_kernel_can_do_differently():
    up = [c for c in S.CASES if c.mode == 0]
    assert {(c.fam, c.sn) for c in up} == {(f, s) for f in S.FAMILIES for s in S.SN}
    for n in S.N_NEW:
        assert sum(c.n_new == n for c in up) >= 2
    for r in S.RS:
        assert sum(c.R == r for c in up) >= 2
    assert {c.kind for c in up} == {'cap', 'var', 'capwin'} and {c.ends for c in up} == {True, False}
    assert max(c.R for c in S.CASES) <= 400 and len(set(IDS)) == len(IDS)
    pr = [c for c in S.CASES if c.mode == 1]
    assert {c.var for c in pr} == {0.3, 0.7} and any(c.fam == 'probe' and c.sn == 16 for c in pr)


@pytest.mark.parametrize("cid", [c.id for c in S.CASES if c.mode == 0 and c.sn in (3, 64, 130)])
def test_mode0_is_the_stage1_oracle(cid, float64_default):
    c, (o, d, z, sdf, _), raw64, raw32, *_ = _evaluated(cid)
    cap, use_var = 64.0 * 2 ** c.rnd, c.kind != 'cap'
    n = max(c.n_new, 2)
    # float64: the oracle's upsample on float64 copies (its deterministic quantiles, formed in float64)
    u64 = torch.linspace(0.5 / n, 1.0 - 0.5 / n, steps=n)
    ref = O.upsample(o.double(), d.double(), z.double(), sdf.double(), n, torch.tensor(S.inv_s64(c.var, cap, use_var, 0)))
    got = S.sample_pdf(z.double(), raw64, u64)
    assert ref.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-12
    ref_w = O._excl_cumprod_weights(raw64 * 0 + 0.25)           # the transmittance product, on a constant alpha
    assert float((ref_w - 0.25 * (0.75 + 1e-7) ** torch.arange(c.sn - 1)).abs().max()) <= 1e-12
    assert float((O.sample_pdf(z.double(), raw64, n, u=u64.expand(c.R, n)) - got).abs().max()) <= 1e-12
    # fp32: the same bits as the oracle in fp32
    torch.set_default_dtype(torch.float32)
    ref32 = O.upsample(o, d, z, sdf, n, S.inv_s32(c.var, cap, use_var, 0))
    assert torch.equal(S.sample_pdf(z, raw32, torch.linspace(0.5 / n, 1.0 - 0.5 / n, steps=n)), ref32)


@pytest.mark.parametrize("cid", [c.id for c in S.CASES if c.mode == 1 and c.sn in (3, 16, 65, 256)])
def test_mode1_is_get_weights_of_the_stage1_oracle(cid, float64_default, monkeypatch):
    c, (o, d, z, sdf, _), raw64, raw32, *_ = _evaluated(cid)
    # a stub SDF: the network is not under test, get_weights receives the case's own SDF values whatever the points
    var32 = torch.tensor(c.var, dtype=torch.float32)
    monkeypatch.setattr(O, 'sdf_forward', lambda params, x, prefix='sdf_network': sdf.double().reshape(-1, 1))
    w, mid = O.get_weights({'deviation_network.variance': (var32 * 10.0).double() / 10.0}, z.double(), o.double(), d.double())
    assert w.dtype == torch.float64 and float((w - raw64).abs().max()) <= 1e-12
    torch.set_default_dtype(torch.float32)
    monkeypatch.setattr(O, 'sdf_forward', lambda params, x, prefix='sdf_network': sdf.reshape(-1, 1))
    w32, _ = O.get_weights({'deviation_network.variance': var32}, z, o, d)
    assert torch.equal(w32, raw32)


def test_depth_and_merge_forms():
    g = torch.Generator().manual_seed(3)
    R, nc, nbg = 7, 24, 8
    near, far = 0.5 + torch.rand(R, generator=g), 3.0 + torch.rand(R, generator=g)
    u1, u2 = torch.rand(R, generator=g), torch.rand(R, nbg, generator=g)
    lin_bg, lower, upper = S.bg_bins(nbg)
    # sample_ray of the stage-1 oracle up to its first SDF evaluation (renderer_zerothick.py:572-592)
    z = near[:, None] + (far - near)[:, None] * torch.linspace(0.0, 1.0, nc)[None, :] + (u1[:, None] - 0.5) * 2.0 / nc
    assert torch.equal(S.coarse_depths(near, far, torch.linspace(0.0, 1.0, nc), u1, nc), z)
    zo = torch.linspace(1e-3, 1.0 - 1.0 / (nbg + 1.0), nbg)
    mids = 0.5 * (zo[1:] + zo[:-1])
    zj = torch.cat([zo[:1], mids], -1)[None, :] + (torch.cat([mids, zo[-1:]], -1) - torch.cat([zo[:1], mids], -1))[None, :] * u2
    assert torch.equal(S.bg_depths(far, lower, upper, u2, nbg), far[:, None] / torch.flip(zj, dims=[-1]) + 1.0 / nbg)
    assert torch.equal(S.bg_depths(far, lin_bg, upper, None, nbg), far[:, None] / torch.flip(zo, dims=[-1])[None, :] + 1.0 / nbg)
    # the tie rule: old before new, new in their own order
    zs, ss = S.merge(torch.tensor([[1., 2., 2., 3.]]), torch.tensor([[10., 11., 12., 13.]]),
                     torch.tensor([[2., 2., 3.]]), torch.tensor([[20., 21., 22.]]))
    assert zs.tolist() == [[1., 2., 2., 2., 2., 3., 3.]] and ss.tolist() == [[10., 11., 12., 20., 21., 13., 22.]]


@pytest.mark.parametrize("cid", [c.id for c in S.CASES if c.mode == 0])
def test_input_conditions_hold_for_every_case(cid):
    """Mode 0 only: mode 1 has neither an `inside` test nor the -1e3 clip (its surf = cos < 0 is the sign of s1 - s0, exact)."""
    c, (o, d, z, sdf, _), *_ = _evaluated(cid)
    d_radius, d_clip = S.input_conditions(c, o, d, z, sdf)
    assert d_radius > 4e-6, d_radius
    assert d_clip > 1e-3, d_clip


@pytest.mark.parametrize("cid", IDS)
def test_fp32_cpu_oracle_stays_within_a_quarter_of_K(cid):
    c, (o, d, z, sdf, u), raw64, raw32, zq32, j, arg = _evaluated(cid)
    k = S.k_ref(z, j, arg)
    kw = float(((raw32.sum(-1).double() - S.wsum64(raw64)).abs() / ((c.sn - 1) * S.U24)).max()) if c.mode == 1 else 0.0
    print(f"{cid}: K_ref {k:.3f}  K_w {kw:.3f}  largest residual {float(j.res.max()):.2e}")
    assert k <= S.K / 4 and S.K == 4 * S.K_REF_MAX
    assert kw <= S.KW / 4 and S.KW == 4 * S.KW_REF_MAX
    assert bool((j.res <= S.bound(z, j, arg, S.K / 4)).all())


def test_the_measured_maxima_are_the_ones_K_was_set_from():
    ks = [S.k_ref(_evaluated(cid)[1][2], _evaluated(cid)[5], _evaluated(cid)[6]) for cid in IDS]
    # K comes from the measurement and does not sit far above it
    assert 0.5 * S.K_REF_MAX <= max(ks) <= S.K_REF_MAX, max(ks)


# --------------------------------------------------------------------------------------------------------------------------
# the bound can fail
# --------------------------------------------------------------------------------------------------------------------------
SANITY = [c.id for c in S.CASES if c.mode == 0 and c.fam in ('through', 'second') and c.sn in (64, 65, 66)]


@pytest.mark.parametrize("cid", SANITY)
def test_a_depth_moved_by_half_a_bin_breaks_the_bound(cid):
    c, (o, d, z, sdf, u), raw64, *_, arg = _evaluated(cid)
    zq = S.sample_pdf(z.double(), raw64, u).float()
    j = S.cdf_residual(z, raw64, zq, u)
    assert bool((j.res <= S.bound(z, j, arg)).all())                  # the float64 result, rounded to fp32, passes
    heavy = (j.cw >= 1e-3) & (j.zw > 0)
    assert bool(heavy.any())
    ir = torch.searchsorted(z.double().contiguous(), zq.double().contiguous(), right=True).clamp(1, c.sn - 1)
    upper_half = zq.double() - torch.gather(z.double(), -1, ir - 1) > 0.5 * j.zw          # move towards the far end: stay in the bin
    moved = torch.where(heavy, zq.double() + torch.where(upper_half, -0.5, 0.5) * j.zw, zq.double())
    jm = S.cdf_residual(z, raw64, moved, u)
    assert bool((jm.res > S.bound(z, jm, arg))[heavy].all())          # every moved sample is caught
    assert bool((jm.res <= S.bound(z, jm, arg))[~heavy].all())


@pytest.mark.parametrize("variant", ['inside_inverted', 'no_prev_min'])
@pytest.mark.parametrize("cid", [cid for cid in SANITY if S.CASES[IDS.index(cid)].R >= 5])
def test_a_round_with_a_wrong_rule_breaks_the_bound(cid, variant):
    """More than half of the rows of these cases hit the object (on a row that misses it both wrong rules change nothing)."""
    c, (o, d, z, sdf, u), raw64, *_, arg = _evaluated(cid)
    wrong = S.weights64(o, d, z, sdf, S.inv_s64(c.var, 64.0 * 2 ** c.rnd, c.kind != 'cap', 0), 0, variant=variant)
    zq = S.sample_pdf(z.double(), wrong, u).float()
    j = S.cdf_residual(z, raw64, zq, u)
    over = j.res > S.bound(z, j, arg)
    assert float(over.any(-1).float().mean()) > 0.5, float(over.any(-1).float().mean())
