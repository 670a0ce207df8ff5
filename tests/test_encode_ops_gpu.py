"""The stage-1 encoding kernels of csrc/encode.hip, one by one through the C ABI, against the float64 restatements of
tests/encode_oracle.py (anchored on recorded data by tests/test_encode_oracle_host.py).

Every output buffer starts filled with NaN and has one guard row past P: after the call the columns a kernel owns match the
reference, its pad columns are exactly 0.0, every other column -- and the guard row -- is still NaN.  Input columns a kernel must
not read (the pads of cotangent rows, the unused slots of the point records) hold NaN too.  P covers a lone wave, the 4-waves-per-
block boundary, a ragged last block and the grid-stride wrap past 8192 blocks; the float64 reference covers every row.

Tolerances (u = 2^-24, the unit roundoff of fp32; none is tuned to what a kernel returns):
  * sin / cos columns: 5e-6 absolute -- sinf / cosf at the argument the kernel holds, |argument| <= 2^9 (the figure of
    test_generic_embedding_matches_the_eager_formula).  Where the kernel computes the argument itself (x / |x| of the NeRF++ code,
    r and v^ of the shading rows) the raw columns it stores next to the sin / cos columns are held to float64 within their own
    rounding, and the sin / cos columns to float64 sin / cos OF THOSE STORED ARGUMENTS: an fp32 argument off by its rounding
    delta moves sin(2^k a) by 2^k delta, 3e-5 at k = 9, which is the conditioning of the formula in fp32 and no property of sinf.
  * IDE columns and their gradients: the conditioning-aware model of test_shade_encode_kernels_vs_float64 (same device functions):
    forward 2e-5 + 4e-7 sum_k |c_k| per term + 1e-4 |ref|; backward with cotangents on the terms with sum_k |c_k| < 300 only and
    err <= 2e-4 max |ref| + 1e-6.
  * linear maps of stored fp32 inputs (embed_jt, embed_j, embed_jt2, the column sums of nerf_embed_bwd): the reference is the same
    product in float64 of the fp32 values the kernel reads.  The kernel forms each term with 2 to 4 roundings (the sum of the two
    cotangent operands, two or three products, the difference of the first- and second-order parts), adds at most two terms per
    lane (the 84-column case takes two passes) and 64 lanes in a 6-level tree, and embed_jt2 may add the result to dx: at most
    4 + 1 + 6 + 1 = 12 roundings, each relative to a partial sum of magnitude <= mass = sum |term| (+ |dx before|).  So
    |err| <= 16 u mass, the mass from the float64 reference.
  * end-to-end gradients against float64 autograd from x: 2e-5 max |ref| (the figure of the generic-embedding test).
  * the last lines of nerf_embed_bwd and shade_encode_bwd: derived at the tests.

Worst err / bound measured on an MI355X over all cases (each check prints its own figure; run with -s): sdf_embed 0.014; embed_jt
0.19 stored-E, 0.007 end-to-end; embed_j 0.06 / 0.02; embed_jt2 0.26 / 0.013; nerf_embed 0.69 arguments, 0.014 sin / cos;
nerf_embed_bwd dx 0.12 stored, 0.23 end-to-end, ddir 0.16 / 0.02; ide 0.06, ide_bwd 0.004 ddirs, 0.03 dkappa; spec_encode 0.93 (a
degree-16 term of the sphere half); shade_encode_fwd IDE rows 0.11, r 0.23, v^ 0.61, SD 0.62, sin / cos 0.014; shade_encode_bwd dn
0.008, dMraw 0.01."""
import functools

import pytest
import torch
import torch.nn.functional as F

import encode_oracle as EO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PS = [1, 3, 4, 5, 257, 32773]
NAN = float('nan')
TOL72 = 2e-5 + 4e-7 * torch.cat([EO.IDE_KAPPA, EO.IDE_KAPPA])          # forward IDE model, per column of a 72-d row
WELL72 = (torch.cat([EO.IDE_KAPPA, EO.IDE_KAPPA]) < 300.0).double()     # cotangent mask of the backward IDE model


@pytest.fixture(scope="module")
def K(gpu):
    """The library and the few conveniences every case uses."""
    from nu_nerf_amd import _lib as L

    class Ctx:
        lib = L.load()
        err = L.NuNerfLibraryError
        live = []                          # device copies made by dev(): kept until the call that reads them has finished

        @staticmethod
        def ptr(t, col=0):
            """Device address of column `col` of the first row of t (None -> NULL)."""
            return L.ptr(None) if t is None else L.c_p(t.data_ptr() + 4 * col)

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


def host(t):
    return t.detach().cpu().double()


def within(tag, got, ref, bound):
    """got (device fp32) is finite and |got - ref| <= bound everywhere; prints the worst err / bound for the record."""
    got = host(got)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    err = (got - ref.detach()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    print(f"ENCODE-OPS {tag}: worst err/bound {float(ratio.max()):.3g} (err {float(err.max()):.3g})")
    assert bool((err <= bound).all()), f"{tag}: err/bound {float(ratio.max()):.4g}, max err {float(err.max()):.4g}"


def all_nan(t):
    return t.numel() == 0 or bool(torch.isnan(t).all())


def all_zero(t):
    return t.numel() == 0 or float(t.abs().max()) == 0.0        # NaN fails this


def mixed(shape, cols, rnd):
    """An all-NaN [rows, ld] cotangent / operand buffer whose columns `cols` (a slice) hold rnd."""
    t = torch.full(shape, NAN)
    t[:, cols] = rnd
    return t


@functools.lru_cache(maxsize=None)
def inputs(P):
    """Seeded fp32 inputs on the CPU: points with |x| from 0.2 to 1.2 (both sides of the 0.999 sphere-point branch), NeRF++ points
    with |x| from 1 to 8, normals scaled by 1.7 and ray directions by 0.6 (the kernels normalise them), the material logits, the
    8-float point records [x, unused, d, unused] (the unused slots hold NaN)."""
    g = torch.Generator().manual_seed(1000 + P)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = F.normalize(rn(P, 3), dim=-1) * (0.2 + 1.0 * torch.rand(P, 1, generator=g))
    xo = F.normalize(rn(P, 3), dim=-1) * (1.0 + 7.0 * torch.rand(P, 1, generator=g))
    n, d, mraw = 1.7 * rn(P, 3), 0.6 * rn(P, 3), rn(P, 8)
    hole = torch.full((P, 1), NAN)
    return {'x': x, 'xo': xo, 'n': n, 'd': d, 'mraw': mraw, 'pt': torch.cat([x, hole, d, hole], -1), 'pto': torch.cat([xo, hole, d, hole], -1),
            'dirs': F.normalize(rn(P, 3), dim=-1), 'kinv': torch.rand(P, generator=g), 'E': rn(P, 64)}


def rand(P, *shape, seed=0):
    return torch.randn(P, *shape, generator=torch.Generator().manual_seed(77 * P + seed))


def onehot(c, dim):
    return F.one_hot(c, dim).double()


# ------------------------------------------------------------------------------------------------------------------ SDF embedding
def sdf_embed(K, P, pt, pt_ld, aux=True):
    E, U4, YX = K.nan(P + 1, 64), K.nan(P + 1, 256) if aux else None, K.nan(P + 1, 288) if aux else None
    K.call('nu_sdf_embed', K.ptr(pt), pt_ld, P, K.ptr(E), K.ptr(U4), K.ptr(YX))
    return E, U4, YX


@pytest.mark.parametrize("pt_ld,aux", [(8, True), (3, True), (8, False)])
@pytest.mark.parametrize("P", PS)
def test_sdf_embed(K, P, pt_ld, aux):
    I = inputs(P)
    ref = EO.embed64(I['x'].double(), 6)
    E, U4, YX = sdf_embed(K, P, K.dev(I['pt'] if pt_ld == 8 else I['x']), pt_ld, aux)
    assert torch.equal(E[:P, :3].cpu(), I['x'])                                       # the raw columns are copies
    within(f"sdf_embed E P={P} ld={pt_ld}", E[:P, :39], ref, 5e-6)
    assert all_zero(E[:P, 39:]) and all_nan(E[P:])
    if aux:
        assert torch.equal(U4[:P, 217:], E[:P, :39]) and all_nan(U4[:P, :217]) and all_nan(U4[P:])
        assert torch.equal(YX[:P, 257:260].cpu(), I['x']) and all_zero(YX[:P, 260:]) and all_nan(YX[:P, :257]) and all_nan(YX[P:])


def jt_reference(E, g, gb=None, nbar=None):
    """Float64 J^T g (+ the second-order part -f^2 emb gb nbar_c) from the STORED embedding E [P, 39]: (sums [P, 3], masses)."""
    c, f, partner, sign = EO.embed_columns(3, 6)
    J = torch.where(partner < 0, torch.ones_like(E), f * sign * E[:, partner.clamp_min(0)])
    term, mass = g * J, (g * J).abs()
    if nbar is not None:
        t2 = -gb * nbar[:, c] * f * f * E * (partner >= 0)
        term, mass = term + t2, mass + t2.abs()
    return term @ onehot(c, 3), mass @ onehot(c, 3)


@pytest.mark.parametrize("with_gs", [False, True])
@pytest.mark.parametrize("P", PS)
def test_embed_jt(K, P, with_gs):
    I = inputs(P)
    G0, Gs = mixed((P, 64), slice(0, 39), rand(P, 39, seed=1)), mixed((P, 256), slice(217, 256), rand(P, 39, seed=2))
    g = G0[:, :39].double() + (Gs[:, 217:].double() if with_gs else 0.0)
    x = I['x'].double().requires_grad_(True)
    (n_auto,) = torch.autograd.grad((EO.embed64(x, 6) * g).sum(), x)
    E, _, _ = sdf_embed(K, P, K.dev(I['pt']), 8, aux=False)
    n = K.nan(P + 1, 3)
    dGs = K.dev(Gs) if with_gs else None
    K.call('nu_embed_jt', K.ptr(E), K.ptr(K.dev(G0)), 64, K.ptr(dGs, 217), 256, P, K.ptr(n))
    ref, mass = jt_reference(host(E[:P, :39]), g)
    within(f"embed_jt stored-E P={P} gs={with_gs}", n[:P], ref, 16 * U * mass)
    within(f"embed_jt end-to-end P={P} gs={with_gs}", n[:P], n_auto, 2e-5 * float(n_auto.abs().max()))
    assert all_nan(n[P:])


@pytest.mark.parametrize("P", PS)
def test_embed_j(K, P):
    I = inputs(P)
    nbar = rand(P, 3, seed=3)
    c, f, partner, sign = EO.embed_columns(3, 6)
    x = I['x'].double()
    e = EO.embed64(x, 6)
    q_x = torch.where(partner < 0, torch.ones_like(e), f * sign * e[:, partner.clamp_min(0)]) * nbar.double()[:, c]      # J(x) nbar
    E, _, _ = sdf_embed(K, P, K.dev(I['pt']), 8, aux=False)
    Q0, Q4 = K.nan(P + 1, 64), K.nan(P + 1, 256)
    K.call('nu_embed_j', K.ptr(E), K.ptr(K.dev(nbar)), P, K.ptr(Q0), K.ptr(Q4))
    Es = host(E[:P, :39])
    q_s = torch.where(partner < 0, torch.ones_like(Es), f * sign * Es[:, partner.clamp_min(0)]) * nbar.double()[:, c]
    within(f"embed_j stored-E P={P}", Q0[:P, :39], q_s, 16 * U * q_s.abs())             # one term per column: two roundings
    # from x: the stored sin / cos carry <= 5e-6 (test_sdf_embed), scaled by f |nbar_c|
    within(f"embed_j from-x P={P}", Q0[:P, :39], q_x, 16 * U * q_x.abs() + 5e-6 * f * nbar.double()[:, c].abs())
    assert all_zero(Q0[:P, 39:]) and all_nan(Q0[P:])
    assert torch.equal(Q4[:P, 217:], Q0[:P, :39]) and all_nan(Q4[:P, :217]) and all_nan(Q4[P:])


@pytest.mark.parametrize("P", PS)
def test_embed_jt2(K, P):
    I = inputs(P)
    dE, dS = mixed((P, 64), slice(0, 39), rand(P, 39, seed=4)), mixed((P, 256), slice(217, 256), rand(P, 39, seed=5))
    G0, Gs = mixed((P, 64), slice(0, 39), rand(P, 39, seed=6)), mixed((P, 256), slice(217, 256), rand(P, 39, seed=7))
    nbar, before = rand(P, 3, seed=8), rand(P, 3, seed=9)
    E, _, _ = sdf_embed(K, P, K.dev(I['pt']), 8, aux=False)
    Es = host(E[:P, :39])
    dev = {k: K.dev(v) for k, v in (('dE', dE), ('dS', dS), ('G0', G0), ('Gs', Gs), ('nbar', nbar))}
    for with_ds in (False, True):
        for with_nbar in (False, True):
            g = dE[:, :39].double() + (dS[:, 217:].double() if with_ds else 0.0)
            gb = G0[:, :39].double() + Gs[:, 217:].double()
            x = I['x'].double().requires_grad_(True)
            loss = (EO.embed64(x, 6) * g).sum()
            if with_nbar:
                (jt,) = torch.autograd.grad((EO.embed64(x, 6) * gb).sum(), x, create_graph=True)
                loss = loss + (jt * nbar.double()).sum()
            (auto,) = torch.autograd.grad(loss, x)
            ref, mass = jt_reference(Es, g, gb, nbar.double()) if with_nbar else jt_reference(Es, g)
            for accumulate in (0, 1):
                tag = f"P={P} dS={with_ds} nbar={with_nbar} acc={accumulate}"
                dx = K.nan(P + 1, 3)
                if accumulate:
                    dx[:P] = K.dev(before)
                K.call('nu_embed_jt2', K.ptr(E), K.ptr(dev['dE']), 64, K.ptr(dev['dS'] if with_ds else None, 217), 256,
                       K.ptr(dev['G0'] if with_nbar else None), 64, K.ptr(dev['Gs'] if with_nbar else None, 217), 256,
                       K.ptr(dev['nbar'] if with_nbar else None), P, K.ptr(dx), accumulate)
                b = before.double() * accumulate
                within(f"embed_jt2 stored-E {tag}", dx[:P], ref + b, 16 * U * (mass + b.abs()))
                within(f"embed_jt2 end-to-end {tag}", dx[:P], auto + b, 2e-5 * float((auto + b).abs().max()))
                assert all_nan(dx[P:])


# ------------------------------------------------------------------------------------------------------------------ NeRF++ inputs
def nerf_embed(K, P, pt):
    E4, U5, V = K.nan(P + 1, 96), K.nan(P + 1, 352), K.nan(P + 1, 288)
    K.call('nu_nerf_embed', K.ptr(pt), 8, P, K.ptr(E4), K.ptr(U5), K.ptr(V))
    return E4, U5, V


@pytest.mark.parametrize("P", PS)
def test_nerf_embed(K, P):
    I = inputs(P)
    x4 = torch.cat(EO.nerf_inputs64(I['xo'].double()), -1)
    v_ref = EO.embed64(-I['d'].double(), 4)
    E4, U5, V = nerf_embed(K, P, K.dev(I['pto']))
    # (x / |x|, 1 / |x|) in fp32: sum of squares 3 u, square root 1.5 u + u, quotient + u: 3.5 u relative
    within(f"nerf_embed x4 P={P}", E4[:P, :4], x4, 4 * U * x4.abs())
    # sin / cos of the arguments the kernel holds (module docstring)
    within(f"nerf_embed E4 P={P}", E4[:P, :84], EO.embed64(host(E4[:P, :4]), 10), 5e-6)
    assert all_zero(E4[:P, 84:]) and all_nan(E4[P:])
    assert torch.equal(U5[:P, 256:], E4[:P]) and all_nan(U5[:P, :256]) and all_nan(U5[P:])
    assert torch.equal(V[:P, 256:259].cpu(), -I['d'])
    within(f"nerf_embed V P={P}", V[:P, 256:283], v_ref, 5e-6)
    assert all_zero(V[:P, 283:]) and all_nan(V[:P, :256]) and all_nan(V[P:])


@pytest.mark.parametrize("with_gs", [False, True])
@pytest.mark.parametrize("P", PS)
def test_nerf_embed_bwd(K, P, with_gs):
    """dx = Jn(x)^T g4 with g4 [P, 4] the column sums over the 84-column code of (x / |x|, 1 / |x|), ddir = -(column sums of the view code).
    Two references: (a) the float64 sums of the STORED codes E4 / V, pushed through float64 autograd of nerf_inputs64 -- bound by
    rounding alone; (b) float64 autograd from x and d through nerf_inputs64 and embed64 -- bound (a) plus the propagated
    forward bounds of the stored codes (test_nerf_embed: 5e-6 per sin / cos, 4 u per argument, an argument error delta moves
    sin(f a) by f delta).
    Rounding of the last line, dx_c = (g4_c - xh_c (xh . g4)) / |x| - g4_3 xh_c / |x|^2: the sums arrive with <= 11 u mass_c (3 per
    term, 2 per-lane adds, 6 tree levels); |x| carries 2.5 u, xh 3.5 u, the dot product 3.5 + 1 + 2, its product with xh 3.5 + 1, the
    difference 1, the quotient 1 + 2.5 -- 27 u along the longest chain of the first part, 11 + 4.5 + 6 + 1 + 1 < 27 u of the second --
    each relative to a magnitude that the absolute Jacobian applied to the masses bounds:
      A_c = (mass_c + |xh_c| sum_j |xh_j| mass_j) / |x| + mass_3 |xh_c| / |x|^2,     |err dx_c| <= 32 u A_c."""
    I = inputs(P)
    gE = mixed((P, 96), slice(0, 84), rand(P, 84, seed=10))
    gS = mixed((P, 352), slice(256, 340), rand(P, 84, seed=11))
    gV = mixed((P, 288), slice(256, 283), rand(P, 27, seed=12))
    g, gv = gE[:, :84].double() + (gS[:, 256:340].double() if with_gs else 0.0), gV[:, 256:283].double()
    x, d = I['xo'].double().requires_grad_(True), I['d'].double().requires_grad_(True)
    loss = (EO.embed64(torch.cat(EO.nerf_inputs64(x), -1), 10) * g).sum() + (EO.embed64(-d, 4) * gv).sum()
    dx_auto, dd_auto = torch.autograd.grad(loss, (x, d))
    E4, U5, V = nerf_embed(K, P, K.dev(I['pto']))
    dx, ddir = K.nan(P + 1, 3), K.nan(P + 1, 3)
    K.call('nu_nerf_embed_bwd', K.ptr(K.dev(I['pto'])), 8, K.ptr(E4), K.ptr(V), K.ptr(K.dev(gE)), 96,
           K.ptr(K.dev(gS) if with_gs else None, 256), 352, K.ptr(K.dev(gV), 256), 288, P, K.ptr(dx), K.ptr(ddir))
    assert all_nan(dx[P:]) and all_nan(ddir[P:])

    def sums(Es, gg, dim, n_freq):
        c, f, partner, sign = EO.embed_columns(dim, n_freq)
        t = gg * torch.where(partner < 0, torch.ones_like(Es), f * sign * Es[:, partner.clamp_min(0)])
        cond = (gg.abs() * f * (partner >= 0)) @ onehot(c, dim), (gg.abs() * f * f * (partner >= 0)) @ onehot(c, dim)
        return t @ onehot(c, dim), t.abs() @ onehot(c, dim), cond
    # ---- view code: d is an input, its code carries the sin / cos bound only
    v_ref, v_mass, (v_c1, _) = sums(host(V[:P, 256:283]), gv, 3, 4)
    within(f"nerf_embed_bwd ddir stored-V P={P}", ddir[:P], -v_ref, 16 * U * v_mass)
    within(f"nerf_embed_bwd ddir end-to-end P={P}", ddir[:P], dd_auto, 16 * U * v_mass + 5e-6 * v_c1)
    # ---- point code
    g4, m4, (c1, c2) = sums(host(E4[:P, :84]), g, 4, 10)
    xs = I['xo'].double().requires_grad_(True)
    x4 = torch.cat(EO.nerf_inputs64(xs), -1)
    (dx_ref,) = torch.autograd.grad((x4 * g4).sum(), xs)
    xh, inn = x4.detach()[:, :3], x4.detach()[:, 3:]

    def jabs(v):      # the absolute Jacobian of (x / |x|, 1 / |x|), transposed, applied to non-negative v [P, 4]
        return (v[:, :3] + xh.abs() * (xh.abs() * v[:, :3]).sum(-1, keepdim=True)) * inn + v[:, 3:] * xh.abs() * inn * inn
    within(f"nerf_embed_bwd dx stored-E4 P={P} gs={with_gs}", dx[:P], dx_ref, 32 * U * jabs(m4))
    cond = 5e-6 * c1 + 4 * U * x4.detach().abs() * c2
    within(f"nerf_embed_bwd dx end-to-end P={P} gs={with_gs}", dx[:P], dx_auto, 32 * U * jabs(m4) + jabs(cond))


# ------------------------------------------------------------------------------------------------------------------ IDE
def ide_tol(ref):
    return TOL72 + 1e-4 * ref.detach().abs()


@pytest.mark.parametrize("ldo,with_kappa", [(72, True), (96, True), (160, True), (96, False)])
@pytest.mark.parametrize("P", PS)
def test_ide_and_ide_bwd(K, P, ldo, with_kappa):
    I = inputs(P)
    d = I['dirs'].double().requires_grad_(True)
    k = (I['kinv'].double()[:, None] if with_kappa else torch.zeros(P, 1, dtype=torch.float64)).requires_grad_(True)
    ref = EO.ide64(d, k)
    cot = rand(P, 72, seed=13) * WELL72.float()
    dd_ref, dk_ref = torch.autograd.grad((ref * cot.double()).sum(), (d, k))
    dirs, kinv = K.dev(I['dirs']), K.dev(I['kinv']) if with_kappa else None
    out = K.nan(P + 1, ldo)
    K.call('nu_ide', K.ptr(dirs), K.ptr(kinv), P, K.ptr(out), ldo)
    within(f"ide P={P} ldo={ldo} kappa={with_kappa}", out[:P, :72], ref, ide_tol(ref))
    assert all_zero(out[:P, 72:]) and all_nan(out[P:])
    ddirs, dk = K.nan(P + 1, 3), K.nan(P + 1) if with_kappa else None
    K.call('nu_ide_bwd', K.ptr(dirs), K.ptr(kinv), K.ptr(K.dev(mixed((P, ldo), slice(0, 72), cot))), ldo, P, K.ptr(ddirs), K.ptr(dk))
    within(f"ide_bwd ddirs P={P} ldo={ldo} kappa={with_kappa}", ddirs[:P], dd_ref, 2e-4 * float(dd_ref.abs().max()) + 1e-6)
    assert all_nan(ddirs[P:])
    if with_kappa:
        within(f"ide_bwd dkappa P={P} ldo={ldo}", dk[:P], dk_ref[:, 0], 2e-4 * float(dk_ref.abs().max()) + 1e-6)
        assert all_nan(dk[P:])


def test_ide_rejects_a_row_shorter_than_the_encoding(K):
    I = inputs(5)
    out = K.nan(6, 71)
    with pytest.raises(K.err, match="code -1"):            # NU_ERR_ARG
        K.call('nu_ide', K.ptr(K.dev(I['dirs'])), K.ptr(K.dev(I['kinv'])), 5, K.ptr(out), 71)
    torch.cuda.synchronize()
    assert all_nan(out)


@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("P", PS)
def test_spec_encode(K, P, sphere):
    I = inputs(P)
    d, x, zero = I['dirs'].double(), I['x'].double(), torch.zeros(P, 1, dtype=torch.float64)
    ref = EO.ide64(d, zero)
    if sphere:
        ref = torch.cat([ref, EO.ide64(EO.sphere_point64(x, d), zero)], -1)
    ldo = 160 if sphere else 96
    out = K.nan(P + 1, ldo)
    K.call('nu_spec_encode', K.ptr(K.dev(I['dirs'])), K.ptr(K.dev(I['x']) if sphere else None), P, sphere, K.ptr(out), ldo)
    within(f"spec_encode P={P} sphere={sphere}", out[:P, :ref.shape[1]], ref,
           torch.cat([ide_tol(ref[:, s:s + 72]) for s in range(0, ref.shape[1], 72)], -1))
    assert all_zero(out[:P, ref.shape[1]:]) and all_nan(out[P:])


def test_spec_encode_rejects_short_rows_and_a_missing_point(K):
    I = inputs(5)
    d, x = K.dev(I['dirs']), K.dev(I['x'])
    for xx, ldo in ((x, 143), (None, 160)):
        out = K.nan(6, 160)
        with pytest.raises(K.err, match="code -1"):        # NU_ERR_ARG
            K.call('nu_spec_encode', K.ptr(d), K.ptr(xx), 5, 1, K.ptr(out), ldo)
        torch.cuda.synchronize()
        assert all_nan(out)


# ------------------------------------------------------------------------------------------------------------------ shading rows
def shade_fwd(K, P, I, sphere, rdim):
    ld_ol, ld_rl = 160 if sphere else 96, max(32, -(-2 * rdim // 32) * 32)            # the engine's row lengths
    B = {'OLin': K.nan(3 * P + 1, ld_ol), 'ILin': K.nan(2 * P + 1, 128), 'IWin': K.nan(P + 1, 96), 'RLin': K.nan(P + 1, ld_rl),
         'SD': K.nan(P + 1, 8)}
    K.call('nu_shade_encode_fwd', K.ptr(K.dev(I['n'])), K.ptr(K.dev(I['pt'])), 8, K.ptr(K.dev(I['E'])), K.ptr(K.dev(I['mraw'])), 8, P,
           sphere, ld_ol, rdim, ld_rl, K.ptr(B['OLin']), K.ptr(B['ILin']), K.ptr(B['IWin']), K.ptr(B['RLin']), K.ptr(B['SD']))
    return B, ld_ol, ld_rl


@pytest.mark.parametrize("rdim", [39, 15])
@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("P", PS)
def test_shade_encode_fwd(K, P, sphere, rdim):
    """Rounding of the directions in fp32 (u each operation): |n| carries 3 u / 2 + u, its reciprocal + u, n^ and v^ 4.5 u relative;
    NoV sums three products of 10 u each in two additions: 12 u absolute; r = 2 NoV n^ - v^: (12 + 5.5 |NoV|) 2 |n^_c| + 4.5 + 1
    <= 41 u absolute; rho = 1 / (1 + exp(-m)): expf 2 u, sum, quotient: 4 u relative."""
    I = inputs(P)
    E = I['E'].double()[:, :39]
    dirs = EO.shade_dirs64(I['n'].double(), I['d'].double())
    rho = torch.sigmoid(I['mraw'].double()[:, 1:2])
    rows = EO.shade_rows64(E, I['x'].double(), *dirs, rho, sphere, rdim)
    B, ld_ol, ld_rl = shade_fwd(K, P, I, sphere, rdim)
    tag = f"P={P} sphere={sphere} rdim={rdim}"
    w = rows['OLin'].shape[1]
    for blk, name in enumerate(("IDE(n,1)", "IDE(r,rho)", "IDE(r,0)")):               # rows p, P + p, 2P + p
        ref = rows['OLin'][blk * P:(blk + 1) * P]
        within(f"shade_fwd OLin {name} {tag}", B['OLin'][blk * P:(blk + 1) * P, :w], ref,
               torch.cat([ide_tol(ref[:, s:s + 72]) for s in range(0, w, 72)], -1))
    assert all_zero(B['OLin'][:3 * P, w:]) and all_nan(B['OLin'][3 * P:])
    Ed = K.dev(I['E'])
    for blk in range(2):
        got, ref = B['ILin'][blk * P:(blk + 1) * P], rows['ILin'][blk * P:(blk + 1) * P]
        assert torch.equal(got[:, :39], Ed[:, :39])
        within(f"shade_fwd ILin block {blk} {tag}", got[:, 39:111], ref[:, 39:], ide_tol(ref[:, 39:]))
    assert all_zero(B['ILin'][:2 * P, 111:]) and all_nan(B['ILin'][2 * P:])
    # IWin = [E, r, sin / cos of the r the kernel holds]
    assert torch.equal(B['IWin'][:P, :39], Ed[:, :39])
    within(f"shade_fwd IWin r {tag}", B['IWin'][:P, 39:42], rows['IWin'][:, 39:42], 41 * U)
    within(f"shade_fwd IWin embed(r) {tag}", B['IWin'][:P, 39:78], EO.embed64(host(B['IWin'][:P, 39:42]), 6), 5e-6)
    assert all_zero(B['IWin'][:P, 78:]) and all_nan(B['IWin'][P:])
    # RLin = [E prefix, v^, sin / cos of the v^ the kernel holds] (the first rdim columns of the 6-frequency code)
    assert torch.equal(B['RLin'][:P, :rdim], Ed[:, :rdim])
    within(f"shade_fwd RLin v {tag}", B['RLin'][:P, rdim:rdim + 3], rows['RLin'][:, rdim:rdim + 3], 4.5 * U * rows['RLin'][:, rdim:rdim + 3].abs())
    within(f"shade_fwd RLin embed(v) {tag}", B['RLin'][:P, rdim:2 * rdim], EO.embed64(host(B['RLin'][:P, rdim:rdim + 3]), 6)[:, :rdim], 5e-6)
    assert all_zero(B['RLin'][:P, 2 * rdim:]) and all_nan(B['RLin'][P:])
    sd = rows['SD']
    within(f"shade_fwd SD {tag}", B['SD'][:P], sd,
           torch.cat([4.5 * U * sd[:, :3].abs(), torch.full((P, 1), 12 * U, dtype=torch.float64), 3.5 * U * sd[:, 4:5], 4 * U * sd[:, 5:6],
                      torch.zeros(P, 2, dtype=torch.float64)], -1))
    assert all_nan(B['SD'][P:])


def test_shade_encode_fwd_rejects_short_rows(K):
    I = inputs(5)
    for sphere, ld_ol, rdim, ld_rl in ((1, 143, 39, 96), (0, 71, 39, 96), (0, 96, 39, 77), (0, 96, 45, 96)):
        B = [K.nan(16, 160), K.nan(11, 128), K.nan(6, 96), K.nan(6, 96), K.nan(6, 8)]
        with pytest.raises(K.err, match="code -1"):        # NU_ERR_ARG
            K.call('nu_shade_encode_fwd', K.ptr(K.dev(I['n'])), K.ptr(K.dev(I['pt'])), 8, K.ptr(K.dev(I['E'])), K.ptr(K.dev(I['mraw'])), 8,
                   5, sphere, ld_ol, rdim, ld_rl, *[K.ptr(b) for b in B])
        torch.cuda.synchronize()
        assert all(all_nan(b) for b in B)


@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("P", PS)
def test_shade_encode_bwd(K, P, sphere):
    """dn (w.r.t. the RAW normal) and dMraw[:, 1] += d rho rho (1 - rho) against float64 autograd of
    <OLin, dOLin> + <ILin[:, 39:111], dILin[:, 39:111]> + <NoV, dNoV>.
    Bound: the IDE gradient model gives the three wave-reduced partials -- G_n w.r.t. n^ (IDE(n^, 1) and its sphere point), G_r
    w.r.t. r, G_rho w.r.t. rho, each available from float64 autograd with n^, r, rho as leaves -- to eps_* = 2e-4 max |G_*| + 1e-6.
    The last lines are  t = G_n + 2 NoV G_r + (dNoV + 2 G_r . n^) v^,  dn = (t - n^ (n^ . t)) / |n|:
      |err t_c| <= eps_n + eps_r (2 |NoV| + 2 |v^_c| sum_j |n^_j|) + 48 u T_c,
      T_c = |G_n,c| + 2 |NoV| |G_r,c| + (|dNoV| + 2 sum_j |G_r,j n^_j|) |v^_c|   (the mass of the line; the directions carry <= 12 u
      (test_shade_encode_fwd), each of the <= 6 operations of a chain one more, the projection and 1 / |n| <= 12 more: < 48 u),
      |err dn_c| <= (|err t_c| + |n^_c| sum_j |n^_j| |err t_j|) / |n|        (the absolute Jacobian of n / |n|)
    and dMraw[:, 1] = before + G_rho rho (1 - rho): eps_rho rho (1 - rho) + 8 u (|before| + |G_rho| rho (1 - rho))."""
    I = inputs(P)
    ld_ol = 160 if sphere else 96
    w = 144 if sphere else 72
    cOL = mixed((3 * P, ld_ol), slice(0, w), torch.randn(3 * P, w, generator=torch.Generator().manual_seed(5 * P + 1)) * torch.cat([WELL72] * (w // 72)).float())
    cIL = mixed((2 * P, 128), slice(39, 111), torch.randn(2 * P, 72, generator=torch.Generator().manual_seed(5 * P + 2)) * WELL72.float())
    cNoV, before = rand(P, seed=14), rand(P, 8, seed=15)
    E, x, d = I['E'].double()[:, :39], I['x'].double(), I['d'].double()

    def loss_of(nh, vh, nov, r, inorm, rho, with_nov=True):
        rows = EO.shade_rows64(E, x, nh, vh, nov, r, inorm, rho, sphere, 39)
        out = (rows['OLin'] * cOL[:, :w].double()).sum() + (rows['ILin'][:, 39:] * cIL[:, 39:111].double()).sum()
        return out + (nov[:, 0] * cNoV.double()).sum() if with_nov else out
    n, m1 = I['n'].double().requires_grad_(True), I['mraw'].double()[:, 1:2].clone().requires_grad_(True)
    dn_ref, dm_ref = torch.autograd.grad(loss_of(*EO.shade_dirs64(n, d), torch.sigmoid(m1)), (n, m1))
    nh, vh, nov, r, inorm = (t.detach() for t in EO.shade_dirs64(n, d))
    rho = torch.sigmoid(m1).detach()
    leaves = [t.clone().requires_grad_(True) for t in (nh, r, rho)]
    G_n, G_r, G_rho = torch.autograd.grad(loss_of(leaves[0], vh, nov, leaves[1], inorm, leaves[2], with_nov=False), leaves)
    eps_n, eps_r, eps_rho = (2e-4 * float(G.abs().max()) + 1e-6 for G in (G_n, G_r, G_rho))
    T = G_n.abs() + 2 * nov.abs() * G_r.abs() + (cNoV.double().abs()[:, None] + 2 * (G_r * nh).abs().sum(-1, keepdim=True)) * vh.abs()
    et = eps_n + eps_r * (2 * nov.abs() + 2 * vh.abs() * nh.abs().sum(-1, keepdim=True)) + 48 * U * T
    bound_dn = (et + nh.abs() * (nh.abs() * et).sum(-1, keepdim=True)) * inorm
    dsig = rho * (1 - rho)
    bound_dm = eps_rho * dsig + 8 * U * (before.double()[:, 1:2].abs() + G_rho.abs() * dsig)

    B, _, _ = shade_fwd(K, P, I, sphere, 39)
    dn, dM = K.nan(P + 1, 3), K.nan(P + 1, 8)
    dM[:P] = K.dev(before)
    K.call('nu_shade_encode_bwd', K.ptr(K.dev(I['n'])), K.ptr(K.dev(I['pt'])), 8, K.ptr(B['SD']), K.ptr(K.dev(cOL)), ld_ol, sphere,
           K.ptr(K.dev(cIL)), K.ptr(K.dev(cNoV)), P, K.ptr(dn), K.ptr(dM), 8)
    within(f"shade_bwd dn P={P} sphere={sphere}", dn[:P], dn_ref, bound_dn)
    within(f"shade_bwd dMraw[:,1] P={P} sphere={sphere}", dM[:P, 1:2], before.double()[:, 1:2] + dm_ref, bound_dm)
    keep = [0, 2, 3, 4, 5, 6, 7]
    assert torch.equal(dM[:P, keep].cpu(), before[:, keep])                           # bit-identical: the kernel owns column 1 only
    assert all_nan(dn[P:]) and all_nan(dM[P:])
