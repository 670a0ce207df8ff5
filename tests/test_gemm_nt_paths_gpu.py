"""Every epilogue path and both tile heights of the exact-fp32 NT GEMM (csrc/gemm_nt.hip: gemm_nt2_kernel / gemm_nt2b_kernel, the
epilogue of csrc/gemm_epi.h) against ONE float64 statement of the NuGemmNT contract of include/nu_nerf.h, through the C ABI.

What every test here does
  * the expected values come from `_expect`: v = alpha A W^T in float64, the nine epilogues, act_cols (columns >= act_cols of a
    derivative epilogue are plain v, C2 is 0 there), zero_to (columns [N, zero_to) are 0), groups with their own strides;
  * C, C2 and the sign-bit words sit in allocations with guard rows in front of row 0 and behind row M - 1 and guard columns behind
    max(N, zero_to), pre-filled with NaN (the words: with a fixed bit pattern); the guards must come back untouched, so a store past
    the last row or column of a ragged tile is seen even where it would land inside a neighbour's memory;
  * whatever the contract says is not read is NaN: the pad columns of A, W, H, D and Cadd, H where sign-bit words replace it, and
    H / D / Cadd in the columns >= act_cols -- and every output must come back finite and right;
  * nu_gemm_nt_tile_rows must name the tile height the test is about (64: gemm_nt2_kernel<E, 1>, 128: <E, 2>), so a change of
    the dispatch rule cannot move a test off its kernel unnoticed.

The bound is relative to the MASS of an output element, mass = |alpha| (|A| |W|^T) |d out / d v| + |bias| + |Cadd|:
  |out - float64| <= (4e-7 max(1, sqrt(K) / 4) + 4 R[epilogue]) mass.
The first term is the accumulation bound of test_gemm_gpu.py::test_bf16x6_nt_is_fp32_equivalent.  R is the distance of the epilogue
formula itself, evaluated in plain torch fp32 from the fp32-rounded float64 v, to float64: the largest mass-relative distance over
all inputs of this file (`restatement_distance`; measured on the MI355X with torch's own fp32 exp / log1p, NOT with the kernel).
The factor 4 is for the hardware exp2 / log2 of the kernel (about 1 ulp each where libm is correctly rounded to half an ulp) and the
rounding of the argument scaling 100 log2(e).  Measured R (MEASURED_R below) and the constant 4 R it adds to 5.7e-7 (K = 32):
  epilogues 0, 1, 2, 3, 7, 8   R = 1.04e-7, 9.69e-8, 9.69e-8, 5.38e-8, 5.45e-8, 9.0e-8 (one rounding of v)   4 R <= 4.2e-7
  MUL_DSP, Q_SP (C)            R = 6.28e-4                                                                  4 R = 2.5e-3
  B_SP                         R = 1.16e-5 (|Cadd| is part of its mass)                                    4 R = 4.6e-5
  Q_SP (C2)                    R = 2.98e-7                                                                  4 R = 1.2e-6
The large R of the softplus-derivative family is one element in millions: sp' = 1 - exp(-100 h) is a difference of two numbers near
1 where h is small (five standard deviations down, among 16 million real softplus outputs), its absolute error stays one ulp of 1,
and the mass carries the factor sp'.  A maximum over such a tail says little about ordinary elements, so a second bound holds beside the
first, with the activation term relative to the WHOLE mass, wmass = |alpha| |A| |W|^T + |bias| + |Cadd| (no |d out / d v|):
  |out - float64| <= 4e-7 max(1, sqrt(K) / 4) mass + 4 R' wmass,
R' measured as R is, relative to wmass: 1.05e-7 (MUL_DSP, Q_SP), 1.34e-7 (B_SP), as R for the others.  An element must meet both.
On the MI355X the kernel's largest error is 0.72 of the smaller of the two bounds (Q_SP, 40000 x 128), 0.2 to 0.5 elsewhere.
ReLU outputs (epilogue 1) whose float64 pre-activation lies within the accumulation bound of 0 are held to that bound as an absolute
error: which side of 0 the fp32 sum falls on is not decided there.  Where sign-bit words are read, the expected gate is the writer's
own stored output > 0, the definition of the words.
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DERIV = (3, 4, 5, 6, 8)                   # epilogues that read H (act_cols applies to them)
SP_FAMILY, RELU_FAMILY = (4, 5, 6), (3, 8)
GR = 3                                    # guard rows on either side of an output matrix
GW = 64                                   # guard words on either side of a sign-bit buffer
WORD = 0x5A5A5A5A5A5A5A5A                 # what the sign-bit buffers hold before a launch
ACC = 4e-7                                # accumulation bound per unit of mass, times max(1, sqrt(K) / 4)

# restatement_distance over every input set of this file (INPUT_SETS), on the MI355X: epilogue -> (R of C, R of C2, R of C over the
# whole mass)
MEASURED_R = {0: (1.04e-7, 0.0, 1.04e-7), 1: (9.69e-8, 0.0, 9.69e-8), 2: (9.69e-8, 0.0, 9.69e-8), 3: (5.38e-8, 0.0, 5.38e-8),
              4: (6.28e-4, 0.0, 1.05e-7), 5: (6.28e-4, 2.98e-7, 1.05e-7), 6: (1.16e-5, 0.0, 1.34e-7), 7: (5.45e-8, 0.0, 5.45e-8),
              8: (9.0e-8, 0.0, 9.0e-8)}


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and the float64 statement of the contract
# ------------------------------------------------------------------------------------------------------------------------------
class _Inputs:
    """One [groups] x (M, N, K) problem's operands in their logical shapes, and the float64 products every epilogue shares."""

    def __init__(self, dev, M, N, K, groups=1):
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000003 * M + 1009 * N + 17 * K + groups)
        self.M, self.N, self.K, self.groups, self.dev = M, N, K, groups, dev

        def randn(*shape):
            return torch.randn(*shape, device=dev, generator=gen)
        self.A = randn(groups, M, K)
        self.W = randn(groups, N, K) / K ** 0.5
        self.bias = randn(groups, N)
        # H of the softplus family: real softplus_100 outputs, some exactly 0 (sp' = 0) and some 0.5 (exp(-100 h) ~ 0)
        pick = torch.rand(groups, M, N, device=dev, generator=gen)
        Hsp = F.softplus(randn(groups, M, N) * 0.02, beta=100)
        self.Hsp = torch.where(pick < 0.02, torch.zeros_like(Hsp), torch.where(pick > 0.98, torch.full_like(Hsp, 0.5), Hsp))
        self.Hre = torch.relu(randn(groups, M, N) * 0.02)            # a ReLU output: half of it exact zeros
        self.D = randn(groups, M, N)
        self.Cadd = randn(groups, M, N)
        self.v64 = self.A.double() @ self.W.double().transpose(1, 2)               # alpha not applied
        self.av64 = self.A.double().abs() @ self.W.double().abs().transpose(1, 2)


@functools.lru_cache(maxsize=16)
def _inputs(dev, M, N, K, groups=1):
    return _Inputs(dev, M, N, K, groups)


def _epilogue(epi, v, b, h, d, ca):
    """(C, C2) of epilogue `epi` as include/nu_nerf.h states it, in the dtype of the arguments."""
    if epi == 0:
        return v + b, None
    if epi == 1:
        return torch.relu(v + b), None
    if epi == 2:
        return F.softplus(v + b, beta=100), None
    if epi == 3:
        return v * (h > 0), None
    if epi == 7:
        return v, None
    if epi == 8:
        return v * (h > 0) + ca, None
    e = torch.exp(-100 * h)                                           # 1 - sp'(H)
    if epi == 4:
        return v * (1 - e), None
    if epi == 5:
        return v * (1 - e), v * d * 100 * e
    if epi == 6:
        return v * (1 - e) + ca, None
    raise ValueError(epi)


def _expect(inp, epi, alpha=1.0, act_cols=0, zero_to=0, gate=None, dtype=torch.float64):
    """The contract on `inp`: (C, C2, bound of C, bound of C2) as [groups, M, max(N, zero_to)] (C2 and its bound None unless Q_SP).
    gate: [groups, M, N] bool replacing H > 0 (what sign-bit words stand for).  dtype float32: the same formulas in torch fp32
    from the fp32-rounded float64 v (the restatement whose distance to float64 is R); the bounds then are the masses."""
    N, K = inp.N, inp.K
    v64 = alpha * inp.v64
    av = abs(alpha) * inp.av64
    v = v64.to(dtype)
    b = inp.bias.to(dtype).unsqueeze(1)
    h = (gate.to(dtype) if gate is not None else inp.Hre.to(dtype)) if epi in RELU_FAMILY else inp.Hsp.to(dtype)
    d, ca = inp.D.to(dtype), inp.Cadd.to(dtype)
    C, C2 = _epilogue(epi, v, b, h, d, ca)
    # |d out / d v| and the additive terms, float64
    x64 = v64 + inp.bias.double().unsqueeze(1) if epi <= 2 else None
    e64 = torch.exp(-100 * inp.Hsp.double()) if epi in SP_FAMILY else None
    if epi in (0, 7):
        dfac = 1.0
    elif epi == 1:
        dfac = (x64 > 0).double()
    elif epi == 2:
        dfac = torch.sigmoid(100 * x64)
    elif epi in RELU_FAMILY:
        dfac = (h > 0).double()
    else:
        dfac = 1 - e64
    add = inp.bias.double().abs().unsqueeze(1) if epi <= 2 else (inp.Cadd.double().abs() if epi in (6, 8) else 0.0)
    mass = av * dfac + add
    mass2 = av * (100 * inp.D.double() * e64).abs() if epi == 5 else None
    plain = epi in DERIV and 0 < act_cols < N
    if plain:
        C = torch.cat([C[..., :act_cols], v[..., act_cols:]], -1)
        mass = torch.cat([mass[..., :act_cols], av[..., act_cols:]], -1)
        if C2 is not None:
            C2 = torch.cat([C2[..., :act_cols], torch.zeros_like(v[..., act_cols:])], -1)
            mass2 = torch.cat([mass2[..., :act_cols], torch.zeros_like(av[..., act_cols:])], -1)
    if dtype == torch.float64:
        acc = ACC * max(1.0, math.sqrt(K) / 4)
        r, r2, rflat = MEASURED_R[epi]
        # both bounds hold (see the module docstring): the mass-relative one, and the one with the activation term on the whole mass
        bound = torch.minimum((acc + 4 * r) * mass, acc * mass + 4 * rflat * (av + add))
        if epi == 1:          # the sign of a pre-activation inside the accumulation bound is open: absolute error only
            full = acc * (av + add)
            bound = torch.where(x64.abs() <= full, full, bound)
        bound2 = (acc + 4 * r2) * mass2 if mass2 is not None else None
    else:
        # the masses themselves; C's as a pair with the whole mass |alpha| |A| |W|^T + |bias| + |Cadd| (no |d out / d v|)
        bound, bound2 = torch.stack([mass.expand_as(av), (av + add).expand_as(av)]), mass2
    if zero_to > N:
        def pad(t):
            return torch.cat([t, torch.zeros(*t.shape[:-1], zero_to - N, dtype=t.dtype, device=t.device)], -1)
        C, bound = pad(C), pad(bound)
        if C2 is not None:
            C2, bound2 = pad(C2), pad(bound2)
    return C, C2, bound, bound2


# (M, N, K, groups) of every input set the tests below draw: what R is measured over
INPUT_SETS = []


def restatement_distance(inp, epi, alpha=1.0, act_cols=0):
    """max |fp32 restatement - float64| / mass of epilogue `epi` on `inp`: C over its mass, C2 over its mass, C over the whole mass
    (elements of zero mass must agree exactly)."""
    C64, C264, _, _ = _expect(inp, epi, alpha, act_cols)
    C32, C232, masses, mass2 = _expect(inp, epi, alpha, act_cols, dtype=torch.float32)
    out = []
    for a, b, m in ((C32, C64, masses[0]), (C232, C264, mass2), (C32, C64, masses[1])):
        if a is None:
            out.append(0.0)
            continue
        err = (a.double() - b).abs()
        if epi == 1:          # a float64 pre-activation that rounds across 0 in fp32: outside what R describes (see the module docstring)
            x = alpha * inp.v64 + inp.bias.double().unsqueeze(1)
            err = torch.where(x.abs() <= ACC * (abs(alpha) * inp.av64 + inp.bias.double().abs().unsqueeze(1)), torch.zeros_like(err), err)
        assert bool((err[m == 0] == 0).all())
        out.append(float((err / m.clamp_min(1e-300)).max()) if err.numel() else 0.0)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------
# buffers, launches, checks
# ------------------------------------------------------------------------------------------------------------------------------
def _r4(n):
    return (n + 3) // 4 * 4


def _strided(X, ld, valid_cols=None, shift=0):
    """X [groups, rows, cols] in a NaN-filled buffer of leading dimension ld, its first `valid_cols` columns kept, element (0, 0, 0)
    `shift` floats behind the (16-byte aligned) start.  Returns (tensor to keep alive, address, group stride)."""
    G, rows, cols = X.shape
    valid = cols if valid_cols is None else min(cols, valid_cols)
    assert shift + valid <= ld
    buf = torch.full((G * rows * ld + 8,), float("nan"), device=X.device)
    view = buf[:G * rows * ld].view(G, rows, ld)
    view[:, :, shift:shift + valid] = X[:, :, :valid]
    return buf, buf.data_ptr() + 4 * shift, rows * ld


class _Out:
    """An output matrix [groups][GR guard rows | M rows | GR guard rows][ld], all NaN before the launch."""

    def __init__(self, dev, groups, M, ld, used_cols):
        assert used_cols <= ld - 1
        self.buf = torch.full((groups, M + 2 * GR, ld), float("nan"), device=dev)
        self.M, self.used = M, used_cols
        self.addr = self.buf.data_ptr() + 4 * GR * ld
        self.stride = (M + 2 * GR) * ld

    def values(self):
        return self.buf[:, GR:GR + self.M, :self.used]

    def guards_untouched(self):
        g = self.buf.clone()
        g[:, GR:GR + self.M, :self.used] = float("nan")
        return bool(torch.isnan(g).all())


class _Words:
    """Sign-bit words of an [M, 128 nct] activation matrix between two runs of guard words."""

    def __init__(self, dev, M, nct):
        self.n = (M + 127) // 128 * nct * 256
        self.nct = nct
        self.buf = torch.full((self.n + 2 * GW,), WORD, dtype=torch.int64, device=dev)
        self.addr = self.buf.data_ptr() + 8 * GW

    def guards_untouched(self):
        return bool((self.buf[:GW] == WORD).all()) and bool((self.buf[GW + self.n:] == WORD).all())


class _Problem:
    """One NuGemmNT on `inp`: buffers laid out with five different leading dimensions, the struct, the expected values."""

    def __init__(self, inp, epi, *, alpha=1.0, zero_to=0, act_cols=0, ldc_odd=False, ldc2_odd=False, h_shift=0, words=None, ct0=0,
                 gate=None, read_words=False):
        from nu_nerf_amd._lib import GemmNT
        G, M, N, K, dev = inp.groups, inp.M, inp.N, inp.K, inp.dev
        self.inp, self.epi, self.alpha, self.zero_to, self.act_cols, self.gate, self.words = inp, epi, alpha, zero_to, act_cols, gate, words
        used = max(N, zero_to)
        Z = _r4(used)
        ldc, ldc2, ldh, ldd, ldadd = Z + 12 + (1 if ldc_odd else 0), Z + 8 - (1 if ldc2_odd else 0), Z + 4, Z + 16, Z + 20
        Np = (N + 127) // 128 * 128
        Wp = torch.zeros(G, Np, K, device=dev)                        # packed weights: ceil128(N) rows, zero padded
        Wp[:, :N] = inp.W
        self.keep = []

        def put(X, ld, valid_cols=None, shift=0):
            buf, addr, stride = _strided(X, ld, valid_cols, shift)
            self.keep.append(buf)
            return addr, stride
        a, sA = put(inp.A, K + 4)
        w, sB = put(Wp, K + 8)
        kw = dict(A=a, lda=K + 4, B=w, ldb=K + 8, M=M, N=N, K=K, zero_to=zero_to, act_cols=act_cols, alpha=alpha, groups=G, sA=sA, sB=sB,
                  epi=epi, bf16=0)
        self.C = _Out(dev, G, M, ldc, used)
        kw.update(C=self.C.addr, ldc=ldc, sC=self.C.stride)
        self.C2 = None
        if epi == 5:
            self.C2 = _Out(dev, G, M, ldc2, used)
            kw.update(C2=self.C2.addr, ldc2=ldc2, sC2=self.C2.stride)
        if epi <= 2:
            kw["bias"], kw["sBias"] = put(inp.bias.unsqueeze(1), N + 5)
        live = min(N, act_cols) if act_cols > 0 else N               # columns whose H / D / Cadd the contract reads
        if epi in DERIV:
            H = inp.Hre if epi in RELU_FAMILY else inp.Hsp
            kw["H"], kw["sH"] = put(H, ldh, 0 if read_words else live, h_shift)      # sign-bit words replace H: all of it is NaN
            kw["ldh"] = ldh
        if epi == 5:
            kw["D"], kw["sD"] = put(inp.D, ldd, live)
            kw["ldd"] = ldd
        if epi in (6, 8):
            kw["Cadd"], kw["sCadd"] = put(inp.Cadd, ldadd, live)
            kw["ldadd"] = ldadd
        if words is not None:
            kw.update(mask=words.addr, mask_nct=words.nct, mask_ct0=ct0)
        self.kw = kw
        self.g = GemmNT(**kw)

    def check(self, what):
        """The launch's outputs against the contract; returns the largest error / bound it saw."""
        C, C2, bound, bound2 = _expect(self.inp, self.epi, self.alpha, self.act_cols, self.zero_to, self.gate)
        worst = 0.0
        for name, out, want, bnd in (("C", self.C, C, bound), ("C2", self.C2, C2, bound2)):
            if out is None:
                continue
            got = out.values().double()
            err = (got - want).abs()
            ok = err <= bnd                                            # (NaN: not ok)
            ratio = float((err / bnd.clamp_min(1e-300))[bnd > 0].max()) if bool((bnd > 0).any()) else 0.0
            nbad = int((~ok).sum())
            if nbad:
                i = tuple(int(t[0]) for t in torch.nonzero(~ok)[:1].unbind(1))
                raise AssertionError(f"{what} epi {self.epi} {name}: {nbad} of {ok.numel()} elements off; first (group, row, col) {i}: got "
                                     f"{float(got[i])!r} want {float(want[i])!r} bound {float(bnd[i])!r}; largest finite error / bound {ratio:.3g}")
            assert out.guards_untouched(), f"{what} epi {self.epi} {name}: a guard row or column was written"
            worst = max(worst, ratio)
        if self.words is not None:
            assert self.words.guards_untouched(), f"{what} epi {self.epi}: a guard word of the sign bits was written"
        return worst


def _lib():
    from nu_nerf_amd import _lib as L
    return L, L.load()


def _launch(p, rows):
    L, lib = _lib()
    assert lib.nu_gemm_nt_tile_rows(ctypes.byref(p.g), 1) == rows
    assert lib.nu_gemm_nt_ex(ctypes.byref(p.g), L.stream()) == 0
    return p


def _launch_batch(probs, rows):
    L, lib = _lib()
    from nu_nerf_amd._lib import GemmNT
    arr = (GemmNT * len(probs))(*[p.g for p in probs])
    assert lib.nu_gemm_nt_tile_rows(arr, len(probs)) == rows
    assert lib.nu_gemm_nt_batch(arr, len(probs), L.stream()) == 0
    return probs


def _report(name, worst):
    print(f"\n[nt paths] {name}: largest error / bound " + " ".join(f"{k}:{v:.2f}" for k, v in sorted(worst.items())))


def _run_all(inp, rows, epis, name, alphas=(1.0,), **kw):
    worst = {}
    for epi in epis:
        for alpha in alphas:
            p = _launch(_Problem(inp, epi, alpha=alpha, **kw), rows)
            worst[epi] = max(worst.get(epi, 0.0), p.check(f"{name} alpha {alpha}"))
    _report(name, worst)


def _zero_to(N):
    return N // 32 * 32 + 32                # the next multiple of 32 past N


# ------------------------------------------------------------------------------------------------------------------------------
# 1. 64-row kernel, every epilogue, edge shapes
# ------------------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(1, 1, 32), (63, 3, 64), (64, 64, 32), (65, 67, 64), (129, 128, 32), (200, 130, 64), (200, 217, 96), (129, 340, 288),
               (1, 340, 32), (63, 128, 64), (64, 217, 32), (65, 130, 32), (200, 256, 64)]
INPUT_SETS += [(M, N, K, 1) for M, N, K in EDGE_SHAPES]


@pytest.mark.parametrize("M,N,K", EDGE_SHAPES[:12])
def test_64_row_tiles_every_epilogue_at_edge_shapes(gpu, M, N, K):
    """Rows and columns around the tile, slab and lane sizes; K of 1, 2, 3 and 9 chunks; alpha 1 and -0.5; five different leading
    dimensions; zero-filled pad columns."""
    _run_all(_inputs(gpu, M, N, K), 64, range(9), f"edge {M}x{N}x{K}", alphas=(1.0, -0.5), zero_to=_zero_to(N))


def test_zero_to_behind_the_last_column_tile_in_bf16_storage(gpu):
    """Columns [ceil128(N), zero_to) lie in no tile of the grid (N = 128, 256 above); the launch itself zeroes them, whichever kernel
    it dispatches to -- here the bf16-storage one, whose C has 2-byte elements.  It is no exact-fp32 launch: tile height 0."""
    from nu_nerf_amd._lib import GemmNT, NU_GEMM_B16, NU_GEMM_C16
    L, lib = _lib()
    M, N, K, zero_to, ld = 70, 128, 32, 160, 176
    inp = _inputs(gpu, M, N, K)
    A, B = inp.A[0].contiguous(), inp.W[0].bfloat16().contiguous()
    C = torch.full((M + GR, ld), float("nan"), device=gpu, dtype=torch.bfloat16)
    g = GemmNT(A=A.data_ptr(), lda=K, B=B.data_ptr(), ldb=K, M=M, N=N, K=K, C=C.data_ptr(), ldc=ld, zero_to=zero_to, alpha=1.0, groups=1,
               epi=7, bf16=1 | NU_GEMM_B16 | NU_GEMM_C16)
    assert lib.nu_gemm_nt_tile_rows(ctypes.byref(g), 1) == 0
    assert lib.nu_gemm_nt_ex(ctypes.byref(g), L.stream()) == 0
    assert bool((C[:M, N:zero_to] == 0).all()) and bool(torch.isnan(C[:M, zero_to:]).all()) and bool(torch.isnan(C[M:]).all())
    torch.testing.assert_close(C[:M, :N].double(), A.bfloat16().double() @ B.double().t(), rtol=8e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the scalar lanes: vec_ok false in three ways
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(200, 217, 96), (200, 256, 64)])
@pytest.mark.parametrize("how", ["ldc_odd", "h_shift", "ldc2_odd"])
def test_scalar_path_when_a_matrix_is_not_16_byte_addressable(gpu, M, N, K, how):
    """An odd ldc (every epilogue), H one float off a 16-byte boundary (the epilogues that read H), an odd ldc2 (Q_SP): each alone
    sends every lane of the launch through the element-wise branch."""
    inp = _inputs(gpu, M, N, K)
    epis, kw = {"ldc_odd": (range(9), dict(ldc_odd=True)), "h_shift": (DERIV, dict(h_shift=1)), "ldc2_odd": ((5,), dict(ldc2_odd=True))}[how]
    _run_all(inp, 64, epis, f"scalar {how} {M}x{N}", alphas=(1.0, -0.5), zero_to=_zero_to(N), **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. act_cols without sign-bit words
# ------------------------------------------------------------------------------------------------------------------------------
INPUT_SETS += [(200, 340, 64, 1)]


@pytest.mark.parametrize("act_cols", [128, 192, 130])
def test_act_cols_on_64_row_tiles(gpu, act_cols):
    """Plain columns from a column-tile boundary, from a slab boundary (the plain copy of the fast path beside a regular slab of
    one tile) and from a column inside a lane's four; three interior row tiles and a ragged one.  H, D and Cadd are NaN from act_cols on."""
    _run_all(_inputs(gpu, 200, 340, 64), 64, DERIV, f"act_cols {act_cols}", alphas=(1.0, -0.5), zero_to=352, act_cols=act_cols)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. 128-row kernel
# ------------------------------------------------------------------------------------------------------------------------------
INPUT_SETS += [(8155, 256, 32, 4), (16300, 450, 32, 1), (16300, 512, 32, 1), (65500, 128, 32, 1)]


def test_128_row_tiles_every_epilogue_grouped(gpu):
    """Four groups of 8155 x 256 (512 tiles), a ragged last row tile, every group stride different."""
    inp = _inputs(gpu, 8155, 256, 32, 4)
    p = _Problem(inp, 5, zero_to=288)
    strides = [p.kw[k] for k in ("sA", "sB", "sC", "sC2", "sH", "sD")] + [_Problem(inp, 0, zero_to=288).kw["sBias"],
                                                                         _Problem(inp, 6, zero_to=288).kw["sCadd"]]
    assert len(set(strides)) == 8, strides
    _run_all(inp, 128, range(9), "128-row grouped", alphas=(-0.5,), zero_to=288)


def test_128_row_tiles_ragged_last_column_tile(gpu):
    _run_all(_inputs(gpu, 16300, 450, 32), 128, range(9), "128-row N 450", zero_to=480)


@pytest.mark.parametrize("act_cols", [192, 256])
def test_act_cols_on_128_row_tiles(gpu, act_cols):
    _run_all(_inputs(gpu, 16300, 512, 32), 128, DERIV, f"128-row act_cols {act_cols}", alphas=(-0.5,), act_cols=act_cols)


def test_scalar_path_on_128_row_tiles(gpu):
    _run_all(_inputs(gpu, 65500, 128, 32), 128, (2, 5, 6), "128-row odd ldc", ldc_odd=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the persistent walk: several tiles per workgroup, padding slots past the last row tile
# ------------------------------------------------------------------------------------------------------------------------------
INPUT_SETS += [(63990, 256, 32, 1), (40000, 128, 32, 1)]


@pytest.mark.parametrize("M,N,rows", [(63990, 256, 128), (40000, 128, 64)])
def test_persistent_walk_is_right_and_repeatable(gpu, M, N, rows):
    inp = _inputs(gpu, M, N, 32)
    worst = {}
    for epi in (2, 5, 6):
        first = _launch(_Problem(inp, epi), rows)
        worst[epi] = first.check(f"walk {M}x{N}")
        again = _launch(_Problem(inp, epi), rows)                   # fresh buffers
        assert torch.equal(first.C.values(), again.C.values())
        if epi == 5:
            assert torch.equal(first.C2.values(), again.C2.values())
    _report(f"walk {M}x{N}", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. sign-bit words written on one tile height and read on the other
# ------------------------------------------------------------------------------------------------------------------------------
INPUT_SETS += [(16300, 512, 32, 1), (16300, 256, 32, 1), (16300, 256, 64, 1), (16300, 340, 32, 1)]


def _gate_of(writer, c0, c1):
    return writer.C.values()[:, :, c0:c1] > 0


def test_sign_bits_of_a_128_row_writer_read_on_64_row_tiles(gpu):
    M = 16300
    words = _Words(gpu, M, 4)
    writer = _launch(_Problem(_inputs(gpu, M, 512, 32), 1, words=words), 128)
    worst = {"w": writer.check("writer")}
    for ct0, rd in ((0, _inputs(gpu, M, 256, 32)), (2, _inputs(gpu, M, 256, 64))):
        gate = _gate_of(writer, 128 * ct0, 128 * ct0 + 256)
        for epi in RELU_FAMILY:
            r = _launch(_Problem(rd, epi, alpha=-0.5, words=words, ct0=ct0, gate=gate, read_words=True), 64)
            worst[f"{epi}@{ct0}"] = r.check(f"reader at column tile {ct0}")
    # plain columns behind the 256 gated ones
    rd = _inputs(gpu, M, 340, 32)
    gate = torch.cat([_gate_of(writer, 256, 512), torch.zeros(1, M, 84, dtype=torch.bool, device=gpu)], -1)
    for epi in RELU_FAMILY:
        r = _launch(_Problem(rd, epi, words=words, ct0=2, gate=gate, read_words=True, act_cols=256, zero_to=352), 64)
        worst[f"{epi}+plain"] = r.check("reader with plain columns")
    _report("128-row writer, 64-row readers", worst)


def test_sign_bits_of_64_row_writers_read_on_128_row_tiles(gpu):
    M = 16300
    words = _Words(gpu, M, 4)
    writers = [_launch(_Problem(_inputs(gpu, M, 256, K), 1, alpha=a, words=words, ct0=ct0), 64) for ct0, K, a in ((0, 32, 1.0), (2, 64, -0.5))]
    worst = {f"w{i}": w.check("writer") for i, w in enumerate(writers)}
    gate = torch.cat([_gate_of(w, 0, 256) for w in writers], -1)
    rd = _inputs(gpu, M, 512, 32)
    for epi in RELU_FAMILY:
        r = _launch(_Problem(rd, epi, words=words, gate=gate, read_words=True), 128)
        worst[str(epi)] = r.check("128-row reader")
    _report("64-row writers, 128-row reader", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. nu_gemm_nt_batch
# ------------------------------------------------------------------------------------------------------------------------------
BATCH_SMALL = [(200, 217, 96), (0, 64, 32), (1, 130, 64), (129, 340, 288), (65, 67, 64)]
BATCH_SMALL_64 = [(200, 256, 64), (0, 64, 32), (1, 128, 32), (129, 64, 64), (64, 64, 32)]         # N % 64 == 0: sign-bit writers
BATCH_BIG = [(8155, 256, 32), (8192, 256, 64), (8100, 256, 32), (8129, 256, 32), (8065, 256, 64), (8190, 256, 32), (8180, 256, 32), (8170, 256, 32)]
INPUT_SETS += [(M, N, K, 1) for M, N, K in BATCH_SMALL + BATCH_SMALL_64 + BATCH_BIG if M > 0] + [(129, 128, 32, 2)]


def _check_all(probs, name):
    worst = {}
    for i, p in enumerate(probs):
        worst[f"{i}/e{p.epi}"] = p.check(f"{name} problem {i}")
    _report(name, worst)


@pytest.mark.parametrize("shapes,rows", [(BATCH_SMALL, 64), (BATCH_BIG, 128)])
@pytest.mark.parametrize("epi", [0, 7])
def test_batch_of_bias_and_plain_epilogues(gpu, shapes, rows, epi):
    """Problems of different M (0 and 1 among them), ragged N and different K in one launch, against the contract."""
    probs = [_Problem(_inputs(gpu, M, N, K), epi, alpha=(-0.5 if i % 2 else 1.0), zero_to=_zero_to(N)) for i, (M, N, K) in enumerate(shapes)]
    _check_all(_launch_batch(probs, rows), f"batch epi {epi} ({rows}-row)")


@pytest.mark.parametrize("shapes,rows", [(BATCH_SMALL_64, 64), (BATCH_BIG, 128)])
def test_batch_of_relu_writers_then_readers(gpu, shapes, rows):
    """BIAS_RELU problems with their own sign-bit buffers in one launch, then MUL_DRELU problems that read them (H is NaN)."""
    words = [_Words(gpu, M, (N + 127) // 128) for M, N, K in shapes]
    writers = [_Problem(_inputs(gpu, M, N, K), 1, words=w) for (M, N, K), w in zip(shapes, words)]
    _check_all(_launch_batch(writers, rows), f"batch writers ({rows}-row)")
    readers = [_Problem(_inputs(gpu, M, N, K), 3, alpha=-0.5, words=w, gate=_gate_of(wr, 0, N), read_words=True)
               for (M, N, K), w, wr in zip(shapes, words, writers)]
    _check_all(_launch_batch(readers, rows), f"batch readers ({rows}-row)")


def test_batch_list_with_a_change_of_epilogue(gpu):
    probs = [_Problem(_inputs(gpu, M, N, K), epi, zero_to=_zero_to(N)) for (M, N, K), epi in zip(BATCH_SMALL, (0, 0, 0, 7, 7))]
    _check_all(_launch_batch(probs, 64), "batch 0 0 0 7 7")


def test_batch_list_of_epilogues_without_a_batch_build(gpu):
    probs = [_Problem(_inputs(gpu, M, N, K), epi, zero_to=_zero_to(N)) for (M, N, K), epi in zip(BATCH_SMALL, (2, 2, 4, 4, 2))]
    _check_all(_launch_batch(probs, 64), "batch 2 2 4 4 2")


def test_batch_list_longer_than_one_launch_takes(gpu):
    """Five two-group problems and a single one: 11 problems after group expansion, NU_NT_BATCH_MAX is 8."""
    from nu_nerf_amd._lib import NU_NT_BATCH_MAX
    assert NU_NT_BATCH_MAX == 8
    two = _inputs(gpu, 129, 128, 32, 2)
    probs = [_Problem(two, 0, alpha=1.0 + i, zero_to=160) for i in range(5)] + [_Problem(_inputs(gpu, 65, 67, 64), 0)]
    _check_all(_launch_batch(probs, 64), "batch of 11")


def test_batch_of_nothing(gpu):
    L, lib = _lib()
    assert lib.nu_gemm_nt_batch(None, 0, L.stream()) == L.NU_OK


# ------------------------------------------------------------------------------------------------------------------------------
# the recorded R still describes these inputs
# ------------------------------------------------------------------------------------------------------------------------------
def test_recorded_restatement_distance_covers_the_small_inputs(gpu):
    """MEASURED_R is a recorded figure: it must not fall behind the inputs (a new shape, another H distribution)."""
    for M, N, K in EDGE_SHAPES:
        inp = _inputs(gpu, M, N, K)
        for epi in range(9):
            for alpha in (1.0, -0.5):
                r = restatement_distance(inp, epi, alpha)
                assert all(x <= y for x, y in zip(r, MEASURED_R[epi])), (M, N, K, epi, alpha, r)
