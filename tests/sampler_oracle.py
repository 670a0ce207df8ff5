"""Float64 oracle of the hierarchical sampler (csrc/sampler.hip) and the CDF-space judge of its new depths.  Plain torch, no device code.

What is restated (paths of the original project; oracle/stage1_oracle.py:273-313, 384-400 restates the same in fp32):
  upsample     network/renderer_zerothick.py:525-554   mode 0: cos = min(previous interval's cos, cos) clipped to [-1e3, 0], zeroed
                                                       unless one end point of the interval has |x| < 1
  get_weights  network/field.py:501-521                mode 1: cos = min(cos, 0), alpha masked by cos < 0
  sample_pdf   network/field.py:468-498                w = alpha T + 1e-5, cdf, searchsorted(right), den < 1e-5 -> 1
  sample_ray   network/renderer_zerothick.py:572-612   coarse / background depths;  cat_z_vals :556-570 the merge

The criterion.  The inverse CDF amplifies last-bit differences of the weights without bound in z (a bin that holds 1e-5 of the mass
moves a sample across its whole width for a CDF change of 1e-5), so a z-space comparison has to be loose.  In CDF space the kernel
is well conditioned: with the float64 weights of the fp32 inputs the kernel read,
    w_m = alpha_m T_m + 1e-5,  total = sum w_m,  c_0 = 0,  c_{m+1} = c_m + w_m / total,
F the piecewise-linear interpolant through (z_j, c_j), and zq the depth the kernel returned for the quantile u, the residual is the
distance from u to [F-(zq), F+(zq)] (the one-sided limits; they differ only where zq sits on tied knots).  Every sample of every ray
is held to

    B = flat + 4 u24 max|z_r| slope + A_r + K u24 ni / total_r            u24 = 2^-24, ni = sn - 1

  flat   the float64 CDF width of the bin the sample fell in when that width is below 1.1e-5, else 0: sample_pdf's own branch
         (den < 1e-5 -> den = 1) parks such a sample at the bin's lower knot, at most the bin's width from u; the 10 % margin covers
         the fp32 rounding of den (6e-8 on 1e-5).
  slope  CDF width / z width of the bin: the rounding of z_new to fp32 and of z_lo + t (z_hi - z_lo), carried into CDF space.  0 for
         a bin of zero width ([F-, F+] covers it).  A sample that sits exactly on a knot lies in both closed bins that meet there:
         the larger of their two slopes is taken.
  A_r    the cancellation in the sigmoid arguments, derived at arg_term64 (no constant of it is measured): mid -+ cos dz / 2 is
         formed from terms that can each be 100 x the result, and its rounding is multiplied by inv_s and sigmoid'.  On rows of two
         intervals it is the whole error (2.5e-6 in a weight of 0.43, found while calibrating K: without this term the fp32 CPU
         oracle itself needs K_ref = 9.9 on such a row and 0.41 elsewhere).  Its largest value per family is listed with K_ref: at
         most 6e-4, but 4e-3 on rows that start inside the object and whose total is ~1e-3.
  K      what is left: pc - nc + 1e-5 with pc, nc near 1 carries an absolute error of a few u24 against weights of 1e-5, the cdf
         error scales as u24 ni / total.  K = 4 K_REF_MAX, K_REF_MAX = the largest value of
             (residual - flat - slope term - A_r)+ total / (ni u24)
         the fp32 CPU evaluation of the same formulas reaches over every case of CASES (tests/test_sampler_oracle_host.py measures
         it again at every run and holds it to K / 4); the factor 4 allows the kernel's 1 / (1 + expf(-x)) and its chunked products
         a rounding or two more each than torch's.
  wsum   (mode 1: sum alpha_m T_m, the hit probability) is held to KW u24 ni absolute, KW = 4 KW_REF_MAX measured the same way.

Measured K_ref / K_w per group of cases: see the docstring of tests/test_sampler_oracle_host.py and DESIGN.md section 33."""
import collections
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
K_REF_MAX = 0.25      # measured 0.239 (rounded up to a multiple of 0.05), see tests/test_sampler_oracle_host.py
KW_REF_MAX = 1.75     # measured 1.66 (a row of ni = 1; rounded up to a multiple of 0.05)
K = 4.0 * K_REF_MAX
KW = 4.0 * KW_REF_MAX
FLAT = 1.1e-5

SN = (2, 3, 16, 64, 65, 66, 129, 130, 193, 194, 256)
N_NEW = (1, 8, 16, 32, 64, 100)
RS = (1, 5, 37, 400)
FAMILIES = ('through', 'miss', 'graze', 'inside', 'ties', 'second')
PROBE_FAMILIES = ('through', 'inside', 'ties', 'second', 'probe', 'rising')
PROBE_SN = (2, 3, 16, 64, 65, 130, 256)


# ------------------------------------------------------------------------------------------------------------------------------
# the operations, in the dtype of their inputs (float64 for the reference, fp32 for the CPU evaluation that calibrates K)
# ------------------------------------------------------------------------------------------------------------------------------
def _alpha(o, d, z, sdf, inv_s, mode, variant=None):
    """(alpha, mid, cos dz / 2, p, q) of every interval, in the operation order of oracle/stage1_oracle.py (upsample / get_weights)."""
    s0, s1, z0, z1 = sdf[:, :-1], sdf[:, 1:], z[:, :-1], z[:, 1:]
    mid = (s0 + s1) * 0.5
    cos = (s1 - s0) / (z1 - z0 + 1e-5)
    if mode == 0:
        pts = o[:, None, :] + d[:, None, :] * z[..., None]
        r = torch.linalg.norm(pts, dim=-1)
        inside = (r[:, :-1] < 1.0) | (r[:, 1:] < 1.0)
        if variant == 'inside_inverted':
            inside = ~inside
        prev = torch.cat([torch.zeros_like(cos[:, :1]), cos[:, :-1]], -1)
        if variant != 'no_prev_min':
            cos = torch.minimum(prev, cos)
        cos = cos.clip(-1e3, 0.0) * inside
        surf = None
    else:
        surf = cos < 0
        cos = torch.clamp(cos, max=0)
    dz = z1 - z0
    p = torch.sigmoid((mid - cos * dz * 0.5) * inv_s)
    q = torch.sigmoid((mid + cos * dz * 0.5) * inv_s)
    alpha = (p - q + 1e-5) / (p + 1e-5)
    if surf is not None:
        alpha = alpha * surf.to(alpha.dtype)
    return alpha, mid, cos * dz * 0.5, p, q


def _transmittance(alpha):
    ones = torch.ones_like(alpha[..., :1])
    return torch.cumprod(torch.cat([ones, 1. - alpha + 1e-7], -1), -1)[..., :-1]


def weights(o, d, z, sdf, inv_s, mode, variant=None):
    """alpha_m T_m of one round, [R, sn - 1], in the dtype of the inputs.
    variant (the judge's self-test only): 'inside_inverted', 'no_prev_min'."""
    alpha = _alpha(o, d, z, sdf, inv_s, mode, variant)[0]
    return alpha * _transmittance(alpha)


def arg_term64(o, d, z, sdf, inv_s, mode):
    """The part of B that the sigmoid arguments' cancellation contributes, [R, 1], float64:

        A_r = 4 / total_r  sum_m T_m (dp_m + dq_m) / (p_m + 1e-5),   dp_m = sigmoid'(x_p) inv_s u24 (|mid_m| + 6 |b_m|),  b = cos dz / 2

    x = (mid -+ b) inv_s: mid carries one rounding, b six (s1 - s0, z1 - z0, + 1e-5, the division, dz, the product; * 0.5 is exact), so
    mid -+ b is off by up to u24 (|mid| + 6 |b|) HOWEVER SMALL IT IS, and inv_s and sigmoid' carry that into p and q (dq likewise at
    x_q).  alpha = (p - q + 1e-5) / (p + 1e-5) <= 1 moves by at most (dp + dq) / (p + 1e-5) twice over (numerator, denominator); a
    change of alpha_m moves w_m = alpha_m T_m by T_m d alpha_m and all later weights together by no more than that again (they sum to
    at most T_{m+1}); a knot c = partial sum / total moves by at most twice the summed weight changes over total.  2 * 2 = 4 covers
    alpha's two occurrences of p and the normalisation; own + later weights are the two halves of the second factor.
    The roundings relative to the RESULTS of these operations (of x itself, of the sigmoid, of the products) are the K term's."""
    o, d, z, sdf = o.double(), d.double(), z.double(), sdf.double()
    alpha, mid, b, p, q = _alpha(o, d, z, sdf, float(inv_s), mode)
    t = _transmittance(alpha)
    total = (alpha * t + 1e-5).sum(-1, keepdim=True)
    dx = float(inv_s) * U24 * (mid.abs() + 6.0 * b.abs())
    dpq = (p * (1 - p) + q * (1 - q)) * dx * (alpha != 0)       # a masked interval of mode 1 has alpha = 0 whatever p and q
    return 4.0 / total * (t * dpq / (p + 1e-5)).sum(-1, keepdim=True)


def weights64(o, d, z, sdf, inv_s, mode, variant=None):
    """weights() in float64 of the fp32 values the kernel reads; inv_s is what the caller chose (inv_s64)."""
    return weights(o.double(), d.double(), z.double(), sdf.double(), float(inv_s), mode, variant)


def inv_s64(var, cap, use_variance, mode):
    """The kernel's choice: exp(10 var) uncapped in mode 1, min(exp(10 var), cap) with use_variance, else the cap -- the exact
    exponential of the fp32 product the kernel forms (its expf is within an ulp or two of that; the sigmoid arguments that matter
    are below ~20, where 2 ulp of inv_s move a sigmoid by less than 1e-8)."""
    e = math.exp(float(torch.tensor(var, dtype=torch.float32) * 10.0))
    if mode == 1:
        return e
    return min(e, float(cap)) if use_variance else float(cap)


def inv_s32(var, cap, use_variance, mode):
    """The same choice as an fp32 tensor, as oracle/stage1_oracle.py:348-351 forms it."""
    e = torch.exp(torch.tensor(var, dtype=torch.float32) * 10.0)
    if mode == 1:
        return e
    return torch.clamp(e, max=float(cap)) if use_variance else torch.tensor(float(cap))


def sample_pdf(z, raw, u):
    """sample_pdf for the quantiles u [n] (or [R, n]) in the dtype of z: the operations of oracle/stage1_oracle.py:273-289."""
    w = raw + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    u = u.to(z.dtype).expand(list(cdf.shape[:-1]) + [u.shape[-1]]).contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    lo = torch.clamp(idx - 1, min=0)
    hi = torch.clamp(idx, max=cdf.shape[-1] - 1)
    c_lo, c_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    b_lo, b_hi = torch.gather(z, -1, lo), torch.gather(z, -1, hi)
    den = c_hi - c_lo
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    return b_lo + (u - c_lo) / den * (b_hi - b_lo)


def wsum64(raw64):
    """The hit probability nu_probe_weights returns: sum alpha_m T_m without the 1e-5."""
    return raw64.sum(-1)


def coarse_depths(near, far, lin, u1, n):
    """z[r, j] = near + (far - near) lin[j] (+ (u1 - 0.5) 2 / n); near, far [R], u1 [R] or None; dtype of the inputs."""
    z = near[:, None] + (far - near)[:, None] * lin[None, :]
    if u1 is not None:
        z = z + (u1[:, None] - 0.5) * 2.0 / n
    return z


def bg_depths(far, lower, upper, u2, n):
    """The background depths in the order the sampler stores them (reversed): far / flip(zo) + 1 / n, zo = lower (no jitter) or
    lower + (upper - lower) u2."""
    zo = lower[None, :].expand(far.shape[0], n)
    if u2 is not None:
        zo = lower[None, :] + (upper - lower)[None, :] * u2
    return far[:, None] / torch.flip(zo, dims=[-1]) + 1.0 / n


def bg_bins(n, dtype=torch.float32):
    """(lin_bg, lower, upper) of renderer_zerothick.py:578-590 for n background samples."""
    zo = torch.linspace(1e-3, 1.0 - 1.0 / (n + 1.0), n, dtype=dtype)
    mids = 0.5 * (zo[1:] + zo[:-1])
    return zo, torch.cat([zo[:1], mids], -1), torch.cat([mids, zo[-1:]], -1)


def merge(z, s, zn, s_n):
    """cat_z_vals: the sorted concatenation; on equal depths old before new, new in their own order (a stable sort of [old, new]).
    s / s_n may be None."""
    zs, index = torch.sort(torch.cat([z, zn], -1), dim=-1, stable=True)
    return zs, (None if s is None else torch.gather(torch.cat([s, s_n], -1), -1, index))


def sdf_analytic(p):
    """The SDF every family is built on: a 0.5-sphere plus a smooth wobble (|grad wobble| <= 0.23)."""
    return torch.linalg.norm(p, dim=-1) - 0.5 + 0.03 * torch.sin(7.0 * p[..., 0] + 3.0 * p[..., 1])


# ------------------------------------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------------------------------------
Judged = collections.namedtuple('Judged', 'res cw zw slope total')


def cdf_residual(z, raw64, zq, u):
    """For every new depth zq [R, n] returned for the quantiles u [n] (or [R, n]) on the knots z [R, sn] with the float64 weights
    raw64 [R, sn - 1]: (residual, float64 CDF width and z width of the bin the sample fell in, slope, total [R, 1]).
    The bin of a sample strictly between two knots is the one between them; of a sample on a knot (or on tied knots) the bin to the
    right of the last of them, where sample_pdf's den < 1e-5 branch would have put it (the last bin for zq = z_{sn-1})."""
    z, zq = z.double().contiguous(), zq.double().contiguous()
    sn = z.shape[-1]
    u = u.double().expand(zq.shape)
    w = raw64 + 1e-5
    total = w.sum(-1, keepdim=True)
    pdf = w / total
    c = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    ir = torch.searchsorted(z, zq, right=True)         # knots <= zq
    il = torch.searchsorted(z, zq, right=False)        # knots <  zq
    on = ir > il
    lo = torch.clamp(il - 1, 0, sn - 2)
    zl, zh = torch.gather(z, -1, lo), torch.gather(z, -1, lo + 1)
    cl, ch = torch.gather(c, -1, lo), torch.gather(c, -1, lo + 1)
    gap = zh - zl
    t = torch.where(gap > 0, (zq - zl) / torch.where(gap > 0, gap, torch.ones_like(gap)), torch.zeros_like(gap))
    between = cl + t * (ch - cl)                        # beyond the end knots this leaves [0, 1]: such a sample is far off
    f_minus = torch.where(on, torch.gather(c, -1, torch.clamp(il, max=sn - 1)), between)
    f_plus = torch.where(on, torch.gather(c, -1, torch.clamp(ir - 1, min=0)), between)
    res = torch.clamp(torch.maximum(f_minus - u, u - f_plus), min=0.0)
    dzs = z[:, 1:] - z[:, :-1]
    slopes = torch.where(dzs > 0, pdf / torch.where(dzs > 0, dzs, torch.ones_like(dzs)), torch.zeros_like(dzs))
    b = torch.clamp(ir - 1, 0, sn - 2)
    bl = torch.clamp(il - 1, 0, sn - 2)
    slope = torch.maximum(torch.gather(slopes, -1, b), torch.gather(slopes, -1, bl))
    return Judged(res, torch.gather(pdf, -1, b), torch.gather(dzs, -1, b), slope, total)


def bound_parts(z, j, arg):
    """(flat, slope term + argument term) of B for every sample; arg = arg_term64 of the round."""
    flat = torch.where(j.cw < FLAT, j.cw, torch.zeros_like(j.cw))
    zmax = z.double().abs().amax(-1, keepdim=True)
    return flat, 4.0 * U24 * zmax * j.slope + arg


def bound(z, j, arg, k=None):
    flat, st = bound_parts(z, j, arg)
    ni = z.shape[-1] - 1
    return flat + st + (K if k is None else k) * U24 * ni / j.total


def k_ref(z, j, arg):
    """The scaled excess of a set of judged samples: max (residual - flat - slope term - argument term)+ total / (ni u24)."""
    flat, st = bound_parts(z, j, arg)
    ni = z.shape[-1] - 1
    return float((torch.clamp(j.res - flat - st, min=0.0) * j.total / (ni * U24)).max())


# ------------------------------------------------------------------------------------------------------------------------------
# the cases (shared by the host test, which checks their input conditions, and the GPU test)
# ------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return F.normalize(v, dim=-1)


def _grid(R, sn, lo, hi, g):
    """Sorted jittered depths (the generator of tests/test_sampler_ops_gpu.py)."""
    return torch.linspace(lo, hi, sn)[None, :] + (torch.rand(R, sn, generator=g) - 0.5) * ((hi - lo) / sn) * 0.9


def _aimed(R, g, closest):
    """Rays from radius 2.5 whose line passes the origin at the distance `closest` [R]."""
    o = _unit(torch.randn(R, 3, generator=g)) * 2.5
    perp = _unit(torch.cross(o, torch.randn(R, 3, generator=g), dim=-1))
    b = closest * 2.5 / torch.sqrt(2.5 ** 2 - closest ** 2)
    return o, _unit(b[:, None] * perp - o)


def family(fam, R, sn, g):
    """(o, d, z, sdf), fp32, of one ray family."""
    noise = 0.0
    if fam in ('through', 'ties', 'second'):             # towards the unit ball, most of them through the 0.5-sphere
        o = _unit(torch.randn(R, 3, generator=g)) * 2.5
        d = _unit(-o + 0.35 * torch.randn(R, 3, generator=g))
        z = _grid(R, sn, 1.2, 3.8, g)
    elif fam == 'miss':                                  # past the unit ball: every interval outside, a uniform CDF
        o, d = _aimed(R, g, 1.2 + 0.5 * torch.rand(R, generator=g))
        z = _grid(R, sn, 1.2, 3.8, g)
    elif fam == 'graze':                                 # even rows graze the object, odd rows the unit ball
        c = torch.where(torch.arange(R) % 2 == 0, 0.5 + 0.12 * (torch.rand(R, generator=g) - 0.5),
                        1.0 + 0.06 * (torch.rand(R, generator=g) - 0.5))
        o, d = _aimed(R, g, c)
        z = _grid(R, sn, 1.2, 3.8, g)
    elif fam == 'inside':                                # the first samples inside the object: SDF < 0, alpha -> 1; even rows z_0 = 0
        o = _unit(torch.randn(R, 3, generator=g)) * (0.05 + 0.3 * torch.rand(R, 1, generator=g))
        d = _unit(torch.randn(R, 3, generator=g))
        z = _grid(R, sn, 0.0, 2.2, g)
        z[:, 0] = torch.where(torch.arange(R) % 2 == 0, torch.zeros(R), z[:, 0].abs())
    elif fam == 'probe':                                 # the occlusion probe's rows: from inside the unit ball to its surface, z_0 = 0
        o = _unit(torch.randn(R, 3, generator=g)) * (0.2 + 0.75 * torch.rand(R, 1, generator=g))
        d = _unit(torch.randn(R, 3, generator=g))
        dtx, xtx = (o * d).sum(-1), (o * o).sum(-1)
        z = (-dtx + torch.sqrt(dtx ** 2 - xtx + 1 + 1e-6))[:, None] * torch.linspace(0, 1, sn)[None, :]
    elif fam == 'rising':                                # radially outwards: the SDF rises along the whole ray, no interval has cos < 0
        o = _unit(torch.randn(R, 3, generator=g))
        d, o = o.clone(), o * 0.1
        z = _grid(R, sn, 0.0, 0.85, g).abs()
        z = torch.sort(z, dim=-1).values
    else:
        raise ValueError(fam)
    if fam == 'ties':                                    # exact ties and gaps of 1e-6; an SDF that differs across them drives the -1e3 clip
        pick = torch.rand(R, sn - 1, generator=g)
        for j in range(sn - 1):
            z[:, j + 1] = torch.where(pick[:, j] < 0.06, z[:, j], torch.where(pick[:, j] < 0.12, z[:, j] + 1e-6, z[:, j + 1]))
        noise = 0.02
    z = z.contiguous()
    sdf = sdf_analytic(o[:, None, :] + d[:, None, :] * z[..., None])
    if noise:
        sdf = sdf + noise * torch.randn(R, sn, generator=g)
    return o.contiguous(), d.contiguous(), z, sdf.contiguous()


def quantiles(n, ends):
    """The deterministic quantiles of sample_pdf; with `ends` (n >= 3) the first and last are 0 and 1.0."""
    if ends and n >= 3:
        m = n - 2
        return torch.cat([torch.zeros(1), torch.linspace(0.5 / m, 1.0 - 0.5 / m, steps=m), torch.ones(1)])
    return torch.linspace(0.5 / n, 1.0 - 0.5 / n, steps=n)


Case = collections.namedtuple('Case', 'id fam mode R sn n_new kind rnd var ends seed')
_KINDS = (('cap', 0.3), ('var', 0.3), ('capwin', 0.9))     # cap only; exp(3) = 20.1 below every cap; exp(9) = 8103 above every cap
SEEDS = {                                                   # case id -> seed, where the default one breaks an input condition
    'm0-through-sn130-R400-n8-var2-v0.3': 7007,
    'm0-graze-sn194-R400-n8-capwin0-v0.9': 95031,
    'm0-ties-sn64-R400-n100-var2-v0.3': 17047,
    'm0-second-sn256-R400-n16-cap1-v0.3': 7065,
}


def _case(fam, mode, R, sn, n_new, kind, rnd, var, ends, i):
    cid = f"m{mode}-{fam}-sn{sn}-R{R}-n{n_new}-{kind}{rnd if mode == 0 else ''}-v{var}{'-ends' if ends else ''}"
    return Case(cid, fam, mode, R, sn, n_new, kind, rnd, var, ends, SEEDS.get(cid, 1000 + i))


def _cases():
    out = []
    for fi, fam in enumerate(FAMILIES):                   # every family meets every sn; R, n_new, the inv_s rule and the cap rotate
        for si, sn in enumerate(SN):
            i = fi * len(SN) + si
            kind, var = _KINDS[(fi + si) % 3]
            out.append(_case(fam, 0, RS[(fi + si) % 4], sn, N_NEW[(2 * fi + si) % 6], kind, (fi + 2 * si) % 4, var, i % 2 == 0, i))
    for fi, fam in enumerate(PROBE_FAMILIES):
        for si, sn in enumerate(PROBE_SN):
            i = 100 + fi * len(PROBE_SN) + si
            out.append(_case(fam, 1, RS[(fi + si + 1) % 4], sn, N_NEW[(fi + 2 * si + 1) % 6], 'probe', 0, (0.3, 0.7)[(fi + si) % 2],
                             i % 2 == 1, i))
    return out


CASES = _cases()


def make_case(c):
    """(o, d, z, sdf, u) of a case: fp32 CPU tensors.  'second' rows: a grid merged with the float64 oracle's own new depths of a
    first round (rounded to fp32), the SDF evaluated at them -- realistically narrow bins."""
    assert torch.get_default_dtype() == torch.float32
    g = torch.Generator().manual_seed(c.seed)
    n_add = 0
    if c.fam == 'second':
        n_add = min(c.sn - max(2, c.sn // 2), 64)
    o, d, z, sdf = family(c.fam, c.R, c.sn - n_add, g)
    if n_add:
        raw = weights64(o, d, z, sdf, 64.0, c.mode)
        zn = sample_pdf(z.double(), raw, quantiles(n_add, False)).float()
        sn_ = sdf_analytic(o[:, None, :] + d[:, None, :] * zn[..., None])
        z, sdf = merge(z, sdf, zn, sn_)
        z, sdf = z.contiguous(), sdf.contiguous()
    return o, d, z, sdf, quantiles(c.n_new, c.ends)


def input_conditions(c, o, d, z, sdf):
    """(distance of the nearest sample radius from 1, relative distance of the nearest raw cosine from the -1e3 clip), float64.
    The kernel decides `inside` from an fp32 radius and the clip from an fp32 cosine: a case must keep clear of both thresholds
    (4e-6 and 1e-3) so that the float64 reference takes the same side."""
    o, d, z, sdf = o.double(), d.double(), z.double(), sdf.double()
    r = torch.linalg.norm(o[:, None, :] + d[:, None, :] * z[..., None], dim=-1)
    cos = (sdf[:, 1:] - sdf[:, :-1]) / (z[:, 1:] - z[:, :-1] + 1e-5)
    return float((r - 1.0).abs().min()), float(((cos + 1e3).abs() / 1e3).min())
