"""Float64 restatements of the stage-1 input encodings (TEST INFRASTRUCTURE -- not a test, not product code).

Plain torch on the CPU, written from the formulas the header comments of nu_nerf_amd/csrc/encode.hip cite (network/field.py:14-61,
:447-464, :636-689, utils/ref_utils.py:84-114, network/renderer_zerothick.py:687-690); no code of the kernels is used.  Every
function takes and returns float64 tensors and is differentiable by autograd.  tests/test_encode_oracle_host.py anchors these on
data recorded from the original project before tests/test_encode_ops_gpu.py compares a kernel with them."""
import numpy as np
import torch

from oracle.stage1_oracle import _IDE_ML, _IDE_MAT        # (m, l) list and coefficient matrix of the IDE (ref_utils.py:7-79)

IDE_M = torch.from_numpy(_IDE_ML[:, 0]).long()            # [36] order m of term i
IDE_L = torch.from_numpy(_IDE_ML[:, 1]).double()          # [36] degree l of term i
IDE_MAT = torch.from_numpy(_IDE_MAT).double()             # [17, 36] coefficient of z^k of term i
IDE_SIGMA = 0.5 * IDE_L * (IDE_L + 1)                     # attenuation exponent l (l + 1) / 2
# sum_k |c_k| per term: fp32 Horner evaluation of a term's polynomial carries eps * this much absolute error (up to 1e5 at l = 16)
IDE_KAPPA = IDE_MAT.abs().sum(0)


def embed64(x, n_freq):
    """[x, sin(2^k x), cos(2^k x)]_k of a D-vector (field.py:14-61): column D + 2 D k + c is sin(2^k x_c), D more is the cosine."""
    cols = [x]
    for k in range(n_freq):
        cols += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(cols, -1)


def embed_columns(dim, n_freq):
    """Per column of embed64: (coordinate c, frequency f (1 for the raw columns), column of the partner whose value times `sign`
    times f is the derivative: d sin(f x) = f cos(f x), d cos(f x) = -f sin(f x); the raw columns have partner -1, derivative 1)."""
    n = dim * (1 + 2 * n_freq)
    c, f, partner, sign = np.zeros(n, np.int64), np.ones(n), -np.ones(n, np.int64), np.ones(n)
    for col in range(n):
        if col < dim:
            c[col] = col
            continue
        k, r = divmod(col - dim, 2 * dim)
        c[col], f[col] = r % dim, 2.0 ** k
        partner[col], sign[col] = (col + dim, 1.0) if r < dim else (col - dim, -1.0)
    return torch.from_numpy(c), torch.from_numpy(f), torch.from_numpy(partner), torch.from_numpy(sign)


def ide64(d, kinv):
    """Integrated directional encoding, 72-d (ref_utils.py:84-114): (x + i y)^m P_i(z) exp(-l (l + 1) / 2 kinv), [Re(36), Im(36)]."""
    xx, yy, zz = d[..., 0:1], d[..., 1:2], d[..., 2:3]
    zp = torch.cat([torch.ones_like(zz)] + [zz ** i for i in range(1, 17)], -1)
    re, im = [torch.ones_like(xx)], [torch.zeros_like(xx)]
    for _ in range(16):
        re.append(re[-1] * xx - im[-1] * yy)
        im.append(re[-2] * yy + im[-1] * xx)
    re, im = torch.cat(re, -1)[..., IDE_M], torch.cat(im, -1)[..., IDE_M]
    att = torch.exp(-IDE_SIGMA * kinv)
    poly = zp @ IDE_MAT
    return torch.cat([re * poly * att, im * poly * att], -1)


def shade_dirs64(n, d):
    """n^ = n / |n|, v^ = -d / |d|, NoV = n^ . v^, r = 2 NoV n^ - v^ (field.py:686-689) and 1 / |n|; NoV and 1 / |n| as [P, 1]."""
    inorm = 1.0 / torch.linalg.norm(n, dim=-1, keepdim=True).clamp_min(1e-12)
    nh = n * inorm
    vh = -d / torch.linalg.norm(d, dim=-1, keepdim=True).clamp_min(1e-12)
    nov = torch.sum(nh * vh, -1, keepdim=True)
    return nh, vh, nov, nov * nh * 2.0 - vh, inorm


def sphere_point64(x, dirs):
    """Unit point where the ray (x, dirs) leaves the unit sphere, x first moved to radius 0.999 when outside it (field.py:447-464,
    :641-643; restated from nu_nerf_amd/shading_glue.sphere_point)."""
    nrm = torch.linalg.norm(x, dim=-1, keepdim=True)
    pp = torch.where(nrm > 0.999, x / nrm * 0.999, x)
    b = torch.sum(pp * dirs, -1, keepdim=True)
    t = -b + torch.sqrt(b * b - torch.sum(pp * pp, -1, keepdim=True) + 1.0 + 1e-6)
    s = pp + dirs * t
    return s / torch.linalg.norm(s, dim=-1, keepdim=True).clamp_min(1e-12)


def nerf_inputs64(x):
    """(x / |x|, 1 / |x|) of the NeRF++ points (renderer_zerothick.py:687-690)."""
    nn = torch.linalg.norm(x, dim=-1, keepdim=True)
    return x / nn, 1.0 / nn


def shade_rows64(E, x, nh, vh, nov, r, inorm, rho, sphere, refrac_dim):
    """The shading stacks' input rows in the layout documented above shade_encode_fwd_kernel, without the zero pads:
      OLin [3P, 72 | 144] : rows p, P + p, 2P + p = IDE(n^, 1) | IDE(r, rho) | IDE(r, 0); with `sphere` each row is followed by the
                            IDE of the sphere point of x along the same direction at kinv 1 | rho | rho (field.py:643-646)
      ILin [2P, 111]      : [E(39), IDE(r, rho)] | [E(39), IDE(r, 0)]
      IWin [P, 78]        : [E(39), embed(r, 6)]
      RLin [P, 2 rdim]    : [E[:, :rdim], embed(v^, 6)[:, :rdim]]
      SD   [P, 8]         : n^(3), NoV, 1 / |n|, rho, 0, 0
    E [P, 39] is the positional code of the points (an input: the kernel copies it), rho [P, 1] the roughness sigmoid(Mraw[:, 1]),
    the directions are those of shade_dirs64 (separate arguments so that a test can differentiate with respect to each)."""
    one, zero = torch.ones_like(rho), torch.zeros_like(rho)
    ol = [ide64(nh, one), ide64(r, rho), ide64(r, zero)]
    if sphere:
        sn, sr = sphere_point64(x, nh), sphere_point64(x, r)
        ol = [torch.cat([ol[0], ide64(sn, one)], -1), torch.cat([ol[1], ide64(sr, rho)], -1), torch.cat([ol[2], ide64(sr, rho)], -1)]
    return {
        'OLin': torch.cat(ol, 0),
        'ILin': torch.cat([torch.cat([E, ide64(r, rho)], -1), torch.cat([E, ide64(r, zero)], -1)], 0),
        'IWin': torch.cat([E, embed64(r, 6)], -1),
        'RLin': torch.cat([E[:, :refrac_dim], embed64(vh, 6)[:, :refrac_dim]], -1),
        'SD': torch.cat([nh, nov, inorm, rho, zero, zero], -1),
    }
