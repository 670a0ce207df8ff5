"""Float64 restatement of the SDF curvature (nu_nerf_amd/curvature.py, csrc/sdf_jet.hip): gradient and Hessian of
oracle.stage1_oracle.sdf_forward by torch autograd, the curvature formulas in float64 numpy, and the closed forms the tests pin the
formulas and the kernel to.  Shares no code with the package's evaluation."""
import math

import numpy as np
import torch

HESS_ORDER = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))        # xx, yy, zz, xy, xz, yz


def curvatures(g, H6, eps2=1e-12):
    """(mean [P], gaussian [P], normal [P,3]) from g [P,3] and H6 [P,6] (HESS_ORDER), float64:
    mean = (|g|^2 tr H - g^T H g) / (2 |g|^3), gaussian = g^T adj(H) g / |g|^4, normal = g / |g|; zeros where |g|^2 < eps2."""
    g, H6 = np.asarray(g, np.float64), np.asarray(H6, np.float64)
    H = np.zeros((len(g), 3, 3))
    for n, (i, j) in enumerate(HESS_ORDER):
        H[:, i, j] = H[:, j, i] = H6[:, n]
    g2 = np.einsum('pi,pi->p', g, g)
    ok = g2 >= eps2
    safe = np.where(ok, g2, 1.0)
    gHg = np.einsum('pi,pij,pj->p', g, H, g)
    mean = (g2 * np.trace(H, axis1=1, axis2=2) - gHg) / (2.0 * safe ** 1.5)
    adj = np.zeros_like(H)                                            # adjugate = transposed cofactors
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            m = H[:, r][:, :, c]
            adj[:, i, j] = (-1) ** (i + j) * (m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0])
    gauss = np.einsum('pi,pij,pj->p', g, adj, g) / safe ** 2
    normal = g / np.sqrt(safe)[:, None]
    return np.where(ok, mean, 0.0), np.where(ok, gauss, 0.0), np.where(ok[:, None], normal, 0.0)


def jet_of(fn, x, device=None):
    """(f [P], g [P,3], H6 [P,6]) float64 numpy of the scalar field fn (torch, float64, [P,3] -> [P]) by autograd (on `device`)."""
    x = torch.as_tensor(np.asarray(x, np.float64)).clone().to(device).requires_grad_(True)
    with torch.enable_grad():
        f = fn(x)
        (g,) = torch.autograd.grad(f.sum(), x, create_graph=True)
        rows = [torch.autograd.grad(g[:, i].sum(), x, retain_graph=True)[0] for i in range(3)]
    H = torch.stack(rows, 1)                                         # [P,3,3]
    H6 = torch.stack([H[:, i, j] for i, j in HESS_ORDER], 1)
    return f.detach().cpu().numpy(), g.detach().cpu().numpy(), H6.detach().cpu().numpy()


def params64(arrays, prefix_from='sdf_network', prefix_to='sdf_network'):
    """The SDF network's parameters as float64 CPU tensors under the oracle's names."""
    return {prefix_to + k[len(prefix_from):]: torch.from_numpy(np.asarray(v)).double()
            for k, v in arrays.items() if k.startswith(prefix_from + '.')}


def sdf_jet64(arrays, x, prefix='sdf_network', device=None):
    """Float64 oracle of the kernel: dict sdf [P], gradient [P,3], hessian [P,6], mean [P], gaussian [P], normal [P,3] of the SDF network
    whose parameters are arrays[prefix + '.lin*']."""
    from oracle import stage1_oracle as O
    p64 = {k: v.to(device) for k, v in params64(arrays, prefix, 'sdf_network').items()}
    f, g, H6 = jet_of(lambda t: O.sdf_forward(p64, t)[:, 0], x, device)
    mean, gauss, normal = curvatures(g, H6)
    return {'sdf': f, 'gradient': g, 'hessian': H6, 'mean': mean, 'gaussian': gauss, 'normal': normal}


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def ellipsoid_gaussian(x, abc):
    """Gaussian curvature of the ellipsoid sum (x_i / a_i)^2 = const through x: K = 1 / (a b c s^2)^2 for the point scaled onto the
    unit-level ellipsoid, s = sum x_i^2 / a_i^4 there."""
    x, abc = np.asarray(x, np.float64), np.asarray(abc, np.float64)
    lam = np.sqrt(np.sum((x / abc) ** 2, 1))                         # x lies on the ellipsoid with semi-axes lam * abc
    ax = lam[:, None] * abc
    s = np.sum(x ** 2 / ax ** 4, 1)
    return 1.0 / (np.prod(ax, 1) * s) ** 2


# ---- the analytic network -----------------------------------------------------------------------------------------------------------
SHIFT = 2.0          # every hidden pre-activation is a column of the embedding (|.| <= 1 inside the unit ball) + SHIFT >= 1


def embed_col(k, c, cos):
    """Column of get_embedder(6, 3) holding sin / cos (2^k x_c)."""
    return 3 + 6 * k + (3 if cos else 0) + c


def analytic_coefficients(seed=5, only_cos0=False):
    """(A [39], B [39]) float32: head weights on the embedding columns that reach the head through layers 0..7 (A) and through the
    skip into layer 4 (B).  Amplitudes fall as 2^-k so that the gradient stays O(1); every frequency up to k = 5 is present on both
    paths.  only_cos0: nothing but the cos(x_c) columns, a field whose gradient vanishes at the origin."""
    A, B = np.zeros(39), np.zeros(39)
    if only_cos0:
        A[[embed_col(0, c, True) for c in range(3)]] = (0.5, -0.25, 0.75)
        B[embed_col(0, 1, True)] = 0.125
        return A.astype(np.float32), B.astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(seed))
    A[:3] = (0.9, -0.4, 0.6)                                         # c . x keeps |g| away from zero
    B[:3] = (0.1, 0.2, -0.1)
    for k in range(6):
        for c in range(3):
            for cos in (False, True):
                A[embed_col(k, c, cos)] = rng.uniform(-0.12, 0.12) / 2 ** k
                B[embed_col(k, c, cos)] = rng.uniform(-0.06, 0.06) / 2 ** k
    return A.astype(np.float32), B.astype(np.float32)


def analytic_overrides(A, B, template, prefix='sdf_network'):
    """Parameter overrides (weight_v / weight_g / bias of lin0..lin8, shaped as in `template`) in which every hidden layer passes its
    input through: lin0 writes embedding column i + SHIFT to hidden column i, the 256-wide layers are identities (softplus(beta = 100)
    is the identity from z = 0.2 on), lin3 keeps the first 217 columns, lin4 also takes the 39 skip columns (+ SHIFT) into hidden
    columns 217..255 -- its weight_g sqrt 2 cancels the skip's 1 / sqrt 2 -- and the sdf row of lin8 sums A over columns 0..38 and B
    over 217..255 with a bias that undoes the shifts: f = sum_i (A_i + B_i) E_i(x), E the embedding."""
    out = {}

    def put(l, W, b):
        W = np.asarray(W, np.float64)
        norm = np.linalg.norm(W, axis=1, keepdims=True)
        assert (norm > 0).all()
        for name, a in (('weight_v', W), ('weight_g', norm), ('bias', np.asarray(b, np.float64))):
            key = f'{prefix}.lin{l}.{name}'
            out[key] = a.astype(np.float32).reshape(template[key].shape)

    W0 = np.zeros((256, 39))
    W0[np.arange(39), np.arange(39)] = 1.0
    W0[39:, 0] = 1.0                                                  # unused hidden columns: x_0 + SHIFT (a zero row has no weight norm)
    put(0, W0, np.full(256, SHIFT))
    for l in (1, 2, 5, 6, 7):
        put(l, np.eye(256), np.zeros(256))
    put(3, np.eye(256)[:217], np.zeros(217))
    W4 = np.zeros((256, 256))
    W4[np.arange(256), np.arange(256)] = math.sqrt(2.0)               # columns 217..255 of the input are the skip embedding
    b4 = np.zeros(256)
    b4[217:] = SHIFT
    put(4, W4, b4)
    W8 = np.asarray(template[f'{prefix}.lin8.weight_v'], np.float64).copy()
    W8[0] = 0.0
    W8[0, :39] = A
    W8[0, 217:] = B
    b8 = np.asarray(template[f'{prefix}.lin8.bias'], np.float64).copy()
    b8[0] = -SHIFT * (float(np.sum(A.astype(np.float64))) + float(np.sum(B.astype(np.float64))))
    put(8, W8, b8)
    return out


def analytic_jet(A, B, x):
    """Closed form of the analytic network: (f [P], g [P,3], H6 [P,6]) float64 at x [P,3] (the float32 points, widened)."""
    x = np.asarray(x, np.float64)
    C = A.astype(np.float64) + B.astype(np.float64)
    f = x @ C[:3]
    g = np.tile(C[:3], (len(x), 1))
    H6 = np.zeros((len(x), 6))
    for k in range(6):
        w = 2.0 ** k
        for c in range(3):
            s, co = np.sin(w * x[:, c]), np.cos(w * x[:, c])
            a, b = C[embed_col(k, c, False)], C[embed_col(k, c, True)]
            f = f + a * s + b * co
            g[:, c] += w * (a * co - b * s)
            H6[:, c] += -w * w * (a * s + b * co)
    return f, g, H6
