"""Restatement of the per-ray sphere tracing of csrc/sdf_trace.hip (include/nu_nerf.h: nu_sdf_trace) in torch over
oracle.stage1_oracle.sdf_forward, in float64 (the oracle) and in float32 (every operation rounded separately, in the kernel's order), and
the standard ray set of the sphere-tracing tests.  Shares no code with the package's evaluation.

A ray's march involves its own row only, so the batch form below (per-ray masks, only the live rays evaluated) is the function called on
each ray alone -- which is what tests/golden/sphere_trace.npz pins it to (the reference's sphere_tracing, one ray per call)."""
import numpy as np
import torch

N_RAYS = 2048
RAY_SEED = 20
ORIGIN_RADIUS = 3.0
TARGET_RADIUS = 1.1


def standard_rays(n=N_RAYS, seed=RAY_SEED):
    """(o [n,3], d [n,3]) float32: origins at radius 3 in random directions, each ray aimed at a random target of radius <= 1.1 (uniform
    in radius), unit directions.  PCG64-seeded (the draw is this project's: the set is defined by this function)."""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.standard_normal((n, 3))
    v = g.standard_normal((n, 3))
    r = g.uniform(0.0, TARGET_RADIUS, (n, 1))
    o = ORIGIN_RADIUS * u / np.linalg.norm(u, axis=1, keepdims=True)
    tgt = r * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def sdf_params(arrays, prefix='sdf_network', dtype=torch.float64, device=None):
    """The SDF network's parameters under the oracle's names, in `dtype`."""
    return {'sdf_network' + k[len(prefix):]: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype)
            for k, v in arrays.items() if k.startswith(prefix + '.')}


def sdf_fn(arrays, prefix='sdf_network', dtype=torch.float64, device=None):
    from oracle import stage1_oracle as O
    p = sdf_params(arrays, prefix, dtype, device)
    return lambda x: O.sdf_forward(p, x)[:, 0]


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def entry(o, d, bound_radius, entry_forward=False):
    """(x, t0, bounded) of the bounding-sphere entry in the dtype of o, every operation on its own, in the kernel's order."""
    rb = torch.as_tensor(bound_radius, dtype=o.dtype, device=o.device)
    a = _dot(d, d)
    b = 2 * _dot(d, o)
    c = _dot(o, o) - rb * rb
    disc = b * b - (4 * a) * c
    bounded = disc >= 0
    t0 = (-b - torch.sqrt(disc)) / (2 * a)
    if entry_forward:
        t0 = torch.clamp(t0, min=0)
    t0 = torch.where(bounded, t0, torch.zeros_like(t0))
    x = torch.where(bounded[:, None], o + d * t0[:, None], o)
    return x, t0, bounded


@torch.no_grad()
def trace(f, o, d, *, dtype=torch.float64, fg=None, max_iter=200, threshold=1e-5, bound_radius=1.0, entry_forward=False, device=None):
    """The per-ray algorithm on rays o, d (numpy or tensors; widened / narrowed to `dtype`) with the scalar field f ([P,3] -> [P]) ->
    dict of numpy arrays pos [R,3], t, sdf [R], iters [R] int32, hit [R] bool, entered [R] bool (foreground after the entry step)."""
    o = torch.as_tensor(o).to(device=device, dtype=dtype)
    d = torch.as_tensor(d).to(device=device, dtype=dtype)
    R = o.shape[0]
    fgr = torch.isfinite(o).all(1)
    if fg is not None:
        fgr = fgr & torch.as_tensor(fg).to(device=o.device).bool()
    x, t = o.clone(), torch.zeros(R, dtype=dtype, device=o.device)
    if bound_radius:
        xe, t0, bounded = entry(o, d, bound_radius, entry_forward)
        fgr = fgr & bounded
        x, t = xe, t0
    x = torch.where(fgr[:, None], x, o)                # a ray that never is foreground stays at its origin with t = 0
    t = torch.where(fgr, t, torch.zeros_like(t))
    entered = fgr.clone()
    iters = torch.zeros(R, dtype=torch.int32, device=o.device)
    last = torch.zeros(R, dtype=dtype, device=o.device)
    conv = torch.zeros(R, dtype=torch.bool, device=o.device)
    live = fgr.clone()
    thr = torch.as_tensor(threshold, dtype=dtype, device=o.device)
    rb = torch.as_tensor(bound_radius or 0.0, dtype=dtype, device=o.device)
    for i in range(max_iter):
        idx = live.nonzero().reshape(-1)
        if idx.numel() == 0:
            break
        s = torch.clamp(f(x[idx]), -10, 10)
        s = torch.nan_to_num(s, nan=10.0)
        xn = x[idx] + d[idx] * s[:, None]
        x[idx] = xn
        t[idx] = t[idx] + s
        iters[idx] = i + 1
        last[idx] = s
        inside = torch.sqrt(_dot(xn, xn)) < rb if bound_radius else torch.ones_like(s, dtype=torch.bool)
        c = s.abs() < thr
        fgr[idx] = inside
        conv[idx] = c
        live[idx] = inside & ~c
    return {'pos': x.cpu().numpy(), 't': t.cpu().numpy(), 'sdf': last.cpu().numpy(), 'iters': iters.cpu().numpy(),
            'hit': (conv & fgr).cpu().numpy(), 'entered': entered.cpu().numpy()}
