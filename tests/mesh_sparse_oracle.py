"""Numpy restatement of the block-sparse extraction's host-checkable parts (nu_nerf_amd/mesh_sparse.py, csrc/mcubes_sparse.hip,
DESIGN.md 37): region geometry and the activation rule, the blocks a dense grid requires, analytic 1-Lipschitz fields, and the
canonical form in which two meshes are compared.  No tolerance lives here: everything is compared as integers or bits, except the
radii, which a test may compare within 1 ulp (the device's double-precision sqrt is the one operation numpy need not reproduce)."""
import numpy as np
import torch


def axes(res, lo=-1.0, hi=1.0):
    """The three grid vectors of mesh.sdf_grid: CPU torch.linspace, fp32."""
    return [torch.linspace(lo, hi, n).numpy() for n in (res if isinstance(res, tuple) else (res,) * 3)]


def inside_mask(X, Y, Z):
    """The dense path's inside test on the lattice: NOT ((x^2 + z^2) + y^2 >= 1), every fp32 operation rounded on its own."""
    x, y, z = np.meshgrid(X.astype(np.float32), Y.astype(np.float32), Z.astype(np.float32), indexing='ij')
    s = (x * x + z * z) + y * y
    assert s.dtype == np.float32
    return ~(s >= np.float32(1.0))


def block_dims(shape, B):
    return tuple((n + B - 1) // B for n in shape)


# ---------------------------------------------------------------------------------------------------- regions and the rule
def regions(X, Y, Z, B):
    """flags int32 [nbx,nby,nbz] (0 never probed, 1 wholly inside, 2 rim), probe fp32 [...,3], radius fp32 [...]: the arithmetic of
    nu_smc_regions, in float64 and in its order."""
    per_axis = []
    for A in (X, Y, Z):
        n = len(A)
        b = np.arange((n + B - 1) // B)
        lo, hi = np.maximum(B * b - 1, 0), np.minimum(B * b + B, n - 1)
        x0, x1 = A[lo].astype(np.float64), A[hi].astype(np.float64)
        per_axis.append(dict(lo=A[lo].astype(np.float32), hi=A[hi].astype(np.float32), c=0.5 * (x0 + x1), e=0.5 * (x1 - x0),
                             near=np.where(x0 > 0.0, x0, np.where(x1 < 0.0, x1, 0.0))))
    g = {k: np.meshgrid(*(a[k] for a in per_axis), indexing='ij') for k in per_axis[0]}

    def sum3(v):
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    near2, diag2, n2 = sum3(g['near']), sum3(g['e']), sum3(g['c'])
    probed = ~(near2 > 1.001)
    all_in = np.ones(near2.shape, bool)
    for e in range(8):
        x, y, z = (g['hi' if (e >> a) & 1 else 'lo'][a] for a in range(3))
        all_in &= ~((x * x + z * z) + y * y >= np.float32(1.0))
    flags = np.where(probed, np.where(all_in, 1, 2), 0).astype(np.int32)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(n2 > 0.999 * 0.999, 0.999 / np.sqrt(n2), 1.0)
    probe = np.stack([(g['c'][a] * s).astype(np.float32) for a in range(3)], -1)
    dd = [g['c'][a] - probe[..., a].astype(np.float64) for a in range(3)]
    radius = ((np.sqrt(diag2) + np.sqrt(sum3(dd))) * 1.000001).astype(np.float32)
    probe[~probed] = 0
    radius[~probed] = 0
    return flags, probe, radius


def active_rule(flags, radius, f, lipschitz, g=None, iso=0.0):
    """The rule of nu_smc_activate for the level set at iso, as a bool array: f (and g) are the probe values, shaped like flags;
    unprobed blocks are never active.  lipschitz x radius is one fp32 product and each value - iso one fp32 subtraction; of the composite (g where
    f < 0, 1 elsewhere) f keeps its comparison with 0 and g is shifted."""
    f = np.asarray(f, np.float32)
    if g is None:
        f = (f - np.float32(iso)).astype(np.float32)
    if np.isinf(lipschitz):
        return flags > 0
    lr = (np.float32(lipschitz) * radius.astype(np.float32)).astype(np.float32)
    rim = flags != 1
    if g is None:
        on = np.where(rim, f <= lr, np.abs(f) <= lr)
    else:
        g = (np.asarray(g, np.float32) - np.float32(iso)).astype(np.float32)
        g_zero = np.where(rim, g <= lr, np.abs(g) <= lr)
        on = (f <= lr) & (g_zero | ((np.abs(f) <= lr) & (g <= lr)))
    return on & (flags > 0)


def required_blocks(u, B, iso=0.0):
    """bool [nbx,nby,nbz]: the blocks that hold a corner of a cell of the dense grid u crossed by the isosurface."""
    ins = u < iso
    nx, ny, nz = u.shape
    corner = [ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    crossed = np.logical_or.reduce(corner) & ~np.logical_and.reduce(corner)
    ci, cj, ck = np.nonzero(crossed)
    need = np.zeros(block_dims(u.shape, B), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                need[(ci + dx) // B, (cj + dy) // B, (ck + dz) // B] = True
    return need, int(crossed.sum())


# ---------------------------------------------------------------------------------------------------- analytic 1-Lipschitz fields
def sphere(p, c=(0.0, 0.0, 0.0), r=0.5):
    return np.linalg.norm(p - np.asarray(c, np.float64), axis=-1) - r


def torus(p, R=0.5, r=0.2):
    return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r


FIELDS = {
    'sphere': lambda p: sphere(p),
    'torus': lambda p: torus(p),
    'clipped': lambda p: sphere(p, (0.3, 0.1, -0.2), 0.9),           # a 0.9-radius sphere that the unit ball clips
}
# (stage-1 field, inner field) of the composite: a nested pair, and a pair whose inner surface leaves the outer one
PAIRS = {
    'nested': (lambda p: sphere(p, r=0.7), lambda p: sphere(p, (0.1, 0.0, 0.0), 0.4)),
    'crossing': (lambda p: sphere(p, r=0.6), lambda p: sphere(p, (0.4, 0.0, 0.0), 0.5)),
}


def lattice(X, Y, Z):
    return np.stack(np.meshgrid(*(A.astype(np.float64) for A in (X, Y, Z)), indexing='ij'), -1)


def dense_field(field, X, Y, Z, outside_val=1.0):
    """The dense fp32 grid of an analytic field: outside_val at the points that fail the inside test."""
    u = field(lattice(X, Y, Z)).astype(np.float32)
    u[~inside_mask(X, Y, Z)] = outside_val
    return u


def dense_composite(pair, X, Y, Z):
    """extract_mesh_stage2.py:42-43 on two analytic fields: the inner one where the outer is < 0, 1 elsewhere."""
    s, g = (dense_field(f, X, Y, Z) for f in pair)
    return np.where(s < 0, g, np.float32(1.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- canonical mesh
def canonical(V, F):
    """(vertex rows as uint32 bits, sorted; face rows over the sorted DISTINCT vertices, each rotated -- orientation kept -- to its
    smallest form, sorted).  Vertices are sorted lexicographically by their bits and the faces remapped; vertices with identical
    bits (a grid value equal to the threshold puts several on one lattice point) share one index, so that the order among them
    cannot matter, and the sorted vertex rows still carry their multiplicity."""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    F = np.asarray(F, np.int64).reshape(-1, 3)
    bits = V.view(np.uint32)
    order = np.lexsort((bits[:, 2], bits[:, 1], bits[:, 0]))
    vs = bits[order]
    if len(vs) == 0:
        return vs, F
    new = np.concatenate([[True], np.any(vs[1:] != vs[:-1], axis=1)])
    ident = np.empty(len(vs), np.int64)
    ident[order] = np.cumsum(new) - 1
    G = ident[F]
    rots = np.stack([G, G[:, [1, 2, 0]], G[:, [2, 0, 1]]], 0)                    # the three rotations keep the orientation
    key = (rots[..., 0] * (len(vs) + 1) + rots[..., 1]) * (len(vs) + 1) + rots[..., 2]
    G = rots[np.argmin(key, axis=0), np.arange(len(G))]
    G = G[np.lexsort((G[:, 2], G[:, 1], G[:, 0]))]
    return vs, G


def same_mesh(a, b):
    (va, fa), (vb, fb) = canonical(*a), canonical(*b)
    return va.shape == vb.shape and fa.shape == fb.shape and np.array_equal(va, vb) and np.array_equal(fa, fb)
