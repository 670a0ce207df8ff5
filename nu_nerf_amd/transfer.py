"""Visibility transfer of a mesh: per surface point ambient occlusion, bent normal and the order-2 spherical-harmonic
transfer vector of the cosine-weighted visibility, baked once per mesh by one fused kernel (nu_transfer_bake: every hemisphere ray of a
point made, traced and reduced inside one wave; one 64-byte row per point is all that is stored).  relight.relight_splitsum(...,
transfer=...) shades with it; `python -m nu_nerf_amd.bake_transfer` writes it beside the material arrays.

Row of a point (ROW = 16 floats): [0:9] T_k, [9] ambient occlusion, [10:13] bent normal, [13:16] zero.
"""
import numpy as np

ROW = 16                        # NU_TR_ROW of csrc/relight.h
MAX_RAYS = 2 ** 31 - 1          # points x samples of one call (include/nu_nerf.h)
SH_BAND = (1.0, 2.0 / 3.0, 0.25)        # the clamped cosine lobe over pi per band: A_l / pi
SH_L = (0, 1, 1, 1, 2, 2, 2, 2, 2)


def sh_basis(dirs):
    """Order-2 real spherical harmonics float64 [...,9] of unit directions [...,3], in the order and with the constants of the header."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def unoccluded_transfer(normals):
    """The transfer vector float64 [...,9] of a point that sees the whole hemisphere about its unit normal: the closed form
    (1, 2/3, 1/4)_l Y_k(n) of the integral of (cos / pi) Y_k."""
    return sh_basis(normals) * np.asarray(SH_BAND, np.float64)[list(SH_L)]


def _seed(seed):
    seed = int(seed) & 0xffffffff
    return seed - (1 << 32) if seed >= 1 << 31 else seed


def _rows(t, dev, what):
    import torch
    t = torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).detach().to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must be [n,3], got {tuple(t.shape)}")
    return t


def _samples(samples):
    samples = int(samples)
    if samples < 16 or samples % 16:
        raise ValueError(f"samples must be a multiple of 16 and >= 16, got {samples}")
    return samples


def _geometry(V, F, scene, bvh, need_normals):
    """(LBVH, vertices, unit vertex normals or None) of a mesh, of a relight.Scene that holds them already, or of an LBVH."""
    import torch
    from .lbvh import LBVH, vertex_normals_and_curvature
    if scene is not None:
        return scene.bvh, scene.V, scene.normals
    if bvh is not None:
        return bvh, bvh.V, vertex_normals_and_curvature(bvh.V, bvh.F)[0].to(bvh.V.device).contiguous() if need_normals else None
    dev = V.device if torch.is_tensor(V) and V.is_cuda else torch.device('cuda', torch.cuda.current_device())
    V = torch.as_tensor(np.asarray(V) if not torch.is_tensor(V) else V).to(device=dev, dtype=torch.float32).contiguous()
    F = torch.as_tensor(np.asarray(F) if not torch.is_tensor(F) else F).to(device=dev, dtype=torch.int32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"mesh must be V [Nv,3], F [Nf,3], got {tuple(V.shape)} {tuple(F.shape)}")
    return LBVH(V, F), V, vertex_normals_and_curvature(V, F)[0].to(dev).contiguous() if need_normals else None


def bake_transfer(V, F, samples=1024, seed=0, eps=None, radius=None, points=None, normals=None, chunk=None, scene=None, bvh=None,
                  id0=0, dump=False):
    """float32 [n,16] transfer rows on the device, of the mesh's vertices under their angle-weighted normals or of `points` [n,3] with
    UNIT `normals` [n,3] (e.g. render_surface hits).  samples: hemisphere rays per point, a multiple of 16; eps: the ray origin is
    p + eps n (default relight.ORIGIN_EPS); radius: occluders farther than this do not count (default: unbounded).  Point i is sampled
    as point id0 + i; `chunk` points go to one launch, and the result does not depend on it, bit for bit.  scene: a relight.Scene
    whose tree and normals are used instead of building them; bvh: an LBVH for V, F.  dump=True returns (rows, vis uint8 [n,samples])
    from the test entry."""
    import torch
    from . import _lib as L
    from .relight import ORIGIN_EPS
    samples = _samples(samples)
    if (points is None) != (normals is None):
        raise ValueError("points and normals come together")
    tree, Vd, Nd = _geometry(V, F, scene, bvh, points is None)
    dev = Vd.device
    if points is None:
        P, N = Vd, Nd
    else:
        P, N = _rows(points, dev, 'points'), _rows(normals, dev, 'normals')
        if P.shape != N.shape:
            raise ValueError(f"points {tuple(P.shape)} and normals {tuple(N.shape)} differ in shape")
    n = int(P.shape[0])
    per = MAX_RAYS // samples
    chunk = per if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    chunk = min(chunk, per)
    eps = ORIGIN_EPS if eps is None else float(eps)
    radius = 1e16 if radius is None else float(radius)
    out = torch.empty(n, ROW, dtype=torch.float32, device=dev)
    vis = torch.empty(n, samples, dtype=torch.uint8, device=dev) if dump else None
    lib = L.load()
    for i0 in range(0, max(n, 1), chunk):
        ni = min(chunk, n - i0)
        args = (L.ptr(tree.buf), tree.n_faces, L.ptr(P[i0:i0 + ni]), L.ptr(N[i0:i0 + ni]), ni, int(id0) + i0, samples, _seed(seed), eps,
                radius, L.ptr(out[i0:i0 + ni]))
        if dump:
            lib.nu_transfer_bake_dump(*args, L.ptr(vis[i0:i0 + ni]), L.stream())
        else:
            lib.nu_transfer_bake(*args, L.stream())
    return (out, vis) if dump else out


def transfer_rays(points, normals, samples, seed=0, eps=None, id0=0):
    """(rays float32 [n * samples, 6], bits int32 [n * samples, 2]): the rays bake_transfer traces and the two 24-bit sample integers
    behind each (tests)."""
    import torch
    from . import _lib as L
    from .relight import ORIGIN_EPS
    L.require_cuda(points, normals)
    P, N = _rows(points, points.device, 'points'), _rows(normals, points.device, 'normals')
    n, samples = int(P.shape[0]), int(samples)
    total = max(n * samples, 0) if n * samples <= MAX_RAYS else 0
    rays = torch.empty(total, 6, dtype=torch.float32, device=P.device)
    bits = torch.empty(total, 2, dtype=torch.int32, device=P.device)
    L.load().nu_transfer_rays(L.ptr(P), L.ptr(N), n, int(id0), samples, _seed(seed), ORIGIN_EPS if eps is None else float(eps),
                              L.ptr(rays), L.ptr(bits), L.stream())
    return rays, bits


def split_rows(rows):
    """{'transfer' [n,9], 'ao' [n,1], 'bent_normal' [n,3]} float32 numpy arrays of transfer rows [n,16]: the files bake_transfer writes."""
    r = np.asarray(rows.detach().cpu() if hasattr(rows, 'detach') else rows, np.float32)
    if r.ndim != 2 or r.shape[1] != ROW:
        raise ValueError(f"transfer rows must be [n,{ROW}], got {r.shape}")
    return {'transfer': np.ascontiguousarray(r[:, 0:9]), 'ao': np.ascontiguousarray(r[:, 9:10]),
            'bent_normal': np.ascontiguousarray(r[:, 10:13])}


def join_rows(transfer, ao, bent_normal):
    """float32 [n,16] rows from the three arrays of split_rows."""
    t = np.asarray(transfer, np.float32)
    n = t.shape[0] if t.ndim == 2 else -1
    a, b = np.asarray(ao, np.float32), np.asarray(bent_normal, np.float32)
    if t.shape != (n, 9) or a.shape not in ((n,), (n, 1)) or b.shape != (n, 3):
        raise ValueError(f"expected transfer [n,9], ao [n,1], bent_normal [n,3], got {t.shape} {a.shape} {b.shape}")
    if not (np.isfinite(t).all() and np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("transfer arrays must be finite")
    return np.ascontiguousarray(np.concatenate([t, a.reshape(n, 1), b, np.zeros((n, 3), np.float32)], 1))


FILES = ('transfer', 'ao', 'bent_normal')


def save_transfer_dir(directory, rows):
    """Write transfer.npy [Nv,9], ao.npy [Nv,1], bent_normal.npy [Nv,3] into `directory`; -> {name: path}."""
    import os
    os.makedirs(directory, exist_ok=True)
    paths = {}
    for k, a in split_rows(rows).items():
        paths[k] = os.path.join(directory, k + '.npy')
        np.save(paths[k], a)
    return paths


def load_transfer_dir(directory, n_verts=None):
    """float32 [Nv,16] rows from a directory as save_transfer_dir writes it."""
    import os
    rows = join_rows(*(np.load(os.path.join(directory, k + '.npy')) for k in FILES))
    if n_verts is not None and rows.shape[0] != n_verts:
        raise ValueError(f"{directory}: transfer of {rows.shape[0]} vertices for a mesh of {n_verts}")
    return rows


def pack_env_sh(env_sh):
    """float32 [9,4] (RGB + pad) from SH coefficients [9,3] of an environment (environment.project_sh)."""
    e = np.asarray(env_sh, np.float64)
    if e.shape != (9, 3) or not np.isfinite(e).all():
        raise ValueError(f"env_sh must be finite [9,3], got {e.shape}")
    return np.ascontiguousarray(np.concatenate([e, np.zeros((9, 1))], 1).astype(np.float32))

