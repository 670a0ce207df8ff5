"""Texture-atlas material baking: the relightable asset with materials in a texture instead of per vertex, and the
files other tools open -- PNG textures, OBJ + MTL, glTF 2.0.

The parametrisation is trivial on purpose: no chart search, every face gets its own right triangle, two faces to a square cell, in file
order (atlas_layout).  A texel holds the material at EXTRAPOLATED barycentrics of its face, so a face's values are affine across all the
texels it owns and a bilinear lookup anywhere in its triangle -- corners and edges included -- reads only texels of that face.
csrc/texture.hip has the three kernels: nu_atlas_texels (texel -> surface point), nu_atlas_sample (the lookup) and nu_atlas_gbuffer
(lookup at the hit points of a G-buffer, into its material columns); materials.bake_materials evaluates the networks at the texel points.
Opt-in: normals='sdf' also bakes the SDF's unit normal at every texel (curvature.bake_normals) into the spare lanes of the
atlas; nu_atlas_sample_normal / nu_atlas_gbuffer_normal look it up, relight takes it as the shading normal (normal_map=True), and
write_gltf exports it as a tangent-space normalTexture in per-face flat frames.

    atlas = bake_textures(renderer, V, F, size=2048)            # device tensors + layout
    write_textures(directory, atlas)                             # atlas.npz, albedo.png, orm.png
    write_gltf(directory + '/mesh.gltf', V, F, atlas['uv'], normals, directory)
    relight.relight_splitsum_linear(scene, ..., texture=atlas)   # every resolve runs unchanged on the textured G-buffer
"""
import json
import os

import numpy as np

CH = 5                          # NU_ATLAS_CH: albedo rgb, metallic, roughness
MAX_SIZE = 32768                # NU_ATLAS_MAX_SIZE
MAX_PAD = 64                    # NU_ATLAS_MAX_PAD
PASS_TEXELS = 1 << 22           # texels of one bake_textures pass by default: 64 MB of texel points


# ---- the layout (host) -------------------------------------------------------------------------------------------------------------------
def atlas_layout(n_faces, size, pad=0):
    """The atlas of `n_faces` faces in a square of `size` = T texels a side: dict(size, n_faces, pad, cols, cell, L).
    cols = ceil(sqrt(ceil(n_faces / 2))) cells a side, cell = c = T // cols texels, L = c - 3 - 3 pad the leg of a face's triangle in
    texels.  Face f sits in cell k = f >> 1 at origin (k % cols, k // cols) c; cell-local, the lower face (f even) has vertices 0, 1, 2
    at (pad, pad), (pad + L, pad), (pad, pad + L) and owns the texels i + j <= c - 2, the upper face is the point mirror
    (s, t) -> (c - 1 - s, c - 1 - t) and owns i + j >= c; the diagonal belongs to nobody.  L < 2 is a ValueError naming the smallest T."""
    n_faces, size, pad = int(n_faces), int(size), int(pad)
    if n_faces < 1:
        raise ValueError(f"atlas_layout: n_faces must be >= 1, got {n_faces}")
    if not 0 <= pad <= MAX_PAD:
        raise ValueError(f"atlas_layout: pad must be in 0..{MAX_PAD}, got {pad}")
    cells = (n_faces + 1) // 2
    cols = int(np.ceil(np.sqrt(cells)))
    while cols * cols < cells:
        cols += 1
    while cols > 1 and (cols - 1) * (cols - 1) >= cells:
        cols -= 1
    smallest = cols * (5 + 3 * pad)
    if size < smallest:
        raise ValueError(f"atlas_layout: {n_faces} faces with pad {pad} do not fit {size} x {size} texels ({cols} x {cols} cells of "
                         f"{size // cols if size > 0 else 0}): the smallest size that works is {smallest}")
    if size > MAX_SIZE:
        raise ValueError(f"atlas_layout: size must be <= {MAX_SIZE}, got {size}")
    c = size // cols
    return {'size': size, 'n_faces': n_faces, 'pad': pad, 'cols': cols, 'cell': c, 'L': c - 3 - 3 * pad}


def _check_layout(layout):
    """A layout dict is what atlas_layout makes of its three numbers, nothing else."""
    want = atlas_layout(layout['n_faces'], layout['size'], layout['pad'])
    if any(int(layout.get(k, -1)) != v for k, v in want.items()):
        raise ValueError(f"not an atlas_layout: {layout}")
    return want


def atlas_corners(layout):
    """Texel coordinates float64 [Nf,3,2] = (x, y) of the three vertices of every face (texel (i, j) is at (i, j); y is the array row)."""
    lay = _check_layout(layout)
    c, pad, L, cols = lay['cell'], lay['pad'], lay['L'], lay['cols']
    f = np.arange(lay['n_faces'])
    k, h = f >> 1, f & 1
    origin = np.stack([(k % cols) * c, (k // cols) * c], -1).astype(np.float64)
    local = np.asarray([[pad, pad], [pad + L, pad], [pad, pad + L]], np.float64)
    st = np.where(h[:, None, None] == 1, (c - 1) - local[None], local[None])
    return origin[:, None, :] + st


def atlas_uv(layout, F=None):
    """UV coordinates float32 [Nf,3,2] of the three corners of every face: ((x + 0.5) / T, (y + 0.5) / T), y the array row -- glTF's
    convention (OBJ takes 1 - v).  F, if given, is only checked against the layout's face count."""
    if F is not None and len(F) != int(layout['n_faces']):
        raise ValueError(f"atlas_uv: {len(F)} faces for a layout of {layout['n_faces']}")
    return ((atlas_corners(layout) + 0.5) / float(layout['size'])).astype(np.float32)


# ---- device passes -----------------------------------------------------------------------------------------------------------------------
def _mesh_on_device(V, F, device=None):
    import torch
    dev = torch.device(device) if device is not None else (V.device if torch.is_tensor(V) and V.is_cuda
                                                           else torch.device('cuda', torch.cuda.current_device()))
    V = torch.as_tensor(np.asarray(V) if not torch.is_tensor(V) else V).detach().to(device=dev, dtype=torch.float32).contiguous()
    F = torch.as_tensor(np.asarray(F) if not torch.is_tensor(F) else F).detach().to(device=dev, dtype=torch.int32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3 or V.shape[0] < 1:
        raise ValueError(f"mesh must be V [Nv,3], F [Nf,3], got {tuple(V.shape)} {tuple(F.shape)}")
    return V, F


def atlas_texels(V, F, layout, vnormals=None, y0=0, rows=None):
    """The device pass over rows [y0, y0 + rows) of the atlas -> (points float32 [rows,T,3], face int32 [rows,T], normals float32
    [rows,T,3] or None): the surface point of every owned texel (zero where unowned), the owning face (-1 where unowned) and, with
    `vnormals` [Nv,3] (unit), the renormalised mix of the vertex normals.  The first two are views of one [rows,T,4] tensor (the
    kernel stores point and face id together); a texel's bits do not depend on the row chunking."""
    import torch
    from . import _lib as L
    lay = _check_layout(layout)
    T = lay['size']
    V, F = _mesh_on_device(V, F)
    if int(F.shape[0]) != lay['n_faces']:
        raise ValueError(f"atlas_texels: {int(F.shape[0])} faces for a layout of {lay['n_faces']}")
    rows = T - int(y0) if rows is None else int(rows)
    if y0 < 0 or rows < 0 or y0 + rows > T:
        raise ValueError(f"atlas_texels: rows [{y0}, {y0 + rows}) are not inside the atlas of {T}")
    texel = torch.empty(rows, T, 4, dtype=torch.float32, device=V.device)
    normal = None
    if vnormals is not None:
        vnormals = torch.as_tensor(np.asarray(vnormals) if not torch.is_tensor(vnormals) else vnormals).detach().to(
            device=V.device, dtype=torch.float32).contiguous()
        if tuple(vnormals.shape) != tuple(V.shape):
            raise ValueError(f"atlas_texels: vnormals {tuple(vnormals.shape)} for vertices {tuple(V.shape)}")
        normal = torch.empty(rows, T, 4, dtype=torch.float32, device=V.device)
    L.load().nu_atlas_texels(L.ptr(V), int(V.shape[0]), L.ptr(F), lay['n_faces'], L.ptr(vnormals), T, lay['pad'], int(y0), rows,
                             L.ptr(texel), L.ptr(normal), L.stream())
    return texel[..., :3], texel.view(torch.int32)[..., 3], (None if normal is None else normal[..., :3])


def _normals_arg(normals):
    if normals not in (None, 'sdf'):
        raise ValueError(f"normals must be None or 'sdf', got {normals!r}")
    return normals is not None


def bake_textures(renderer, V, F, size=2048, pad=0, which=None, rows_per_pass=None, normals=None):
    """The material networks of `renderer` baked into an atlas of `size` texels a side for the mesh (V, F): dict of device tensors
    'albedo' [T,T,3], 'metallic' [T,T], 'roughness' [T,T] (float32, 0 where no face owns the texel), 'face' [T,T] int32 (-1 where
    unowned), plus 'uv' float32 numpy [Nf,3,2] (atlas_uv) and 'layout'.  Texel points come from nu_atlas_texels in passes of
    `rows_per_pass` rows (default: PASS_TEXELS texels), the owned ones are selected (one host read per pass, the count) and evaluated
    by materials.bake_materials -- the fused bake kernel, `which` as there; the result does not depend on rows_per_pass, bit for bit.
    normals='sdf' adds 'normal' float32 [T,T,3]: the SDF's unit normal grad f / |grad f| at the same selected texel
    points (curvature.bake_normals, one more launch per pass), zero where unowned.  It is the raw object-space normal -- it points
    where f grows; nothing is flipped here -- and every other key is what normals=None returns."""
    import torch
    from .materials import bake_engine, bake_materials
    want_normals = _normals_arg(normals)
    V, F = _mesh_on_device(V, F, bake_engine(renderer, which).dev)
    lay = atlas_layout(int(F.shape[0]), size, pad)
    T = lay['size']
    rows_per_pass = max(1, PASS_TEXELS // T) if rows_per_pass is None else int(rows_per_pass)
    if rows_per_pass < 1:
        raise ValueError("rows_per_pass must be >= 1")
    dev = V.device
    five = torch.zeros(T * T, CH, dtype=torch.float32, device=dev)
    face = torch.empty(T, T, dtype=torch.int32, device=dev)
    normal = torch.zeros(T * T, 3, dtype=torch.float32, device=dev) if want_normals else None
    for y0 in range(0, T, rows_per_pass):
        nr = min(rows_per_pass, T - y0)
        points, ids, _ = atlas_texels(V, F, lay, y0=y0, rows=nr)
        face[y0:y0 + nr] = ids
        sel = (ids.reshape(-1) >= 0).nonzero().flatten()
        if sel.numel() == 0:
            continue
        owned = points.reshape(-1, 3)[sel].contiguous()
        out = bake_materials(renderer, owned, which=which)
        five[y0 * T + sel] = torch.cat([out['albedo'], out['metallic'], out['roughness']], 1)
        if want_normals:
            from .curvature import bake_normals
            normal[y0 * T + sel] = bake_normals(renderer, owned, which=which)['normal']
    five = five.reshape(T, T, CH)
    atlas = {'albedo': five[..., 0:3].contiguous(), 'metallic': five[..., 3].contiguous(), 'roughness': five[..., 4].contiguous(),
             'face': face, 'uv': atlas_uv(lay), 'layout': lay}
    if want_normals:
        atlas['normal'] = normal.reshape(T, T, 3)
    return atlas


class PackedAtlas:
    """The device texture of the lookup kernels: tex float32 [2,T,T,4] = (albedo rgb, metallic), (roughness, normal xyz), + layout.
    has_normal: the atlas came with 'normal'; without it the three normal lanes are zero."""

    def __init__(self, tex, layout, has_normal=False):
        self.tex, self.layout, self.has_normal = tex, layout, bool(has_normal)
        self.size, self.n_faces, self.pad = layout['size'], layout['n_faces'], layout['pad']
        self.device = tex.device


def pack_atlas(atlas, layout=None, device=None):
    """PackedAtlas from what bake_textures returns or load_textures reads (a dict with 'albedo' [T,T,3], 'metallic', 'roughness' [T,T]
    and 'layout'), or from one [T,T,5] array (albedo, metallic, roughness) with `layout`.  Arrays may be numpy or tensors.  A dict's
    'normal' [T,T,3] (bake_textures(normals='sdf')) goes into lanes y, z, w of plane 1."""
    import torch
    if isinstance(atlas, PackedAtlas):
        return atlas
    dev = torch.device(device) if device is not None else None
    t = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(torch.float32)      # noqa: E731
    normal = None
    if isinstance(atlas, dict):
        layout = atlas['layout'] if layout is None else layout
        normal = atlas.get('normal')
        al, me, ro = t(atlas['albedo']), t(atlas['metallic']), t(atlas['roughness'])
        if dev is None:
            dev = al.device if al.is_cuda else torch.device('cuda', torch.cuda.current_device())
        T = int(al.shape[0])
        five = torch.cat([al.to(dev).reshape(T, -1, 3), me.to(dev).reshape(T, -1, 1), ro.to(dev).reshape(T, -1, 1)], -1)
    else:
        five = t(atlas)
        five = five.to(dev if dev is not None else (five.device if five.is_cuda else torch.device('cuda', torch.cuda.current_device())))
    if layout is None:
        raise ValueError("pack_atlas: a bare array needs its layout")
    lay = _check_layout(layout)
    T = lay['size']
    if tuple(five.shape) != (T, T, CH):
        raise ValueError(f"pack_atlas: expected [{T},{T},{CH}] values for this layout, got {tuple(five.shape)}")
    tex = torch.zeros(2, T, T, 4, dtype=torch.float32, device=five.device)
    tex[0] = five[..., :4]
    tex[1, ..., 0] = five[..., 4]
    if normal is not None:
        normal = t(normal).to(five.device)
        if tuple(normal.shape) != (T, T, 3):
            raise ValueError(f"pack_atlas: expected [{T},{T},3] normals for this layout, got {tuple(normal.shape)}")
        tex[1, ..., 1:4] = normal
    return PackedAtlas(tex, lay, normal is not None)


def sample_atlas(atlas, face, uv):
    """float32 [N,5] (albedo, metallic, roughness) on the device: the bilinear lookup at barycentrics uv [N,2] = (u, v), the weights of
    vertices 1 and 2, of face [N] (int32).  (u, v) is clamped into the triangle; a face id outside the atlas gives zeros."""
    import torch
    from . import _lib as L
    atlas = pack_atlas(atlas)
    t = lambda a, dt: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(device=atlas.device, dtype=dt).contiguous()  # noqa: E731
    face, uv = t(face, torch.int32).reshape(-1), t(uv, torch.float32)
    if uv.dim() != 2 or uv.shape[1] != 2 or uv.shape[0] != face.shape[0]:
        raise ValueError(f"sample_atlas: face [N] and uv [N,2] expected, got {tuple(face.shape)} {tuple(uv.shape)}")
    out = torch.empty(int(face.shape[0]), CH, dtype=torch.float32, device=atlas.device)
    L.load().nu_atlas_sample(L.ptr(atlas.tex), atlas.size, atlas.n_faces, atlas.pad, L.ptr(face), L.ptr(uv), int(face.shape[0]), L.ptr(out),
                             L.stream())
    return out


def sample_atlas_normal(atlas, face, uv):
    """float32 [N,3] on the device: sample_atlas's lookup on the atlas's normal lanes, divided by its length (nu_atlas_sample_normal);
    zero where the mix has no length in (0, 1e30) -- an atlas without normals, a zero texel -- and for a face id outside the atlas."""
    import torch
    from . import _lib as L
    atlas = pack_atlas(atlas)
    t = lambda a, dt: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(device=atlas.device, dtype=dt).contiguous()  # noqa: E731
    face, uv = t(face, torch.int32).reshape(-1), t(uv, torch.float32)
    if uv.dim() != 2 or uv.shape[1] != 2 or uv.shape[0] != face.shape[0]:
        raise ValueError(f"sample_atlas_normal: face [N] and uv [N,2] expected, got {tuple(face.shape)} {tuple(uv.shape)}")
    out = torch.empty(int(face.shape[0]), 3, dtype=torch.float32, device=atlas.device)
    L.load().nu_atlas_sample_normal(L.ptr(atlas.tex), atlas.size, atlas.n_faces, atlas.pad, L.ptr(face), L.ptr(uv), int(face.shape[0]),
                                    L.ptr(out), L.stream())
    return out


def texture_gbuffer(scene, face, gbuf, pix, atlas, normals=False):
    """Overwrite the material columns (10..14: albedo, metallic, roughness) of the listed hit rows of a G-buffer of relight.gbuffer(scene,
    ...) with the atlas's values at the stored hit points, in place; every other column and every unlisted row stays.  -> gbuf.
    normals=True: the shading normal (columns 7..9) of those rows is also replaced by the atlas's normal at the hit point,
    put on the side of the geometric normal (nu_atlas_gbuffer_normal); a row whose lookup has no length keeps its own.  ValueError for
    an atlas without normals."""
    from . import _lib as L
    if not isinstance(atlas, PackedAtlas):
        raise TypeError("texture_gbuffer takes a PackedAtlas (pack_atlas)")
    if normals and not atlas.has_normal:
        raise ValueError("texture_gbuffer: normals=True needs an atlas with 'normal' (bake_textures(normals='sdf'))")
    if atlas.n_faces != int(scene.F.shape[0]):
        raise ValueError(f"the atlas is laid out for {atlas.n_faces} faces, the scene's mesh has {int(scene.F.shape[0])}")
    import torch
    if atlas.device != gbuf.device or not (gbuf.is_contiguous() and face.is_contiguous() and pix.is_contiguous()) \
            or (gbuf.dtype, face.dtype, pix.dtype) != (torch.float32, torch.int32, torch.int32) or gbuf.numel() != face.numel() * 20:
        raise ValueError("texture_gbuffer: gbuf [*,20] float32, face [*] and pix int32 must be contiguous tensors on the atlas's device")
    L.load().nu_atlas_gbuffer(L.ptr(gbuf), L.ptr(face), L.ptr(pix), int(pix.shape[0]), L.ptr(scene.V), int(scene.V.shape[0]), L.ptr(scene.F),
                              atlas.n_faces, L.ptr(atlas.tex), atlas.size, atlas.pad, L.stream())
    if normals:
        L.load().nu_atlas_gbuffer_normal(L.ptr(gbuf), L.ptr(face), L.ptr(pix), int(pix.shape[0]), L.ptr(scene.V), int(scene.V.shape[0]),
                                         L.ptr(scene.F), atlas.n_faces, L.ptr(atlas.tex), atlas.size, atlas.pad, L.stream())
    return gbuf


def predict_textures(renderer, mesh=None, size=2048, which=None, pad=0, normals=None):
    """bake_textures for the mesh predict_materials reads (None: data/meshes/{name}-300000.ply; a PLY path or a (V, F) pair), as float32 /
    int32 numpy arrays: {'albedo' [T,T,3], 'metallic' [T,T], 'roughness' [T,T], 'face' [T,T], 'uv' [Nf,3,2], 'layout'}, with
    normals='sdf' also 'normal' [T,T,3]."""
    import torch
    if mesh is None:
        mesh = os.path.join('data', 'meshes', f"{renderer.cfg['name']}-300000.ply")
    if isinstance(mesh, (str, os.PathLike)):
        from .mesh import read_ply
        mesh = read_ply(mesh)
    atlas = bake_textures(renderer, mesh[0], mesh[1], size=size, pad=pad, which=which, normals=normals)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in atlas.items()}


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def srgb8(linear):
    """uint8 from linear values by relight.to_srgb8's rule: 323/25 x up to 0.0031308, (211 max(x, eps)^(5/12) - 11) / 200 above, clipped
    to [0, 1], floor(255 x + 0.5)."""
    x = np.asarray(linear, np.float32)
    eps = np.finfo(np.float32).eps
    s = np.where(x <= np.float32(0.0031308), np.float32(323 / 25) * x,
                 (np.float32(211) * np.maximum(x, eps) ** np.float32(5 / 12) - np.float32(11)) / np.float32(200)).astype(np.float32)
    return np.floor(np.clip(s, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def linear8(x):
    """uint8 floor(255 x + 0.5) of values clipped to [0, 1]."""
    return np.floor(np.clip(np.asarray(x, np.float32), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def texture_images(atlas):
    """(albedo uint8 [T,T,3] sRGB-encoded, orm uint8 [T,T,3] linear with R = 255, G = roughness, B = metallic): the two PNGs' pixels."""
    rough, metal = linear8(_np(atlas['roughness'])), linear8(_np(atlas['metallic']))
    return srgb8(_np(atlas['albedo'])), np.stack([np.full_like(rough, 255), rough, metal], -1)


def write_textures(directory, atlas):
    """Write DIR/atlas.npz (albedo, metallic, roughness float32, face int32, uv, and the layout numbers size, n_faces, pad),
    DIR/albedo.png (8-bit sRGB) and DIR/orm.png (8-bit linear: R = 255, no occlusion channel; G = roughness; B = metallic -- glTF's
    metallicRoughnessTexture).  -> {name: path}."""
    from .mask_render import _pillow
    os.makedirs(directory, exist_ok=True)
    lay = _check_layout(atlas['layout'])
    paths = {k: os.path.join(directory, k) for k in ('atlas.npz', 'albedo.png', 'orm.png')}
    extra = {'normal': _np(atlas['normal']).astype(np.float32)} if atlas.get('normal') is not None else {}
    np.savez(paths['atlas.npz'], albedo=_np(atlas['albedo']).astype(np.float32), metallic=_np(atlas['metallic']).astype(np.float32),
             roughness=_np(atlas['roughness']).astype(np.float32), face=_np(atlas['face']).astype(np.int32),
             uv=np.asarray(atlas['uv'], np.float32), size=lay['size'], n_faces=lay['n_faces'], pad=lay['pad'], **extra)
    albedo, orm = texture_images(atlas)
    _pillow().fromarray(albedo, 'RGB').save(paths['albedo.png'])
    _pillow().fromarray(orm, 'RGB').save(paths['orm.png'])
    return paths


def load_textures(directory, n_faces=None):
    """The atlas dict (numpy arrays + 'layout') of a directory write_textures wrote (atlas.npz)."""
    path = os.path.join(directory, 'atlas.npz')
    with np.load(path) as z:
        lay = atlas_layout(int(z['n_faces']), int(z['size']), int(z['pad']))
        atlas = {k: np.ascontiguousarray(z[k]) for k in ('albedo', 'metallic', 'roughness', 'face', 'uv')}
        if 'normal' in z.files:
            atlas['normal'] = np.ascontiguousarray(z['normal'])
    T = lay['size']
    if atlas['albedo'].shape != (T, T, 3) or atlas['metallic'].shape != (T, T) or atlas['roughness'].shape != (T, T) \
            or atlas.get('normal', atlas['albedo']).shape != (T, T, 3):
        raise ValueError(f"{path}: arrays do not have the atlas's size {T}")
    if n_faces is not None and lay['n_faces'] != n_faces:
        raise ValueError(f"{path}: atlas of {lay['n_faces']} faces for a mesh of {n_faces}")
    atlas['layout'] = lay
    return atlas


def tangent_frames(V, F):
    """The flat tangent frame of every face, float64 (Tn, B, N) [Nf,3] each, and `flat` bool [Nf] (faces of zero area).  With
    e1 = v1 - v0, e2 = v2 - v0: N = unit(e1 x e2); Tn = unit(e1) for an even face (the lower one of its atlas cell, where +u runs
    v0 -> v1) and -unit(e1) for an odd one (the point-mirrored frame); B = N x Tn.  The handedness is +1 for both -- the mirror is a
    rotation by 180 degrees, not a reflection.  A face of zero area gets N = (0,0,1), Tn = (1,0,0)."""
    V, F = np.asarray(_np(V), np.float64).reshape(-1, 3), np.asarray(_np(F), np.int64).reshape(-1, 3)
    e1, e2 = V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    n = np.cross(e1, e2)
    ln, l1 = np.linalg.norm(n, axis=1), np.linalg.norm(e1, axis=1)
    flat = ~((ln > 0.0) & (l1 > 0.0))
    safe = lambda a, l: a / np.where(flat, 1.0, l)[:, None]      # noqa: E731
    sign = np.where(np.arange(len(F)) & 1, -1.0, 1.0)[:, None]
    N = np.where(flat[:, None], np.asarray([0.0, 0.0, 1.0]), safe(n, ln))
    Tn = np.where(flat[:, None], np.asarray([1.0, 0.0, 0.0]), sign * safe(e1, l1))
    return Tn, np.cross(N, Tn), N, flat


def tangent_normal_image(atlas, V, F, count=False):
    """uint8 [T,T,3]: the tangent-space normal map of an atlas with 'normal' (object space) for the mesh (V, F), in the flat frames of
    tangent_frames (host, float64).  Pixel = floor(255 clip(0.5 (n.Tn, n.B, n.N) + 0.5, 0, 1) + 0.5) with the frame of the texel's face
    (atlas['face']); unowned texels and the texels of zero-area faces are (128, 128, 255), the unperturbed normal.  count=True: ->
    (image, normal_backfacing), the number of owned texels with n.N <= 0 -- normals that face away from their own face (a mesh far from the zero set, or wound the
    other way round than f grows): they are encoded as they are, and a viewer lights them from behind."""
    if atlas.get('normal') is None:
        raise ValueError("tangent_normal_image: the atlas has no 'normal' (bake_textures(normals='sdf'))")
    face, n = np.asarray(_np(atlas['face']), np.int64), np.asarray(_np(atlas['normal']), np.float64)
    Tn, B, N, flat = tangent_frames(V, F)
    if n.shape != face.shape + (3,) or (face.size and face.max() >= len(Tn)):
        raise ValueError(f"tangent_normal_image: normal {n.shape}, face {face.shape} for a mesh of {len(Tn)} faces")
    f = np.maximum(face, 0)
    own = (face >= 0) & ~flat[f]
    c = np.stack([(n * Tn[f]).sum(-1), (n * B[f]).sum(-1), (n * N[f]).sum(-1)], -1)
    img = np.floor(255.0 * np.clip(0.5 * c + 0.5, 0.0, 1.0) + 0.5).astype(np.uint8)
    img[~own] = (128, 128, 255)
    return (img, int(np.count_nonzero(own & (c[..., 2] <= 0.0)))) if count else img


def _unwelded(V, F, uv, normals):
    """(positions [3 Nf,3], normals [3 Nf,3], uv [3 Nf,2]) float32: one vertex per face corner."""
    V, F = np.asarray(_np(V), np.float32).reshape(-1, 3), np.asarray(_np(F), np.int64).reshape(-1, 3)
    uv, normals = np.asarray(uv, np.float32), np.asarray(_np(normals), np.float32)
    if uv.shape != (len(F), 3, 2):
        raise ValueError(f"uv must be [{len(F)},3,2] (atlas_uv), got {uv.shape}")
    if normals.shape != V.shape:
        raise ValueError(f"normals must be per vertex {V.shape}, got {normals.shape}")
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError("face index out of range")
    return np.ascontiguousarray(V[F.reshape(-1)]), np.ascontiguousarray(normals[F.reshape(-1)]), np.ascontiguousarray(uv.reshape(-1, 2))


def write_obj(path, V, F, uv, normals, directory=None):
    """Wavefront OBJ with `vt` = (u, 1 - v) and `vn` per face corner, plus PATH's .mtl naming the textures of `directory` (default: the
    OBJ's own) relative to the OBJ: map_Kd albedo.png, map_Pr / map_Pm orm.png (the PBR extension; readers take the channel they know)."""
    path = str(path)
    P, N, T2 = _unwelded(V, F, uv, normals)
    base = os.path.dirname(os.path.abspath(path))
    rel = os.path.relpath(os.path.abspath(directory), base) if directory is not None else '.'
    tex = lambda name: name if rel == '.' else (rel + '/' + name).replace(os.sep, '/')      # noqa: E731
    mtl = os.path.splitext(path)[0] + '.mtl'
    with open(mtl, 'w') as fh:
        fh.write("newmtl baked\nKd 1 1 1\nPr 1\nPm 1\n"
                 f"map_Kd {tex('albedo.png')}\nmap_Pr {tex('orm.png')}\nmap_Pm {tex('orm.png')}\n")
    Vn, Fn = np.asarray(_np(V), np.float32).reshape(-1, 3), np.asarray(_np(F), np.int64).reshape(-1, 3)
    with open(path, 'w') as fh:
        fh.write(f"mtllib {os.path.basename(mtl)}\n")
        fh.write(''.join(f"v {float(a)!r} {float(b)!r} {float(c)!r}\n" for a, b, c in Vn))
        fh.write(''.join(f"vt {float(u)!r} {float(np.float32(1.0) - v)!r}\n" for u, v in T2))
        fh.write(''.join(f"vn {float(a)!r} {float(b)!r} {float(c)!r}\n" for a, b, c in N))
        fh.write("usemtl baked\n")
        fh.write(''.join(f"f {a + 1}/{3 * i + 1}/{3 * i + 1} {b + 1}/{3 * i + 2}/{3 * i + 2} {c + 1}/{3 * i + 3}/{3 * i + 3}\n"
                         for i, (a, b, c) in enumerate(Fn)))
    return path, mtl


def write_gltf(path, V, F, uv, normals, directory=None, normal_map=None):
    """glTF 2.0: PATH (.gltf, JSON) + PATH's .bin.  Vertices are unwelded (3 Nf of them, no index buffer): POSITION, NORMAL and
    TEXCOORD_0 accessors with min / max; one material with baseColorTexture = albedo.png and metallicRoughnessTexture = orm.png of
    `directory` (default: the file's own), referenced by relative URI, both factors 1; the sampler is LINEAR / LINEAR without mip
    filter (the atlas's gutter is sized for bilinear taps) and CLAMP_TO_EDGE.
    normal_map: an atlas dict with 'normal' (None: the file above, byte for byte).  Its tangent-space image
    (tangent_normal_image) is written as normal.png beside the other textures and named as the material's normalTexture (scale 1); every
    face corner then carries NORMAL = the face's flat normal instead of the vertex normal, and a TANGENT accessor (VEC4) holds (Tn, 1) of
    tangent_frames.  The frame is constant per face and in the file, so bitangent = cross(NORMAL, TANGENT.xyz) TANGENT.w gives back the
    baked object-space normal whatever the viewer's tangent generator or interpolation."""
    path = str(path)
    P, N, T2 = _unwelded(V, F, uv, normals)
    base = os.path.dirname(os.path.abspath(path))
    rel = os.path.relpath(os.path.abspath(directory), base) if directory is not None else '.'
    tex = lambda name: name if rel == '.' else (rel + '/' + name).replace(os.sep, '/')      # noqa: E731
    bin_path = os.path.splitext(path)[0] + '.bin'
    tangent = None
    if normal_map is not None:
        from .mask_render import _pillow
        image = tangent_normal_image(normal_map, V, F)
        Tn, _, Nf, _ = tangent_frames(V, F)
        N = np.ascontiguousarray(np.repeat(Nf, 3, axis=0), np.float32)
        tangent = np.ascontiguousarray(np.repeat(np.concatenate([Tn, np.ones((len(Tn), 1))], 1), 3, axis=0), np.float32)
        os.makedirs(base if directory is None else directory, exist_ok=True)
        _pillow().fromarray(image, 'RGB').save(os.path.join(base if directory is None else directory, 'normal.png'))
    blobs = [P.astype('<f4').tobytes(), N.astype('<f4').tobytes(), T2.astype('<f4').tobytes()]
    if tangent is not None:
        blobs.append(tangent.astype('<f4').tobytes())
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).tolist()
    with open(bin_path, 'wb') as fh:
        for b in blobs:
            fh.write(b)
    n = int(P.shape[0])
    bounds = lambda a: {'min': [float(x) for x in a.min(0)], 'max': [float(x) for x in a.max(0)]} if n else {}      # noqa: E731
    doc = {
        'asset': {'version': '2.0', 'generator': 'nu_nerf_amd.texture'},
        'scene': 0,
        'scenes': [{'nodes': [0]}],
        'nodes': [{'mesh': 0}],
        'meshes': [{'primitives': [{'attributes': {'POSITION': 0, 'NORMAL': 1, 'TEXCOORD_0': 2}, 'material': 0, 'mode': 4}]}],
        'materials': [{'name': 'baked', 'pbrMetallicRoughness': {'baseColorFactor': [1.0, 1.0, 1.0, 1.0], 'metallicFactor': 1.0,
                                                                'roughnessFactor': 1.0, 'baseColorTexture': {'index': 0},
                                                                'metallicRoughnessTexture': {'index': 1}}}],
        'textures': [{'sampler': 0, 'source': 0}, {'sampler': 0, 'source': 1}],
        'samplers': [{'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}],
        'images': [{'uri': tex('albedo.png')}, {'uri': tex('orm.png')}],
        'buffers': [{'uri': os.path.basename(bin_path), 'byteLength': offsets[-1]}],
        'bufferViews': [{'buffer': 0, 'byteOffset': offsets[i], 'byteLength': len(blobs[i]), 'target': 34962} for i in range(len(blobs))],
        'accessors': [dict({'bufferView': 0, 'componentType': 5126, 'count': n, 'type': 'VEC3'}, **bounds(P)),
                      dict({'bufferView': 1, 'componentType': 5126, 'count': n, 'type': 'VEC3'}, **bounds(N)),
                      dict({'bufferView': 2, 'componentType': 5126, 'count': n, 'type': 'VEC2'}, **bounds(T2))],
    }
    if tangent is not None:
        doc['meshes'][0]['primitives'][0]['attributes']['TANGENT'] = 3
        doc['accessors'].append({'bufferView': 3, 'componentType': 5126, 'count': n, 'type': 'VEC4'})
        doc['materials'][0]['normalTexture'] = {'index': 2, 'scale': 1.0}
        doc['textures'].append({'sampler': 0, 'source': 2})
        doc['images'].append({'uri': tex('normal.png')})
    with open(path, 'w') as fh:
        json.dump(doc, fh, indent=1)
    return path, bin_path
