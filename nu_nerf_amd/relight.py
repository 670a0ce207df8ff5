"""python -m nu_nerf_amd.relight --mesh PLY --material DIR --hdr FILE --name NAME [--texture DIR [--normal-map]] [--trans] [--num 360 --width 800 --height 800
--samples 1024 --cam_dist 3.0 --azimuth 0 --elevation 45] [--splitsum [--pyramid DIR | --levels R ...] [--transfer DIR [--occlusion ao|sh]]] [--inner PLY --inner-material DIR (--ior VALUE_OR_DIR | --shell DIR_OR_PAIR [--shell-curvature FILE])]

relight.py + blender_backend/relight_backend.py on the GPU: the extracted mesh, the per-vertex DIR/metallic.npy, roughness.npy and
albedo.npy that extract_materials writes and a lat-long HDR environment map are rendered from the reference's camera orbit
(generate_relghting_poses) into data/relight/NAME/{k}.png, RGBA with alpha 0 off the object (film_transparent); frames that exist are
skipped (relight_backend.py:82).  Blender is not involved: primary visibility, a G-buffer and `samples` shadow rays per hit pixel are
traced on the HIP LBVH (nu_relight_gbuffer, nu_relight_visibility) and shaded by nu_relight_resolve with the material model the
networks were trained under.  DESIGN.md 20 defines the light transport and lists what is not Cycles; nothing here is pinned
against Blender output.

--inner: the nested object of stage 2.  --mesh is then the transparent outer shell, --inner the cleaned inner mesh with its baked
--inner-material, --ior the shell's index of refraction: a number (default 1.5) or the directory whose ior.npy [V,1]
extract_materials --stage2 wrote; --material is not needed.  The view refracts into the shell, the inner object is lit through it
(DESIGN.md 21).  --trans turns both meshes.  --shell instead of --ior: the shell is the thin glass wall of the non-zero-thickness
stage-2 model around an air-like cavity: the directory whose shell_ior.npy and shell_thickness.npy [V,1]
extract_materials --stage2 wrote for such a config, or "IOR,THICKNESS" (two numbers, e.g. "1.45,0.005").

--texture DIR: the atlas.npz `python -m nu_nerf_amd.bake_textures` wrote for this mesh: albedo, metallic and roughness of
every hit come from the texture atlas, looked up at the hit point, instead of the per-vertex arrays (--material is then not needed).  Works
in the Monte-Carlo and the --splitsum path, also with --transfer; not with --inner.  --normal-map (with --texture): the shading normal
of every hit comes from the atlas as well -- the SDF normals `bake_textures --normals sdf` put there -- instead of the mix
of the mesh's vertex normals; a directory whose atlas.npz has no normals is refused.

--hdr takes a Radiance .hdr (RGBE, flat or run-length scanlines) or a .npy float [H,W,3]; the map is z up in the mesh's frame.
--focal_mm / --sensor_mm: Blender's default camera (50 mm on a 36 mm sensor fitted to the larger image side).  --seed, --chunk
(samples per pass; bounds device memory) and --output (default data/relight/NAME) are this project's own.

--splitsum: the deterministic second path, the split-sum image formation the networks were trained under evaluated from a
prefiltered roughness pyramid -- no sampling, no noise, no shadows: a frame is its G-buffer pass and one resolve launch.  With --hdr the
map is prefiltered at --levels (default 0 .25 .5 .75 1; environment.prefilter); with --pyramid DIR it reads env_pyramid.npy,
roughness.npy and, if present, env_diffuse.npy (otherwise the diffuse map is the level of roughness 1), so a directory written by
extract_environment or prefilter_environment works as it is.  --samples, --seed and --chunk are not used; --inner is refused.
--transfer DIR: the per-vertex ao.npy, bent_normal.npy and transfer.npy that `python -m nu_nerf_amd.bake_transfer` wrote for this mesh
shadow the frame -- --occlusion ao (default) darkens the diffuse light by the ambient occlusion, sh lights it through
the order-2 transfer vector against the environment's SH coefficients (DIR/env_sh.npy of --pyramid if present, otherwise projected
from its env.npy or its level of lowest roughness; from --hdr); both scale the specular light by the specular occlusion.
"""
import argparse
import os
import sys

import numpy as np

ROW = 20                        # floats per G-buffer row (csrc/relight.h)
MISS = 10000000
ORIGIN_EPS = 1e-4               # shadow-ray origin = hit point + ORIGIN_EPS * viewer-facing geometric normal (scenes live in the unit sphere)
VIS_BYTES = 256 << 20           # the visibility bytes of one pass never exceed this
R_BLENDER = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # x_blender = R_BLENDER @ x_wrd (set_camera_by_pose)
TRANS = R_BLENDER               # --trans: the mesh turned +90 degrees about x (relight_backend.py:46-48) -- the same matrix


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def relighting_poses(num, azimuth, elevation, dist):
    """blender_utils.generate_relghting_poses: [num,3,4] float64 world -> camera [R|t] (x right, y down, z forward), t = (0, 0, dist);
    azimuths = azimuth + linspace(-90, 90, num) degrees at a fixed elevation, looking at the origin with z up, the rotation composed
    with R_trans (x_norm = R_trans x_wrd)."""
    az = np.deg2rad(azimuth) + np.linspace(-np.pi / 2, np.pi / 2, num)
    el = np.ones_like(az) * np.deg2rad(elevation)
    pts = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1)
    up = np.array([0.0, 0.0, 1.0])
    z = -pts / np.linalg.norm(pts, 2, 1, keepdims=True)
    y = -(up[None, :] - np.sum(z * up[None, :], 1, keepdims=True) * z)
    y = y / np.linalg.norm(y, 2, 1, keepdims=True)
    x = np.cross(y, z)
    rot = np.stack([x, y, z], 1) @ R_BLENDER[None]
    t = np.repeat(np.array([0.0, 0.0, dist])[None, :, None], num, 0)
    return np.concatenate([rot, t], -1)


def camera_in_mesh_frame(pose):
    """The frame change of set_camera_by_pose without its final Blender-camera axis flip: pose [...,3,4] (x_cam = R x_wrd + t) ->
    [R R_blender^T | t], the world -> camera transform in the frame the mesh is imported into (x_blender = R_blender x_wrd).  With the
    poses of relighting_poses R_trans and R_blender cancel: the result is the plain z-up look-at orbit."""
    pose = np.asarray(pose, np.float64)
    return np.concatenate([pose[..., :3] @ R_BLENDER.T, pose[..., 3:]], -1)


def intrinsics(h, w, focal_mm=50.0, sensor_mm=36.0):
    """K [3,3] float64 of Blender's default camera: fx = fy = focal / sensor * max(w, h), centre (w / 2, h / 2)."""
    f = focal_mm / sensor_mm * max(w, h)
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])


# ---- environment maps --------------------------------------------------------------------------------------------------------------
def read_hdr(path):
    """float32 [H,W,3] from a Radiance RGBE file (flat or new run-length scanlines, `-Y H +X W`) or a .npy float [H,W,3].
    An RGBE pixel (r, g, b, e) is (r, g, b) * 2^(e - 136), and 0 when e = 0: exact in fp32."""
    path = str(path)
    if path.lower().endswith('.npy'):
        a = np.load(path)
        if a.ndim != 3 or a.shape[2] != 3 or not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"{path}: expected a float array [H,W,3], got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a, np.float32)
    with open(path, 'rb') as fh:
        data = fh.read()
    pos, fmt, first = 0, None, True
    while True:
        end = data.find(b'\n', pos)
        if end < 0:
            raise ValueError(f"{path}: the header does not end")
        line = data[pos:end].strip()
        pos = end + 1
        if first:
            if not line.startswith(b'#?'):
                raise ValueError(f"{path}: not a Radiance file (no #? signature)")
            first = False
            continue
        if not line:
            break
        if line.startswith(b'FORMAT='):
            fmt = line[7:].strip()
    if fmt != b'32-bit_rle_rgbe':
        raise ValueError(f"{path}: FORMAT is {fmt!r}, only 32-bit_rle_rgbe is read")
    end = data.find(b'\n', pos)
    tok = data[pos:end].split() if end >= 0 else []
    if len(tok) != 4 or tok[0] != b'-Y' or tok[2] != b'+X' or not (tok[1].isdigit() and tok[3].isdigit()):
        raise ValueError(f"{path}: resolution line {data[pos:max(end, pos)][:40]!r} is not `-Y H +X W`")
    h, w = int(tok[1]), int(tok[3])
    if h <= 0 or w <= 0:
        raise ValueError(f"{path}: empty image {h} x {w}")
    pos = end + 1
    buf = np.frombuffer(data, np.uint8)
    rgbe = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        if pos + 4 > len(buf):
            raise ValueError(f"{path}: the pixel data ends in scanline {y}")
        if 8 <= w <= 0x7fff and buf[pos] == 2 and buf[pos + 1] == 2 and (int(buf[pos + 2]) << 8 | int(buf[pos + 3])) == w:
            pos += 4
            for c in range(4):
                x = 0
                while x < w:
                    if pos >= len(buf):
                        raise ValueError(f"{path}: the pixel data ends in scanline {y}")
                    n = int(buf[pos])
                    pos += 1
                    if n > 128:
                        n -= 128
                        if n == 0 or x + n > w or pos >= len(buf):
                            raise ValueError(f"{path}: bad run in scanline {y}")
                        rgbe[y, x:x + n, c] = buf[pos]
                        pos += 1
                    else:
                        if n == 0 or x + n > w or pos + n > len(buf):
                            raise ValueError(f"{path}: bad literal in scanline {y}")
                        rgbe[y, x:x + n, c] = buf[pos:pos + n]
                        pos += n
                    x += n
        else:
            if pos + 4 * w > len(buf):
                raise ValueError(f"{path}: the pixel data ends in scanline {y}")
            rgbe[y] = buf[pos:pos + 4 * w].reshape(w, 4)
            pos += 4 * w
    e = rgbe[..., 3].astype(np.int32)
    out = np.ldexp(rgbe[..., :3].astype(np.float32), (e - 136)[..., None]).astype(np.float32)
    out[e == 0] = 0.0
    return out


def pack_env(env):
    """float32 [H,W,4] RGBA (A = 1) from [H,W,3]: one 16-byte load per tap on the device."""
    env = np.asarray(env, np.float32)
    if env.ndim != 3 or env.shape[2] != 3 or env.shape[0] < 1 or env.shape[1] < 1:
        raise ValueError(f"environment map must be [H,W,3], got {env.shape}")
    if not np.isfinite(env).all():
        raise ValueError("environment map has non-finite values")
    return np.ascontiguousarray(np.concatenate([env, np.ones_like(env[..., :1])], -1))


# ---- device passes -----------------------------------------------------------------------------------------------------------------------
class Scene:
    """Mesh + LBVH + what the G-buffer pass interpolates: unit vertex normals [V,3] and materials [V,5] = albedo, metallic, roughness.
    materials: a dict with 'albedo' [V,3], 'metallic' [V,1], 'roughness' [V,1] (the arrays extract_materials writes) or one [V,5].
    texture (optional): a texture atlas of the mesh's faces (texture.bake_textures / load_textures / pack_atlas) that
    relight_linear and relight_splitsum_linear shade from instead; materials may then be None (zeros: every hit row is overwritten)."""

    def __init__(self, V, F, materials, device=None, texture=None):
        import torch
        from .lbvh import LBVH, vertex_normals_and_curvature
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        V = torch.as_tensor(np.asarray(V) if not torch.is_tensor(V) else V).to(torch.float32)
        F = torch.as_tensor(np.asarray(F) if not torch.is_tensor(F) else F).to(torch.int32)
        if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"mesh must be V [Nv,3], F [Nf,3], got {tuple(V.shape)} {tuple(F.shape)}")
        if F.numel() and (int(F.min()) < 0 or int(F.max()) >= V.shape[0]):
            raise ValueError("face index out of range")
        if materials is None and texture is not None:
            m = np.zeros((V.shape[0], 5), np.float32)
        elif isinstance(materials, dict):
            m = np.concatenate([np.asarray(materials['albedo'], np.float32).reshape(-1, 3),
                                np.asarray(materials['metallic'], np.float32).reshape(-1, 1),
                                np.asarray(materials['roughness'], np.float32).reshape(-1, 1)], 1)
        else:
            m = np.asarray(materials.cpu() if torch.is_tensor(materials) else materials, np.float32)
        if m.shape != (V.shape[0], 5):
            raise ValueError(f"materials must give 5 values for each of the {V.shape[0]} vertices, got {m.shape}")
        self.V, self.F = V.to(dev).contiguous(), F.to(dev).contiguous()
        self.bvh = LBVH(self.V, self.F)
        self.normals = vertex_normals_and_curvature(V, F)[0].to(dev).contiguous()
        self.materials = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        self.device = dev
        self.texture = None if texture is None else _packed_texture(self, texture)


def gbuffer(scene, cams, h, w, img0=0, y0=0, rows=None):
    """face int32 [n, rows, w], gbuf float32 [n, rows, w, ROW] of rows [y0, y0 + rows) of the images of cams [n,21]."""
    import torch
    from . import _lib as L
    rows = h - y0 if rows is None else rows
    n = int(cams.shape[0])
    face = torch.empty(n, rows, w, dtype=torch.int32, device=scene.device)
    gbuf = torch.empty(n, rows, w, ROW, dtype=torch.float32, device=scene.device)
    L.load().nu_relight_gbuffer(L.ptr(scene.bvh.buf), scene.bvh.n_faces, L.ptr(scene.V), L.ptr(scene.F), L.ptr(scene.normals),
                                L.ptr(scene.materials), L.ptr(cams), n, int(img0), int(h), int(w), int(y0), int(rows), L.ptr(face),
                                L.ptr(gbuf), L.stream())
    return face, gbuf


def hit_pixels(face):
    """int32 indices of the G-buffer rows that hold a hit (one device -> host read: the count)."""
    import torch
    return (face.reshape(-1) != MISS).nonzero().flatten().to(torch.int32)


def visibility(scene, gbuf, pix, samples, s0, s_count, seed, eps=ORIGIN_EPS):
    """uint8 [n_pix, s_count]: 1 where sample s0 + c of pixel pix[i] sees the environment."""
    import torch
    from . import _lib as L
    vis = torch.empty(int(pix.shape[0]), int(s_count), dtype=torch.uint8, device=gbuf.device)
    L.load().nu_relight_visibility(L.ptr(scene.bvh.buf), scene.bvh.n_faces, L.ptr(gbuf), L.ptr(pix), int(pix.shape[0]), int(samples),
                                   int(s0), int(s_count), _seed(seed), float(eps), L.ptr(vis), L.stream())
    return vis


def shadow_rays(gbuf, pix, samples, s0, s_count, seed, eps=ORIGIN_EPS):
    """(rays float32 [n_pix * s_count, 6], bits int32 [n_pix * s_count, 3]): the rays visibility() traces, the two 24-bit sample
    integers behind each and 1 where it is traced (tests)."""
    import torch
    from . import _lib as L
    N = int(pix.shape[0]) * int(s_count)
    rays = torch.empty(N, 6, dtype=torch.float32, device=gbuf.device)
    bits = torch.empty(N, 3, dtype=torch.int32, device=gbuf.device)
    L.load().nu_relight_shadow_rays(L.ptr(gbuf), L.ptr(pix), int(pix.shape[0]), int(samples), int(s0), int(s_count), _seed(seed),
                                    float(eps), L.ptr(rays), L.ptr(bits), L.stream())
    return rays, bits


def resolve(gbuf, pix, samples, s0, s_count, seed, env, vis, out):
    """out [rows of gbuf, 4] += the shaded samples [s0, s0 + s_count) of the listed pixels (env: packed RGBA on the device)."""
    from . import _lib as L
    L.load().nu_relight_resolve(L.ptr(gbuf), L.ptr(pix), int(pix.shape[0]), int(samples), int(s0), int(s_count), _seed(seed), L.ptr(env),
                                int(env.shape[0]), int(env.shape[1]), L.ptr(vis), 2.0 / samples, L.ptr(out), L.stream())
    return out


def env_lookup(env, dirs):
    """Bilinear lat-long lookup of the packed environment at dirs [N,3] -> [N,3] (tests)."""
    import torch
    from . import _lib as L
    dirs = dirs.to(torch.float32).contiguous()
    out = torch.empty(dirs.shape[0], 3, dtype=torch.float32, device=dirs.device)
    L.load().nu_relight_env_lookup(L.ptr(env), int(env.shape[0]), int(env.shape[1]), L.ptr(dirs), int(dirs.shape[0]), L.ptr(out), L.stream())
    return out


def _seed(seed):
    """The seed as the C int the ABI takes (its 32 bits are what the hash reads)."""
    seed = int(seed) & 0xffffffff
    return seed - (1 << 32) if seed >= 1 << 31 else seed


def _scene(V, F=None, materials=None):
    return V if isinstance(V, Scene) else Scene(V, F, materials)


def _packed_texture(scene, texture):
    """The atlas on the scene's device as the lookup kernels read it (texture.PackedAtlas), checked against the scene's face count."""
    from .texture import pack_atlas
    atlas = pack_atlas(texture, device=scene.device)
    if atlas.n_faces != int(scene.F.shape[0]):
        raise ValueError(f"texture: the atlas is laid out for {atlas.n_faces} faces, the mesh has {int(scene.F.shape[0])}")
    if atlas.device != scene.device:
        raise ValueError(f"texture: the atlas is on {atlas.device}, the scene on {scene.device}")
    return atlas


def _texture_of(scene, texture, normal_map=False):
    """texture= of a relight call: the argument if given, otherwise the Scene's own atlas (None: per-vertex materials).  normal_map
    asks for an atlas that carries normals: ValueError without one."""
    tex = scene.texture if texture is None else _packed_texture(scene, texture)
    if normal_map and (tex is None or not tex.has_normal):
        raise ValueError("normal_map=True needs a texture with normals (texture.bake_textures(..., normals='sdf'))")
    return tex


def relight_linear(V, F, materials, env, poses, h, w, samples, seed=0, chunk=256, rows=None, images=1, K=None, img0=0,
                   eps=ORIGIN_EPS, texture=None, normal_map=False):
    """Linear radiance float32 [n,h,w,4] (RGB, alpha 1 on hit pixels and 0 elsewhere) on the device.  poses [n,3,4]: world -> camera in
    the mesh's frame (camera_in_mesh_frame of relighting_poses); K: [3,3] (default intrinsics(h, w)); env [H,W,3]; V may be a Scene.
    Image i is sampled as image img0 + i.  Work is done `images` images x `rows` image rows x `chunk` samples at a time; the result
    does not depend on any of the three, bit for bit.  Device memory besides the mesh, the environment and the result: 100 bytes per
    pixel of a piece (G-buffer row, face id, hit list) plus at most VIS_BYTES of visibility bytes -- independent of `samples`.
    texture: a texture atlas of the mesh (default: the Scene's own, if it has one) -- the material columns of every hit
    row are then looked up in it at the hit point (texture.texture_gbuffer) before anything is shaded; None without one: untouched.
    normal_map=True: the shading normal of every hit row is taken from the texture's normal lanes as well (it needs a
    texture baked with normals='sdf'); the visibility and resolve kernels run unchanged on that G-buffer."""
    import torch
    from .mask_render import _cams
    samples, chunk = int(samples), int(chunk)
    if samples < 2 or samples % 2:
        raise ValueError(f"samples must be even and >= 2, got {samples}")
    if chunk < 1 or images < 1 or (rows is not None and rows < 1):
        raise ValueError("chunk, rows and images must be >= 1")
    scene = _scene(V, F, materials)
    dev = scene.device
    tex = _texture_of(scene, texture, normal_map)
    poses = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float64).reshape(-1, 3, 4)
    K = intrinsics(h, w) if K is None else np.asarray(K, np.float64)
    cams = _cams(K.astype(np.float32), poses.astype(np.float32), dev)
    envd = torch.from_numpy(pack_env(env)).to(dev)
    n, rows = int(cams.shape[0]), int(rows or h)
    out = torch.zeros(n, h, w, 4, dtype=torch.float32, device=dev)
    for i0 in range(0, n, images):
        ni = min(images, n - i0)
        for y0 in range(0, h, rows):
            nr = min(rows, h - y0)
            face, gbuf = gbuffer(scene, cams[i0:i0 + ni], h, w, img0 + i0, y0, nr)
            pix_all = hit_pixels(face)
            if tex is not None:
                from .texture import texture_gbuffer
                texture_gbuffer(scene, face, gbuf, pix_all, tex, normals=bool(normal_map))
            piece = torch.zeros(ni * nr * w, 4, dtype=torch.float32, device=dev)
            per = max(1, min(VIS_BYTES // min(chunk, samples), (2 ** 31 - 1) // ((min(chunk, samples) + 15) // 16)))
            for p0 in range(0, int(pix_all.shape[0]), per):
                pix = pix_all[p0:p0 + per].contiguous()
                for s0 in range(0, samples, chunk):
                    sc = min(chunk, samples - s0)
                    vis = visibility(scene, gbuf, pix, samples, s0, sc, seed, eps)
                    resolve(gbuf, pix, samples, s0, sc, seed, envd, vis, piece)
            out[i0:i0 + ni, y0:y0 + nr] = piece.reshape(ni, nr, w, 4)
    return out


def to_srgb8(linear):
    """uint8 [..., 4] from linear RGBA: RGB through the project's linear_to_srgb, clipped to [0, 1], rounded to 8 bits; alpha 255 / 0."""
    import torch
    from .torch_glue import linear_to_srgb
    rgb = linear_to_srgb(linear[..., :3]).clamp(0.0, 1.0)
    return torch.cat([torch.floor(rgb * 255.0 + 0.5), linear[..., 3:] * 255.0], -1).to(torch.uint8)


def relight(V, F, materials, env, poses, h, w, samples, seed=0, chunk=256, **kw):
    """uint8 [n,h,w,4] sRGB + alpha of relight_linear (same arguments)."""
    return to_srgb8(relight_linear(V, F, materials, env, poses, h, w, samples, seed, chunk, **kw))


# ---- split-sum relighting from a prefiltered pyramid ------------------------------------------------------------------
MAX_LEVELS = 16                 # NU_ENV_MAX_LOBES
_FG = {}


def fg_table(device):
    """The split-sum table (params.load_fg_lut) [256,256,2] on the device, uploaded once per device."""
    import torch
    from .params import load_fg_lut
    key = str(device)
    if key not in _FG:
        _FG[key] = torch.from_numpy(np.ascontiguousarray(load_fg_lut().reshape(256, 256, 2))).to(device)
    return _FG[key]


def pack_pyramid(pyramid, levels):
    """(float32 [L,h,w,4] RGBA, float32 [L]) from a pyramid [L,h,w,3] and its roughness levels: finite, strictly ascending, at most
    MAX_LEVELS."""
    pyramid, levels = np.asarray(pyramid, np.float32), np.asarray(levels, np.float32).reshape(-1)
    if pyramid.ndim != 4 or pyramid.shape[3] != 3 or min(pyramid.shape) < 1:
        raise ValueError(f"pyramid must be [L,h,w,3], got {pyramid.shape}")
    if levels.shape[0] != pyramid.shape[0] or not 1 <= levels.shape[0] <= MAX_LEVELS:
        raise ValueError(f"levels must give one roughness for each of the 1..{MAX_LEVELS} pyramid levels, got {levels.shape} for {pyramid.shape}")
    if not np.isfinite(levels).all() or (np.diff(levels) <= 0).any():
        raise ValueError(f"levels must be finite and strictly ascending, got {levels.tolist()}")
    if not np.isfinite(pyramid).all():
        raise ValueError("pyramid has non-finite values")
    return np.ascontiguousarray(np.concatenate([pyramid, np.ones_like(pyramid[..., :1])], -1)), np.ascontiguousarray(levels)


def _levels_arg(levels):
    import ctypes
    levels = np.asarray(levels, np.float32).reshape(-1)
    return (ctypes.c_float * len(levels))(*levels.tolist()), len(levels)


def pyramid_lookup(pyr, levels, dirs, rho):
    """L(d, rho) [N,3] of the packed pyramid pyr [L,h,w,4] (device) with roughness `levels` [L] (host) at dirs [N,3], rho [N]: rho clamped
    to the levels' range, the two levels around it tapped as env_lookup does and mixed linearly."""
    import torch
    from . import _lib as L
    for t, shape, what in ((pyr, (None, None, None, 4), 'pyramid'), (dirs, (None, 3), 'dirs'), (rho, (dirs.shape[0],), 'rho')):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != len(shape) \
                or any(s is not None and int(d) != int(s) for d, s in zip(t.shape, shape)):
            raise L.NuNerfLibraryError(f"nu_env_pyramid_lookup failed with code -1 (NU_ERR_ARG): {what} must be a contiguous float32 "
                                       f"device tensor of shape {list(shape)}")
    lv, nl = _levels_arg(levels)
    if nl != pyr.shape[0]:
        raise L.NuNerfLibraryError(f"nu_env_pyramid_lookup failed with code -1 (NU_ERR_ARG): {nl} levels for a pyramid of {pyr.shape[0]}")
    out = torch.empty(dirs.shape[0], 3, dtype=torch.float32, device=dirs.device)
    L.load().nu_env_pyramid_lookup(L.ptr(pyr), nl, int(pyr.shape[1]), int(pyr.shape[2]), lv, L.ptr(dirs), L.ptr(rho), int(dirs.shape[0]),
                                   L.ptr(out), L.stream())
    return out


def splitsum_resolve(gbuf, pix, pyr, levels, diffuse, out):
    """out [rows of gbuf, 4] = the split-sum colour of the listed hit pixels (pyr [L,h,w,4], diffuse [dh,dw,4]: packed, on the device)."""
    from . import _lib as L
    lv, nl = _levels_arg(levels)
    L.load().nu_relight_splitsum(L.ptr(gbuf), L.ptr(pix), int(pix.shape[0]), L.ptr(pyr), nl, int(pyr.shape[1]), int(pyr.shape[2]), lv,
                                 L.ptr(diffuse), int(diffuse.shape[0]), int(diffuse.shape[1]), L.ptr(fg_table(gbuf.device)), L.ptr(out),
                                 L.stream())
    return out


OCCLUSION = {'ao': 0, 'sh': 1}  # NU_OCC_AO, NU_OCC_SH


def splitsum_resolve_occluded(scene, gbuf, face, pix, pyr, levels, diffuse, transfer, env_sh, mode, out):
    """out [rows of gbuf, 4] = the split-sum colour of the listed hit pixels shadowed by `transfer` [Nv,16] (device; transfer.py): mode
    'ao' scales the diffuse term by the ambient occlusion, 'sh' replaces it by the dot product of the transfer vector with env_sh [9,4]
    (device); both scale the specular term by the specular occlusion.  face: the G-buffer pass's face ids."""
    from . import _lib as L
    lv, nl = _levels_arg(levels)
    L.load().nu_relight_splitsum_occluded(L.ptr(gbuf), L.ptr(face), L.ptr(pix), int(pix.shape[0]), L.ptr(scene.V), L.ptr(scene.F),
                                          L.ptr(transfer), L.ptr(env_sh), OCCLUSION[mode], L.ptr(pyr), nl, int(pyr.shape[1]),
                                          int(pyr.shape[2]), lv, L.ptr(diffuse), int(diffuse.shape[0]), int(diffuse.shape[1]),
                                          L.ptr(fg_table(gbuf.device)), L.ptr(out), L.stream())
    return out


def _transfer_args(scene, transfer, occlusion, env_sh):
    """The device arrays of the shadowed resolve: transfer float32 [Nv,16] (a device tensor is taken as it is) and env_sh [9,4] or None."""
    import torch
    from .transfer import ROW as TR_ROW, pack_env_sh
    if occlusion not in OCCLUSION:
        raise ValueError(f"occlusion must be 'ao' or 'sh', got {occlusion!r}")
    if occlusion == 'sh' and env_sh is None:
        raise ValueError("occlusion='sh' needs env_sh, the SH coefficients [9,3] of the environment (environment.project_sh)")
    t = transfer if torch.is_tensor(transfer) else torch.from_numpy(np.ascontiguousarray(transfer, np.float32))
    t = t.detach().to(device=scene.device, dtype=torch.float32).contiguous()
    if tuple(t.shape) != (int(scene.V.shape[0]), TR_ROW):
        raise ValueError(f"transfer must be [{int(scene.V.shape[0])},{TR_ROW}] (one row per vertex), got {tuple(t.shape)}")
    sh = None if env_sh is None else torch.from_numpy(pack_env_sh(env_sh)).to(scene.device)
    return t, sh


def relight_splitsum_linear(V, F, materials, pyramid, levels, diffuse, poses, h, w, rows=None, images=1, K=None, transfer=None,
                            occlusion='ao', env_sh=None, texture=None, normal_map=False):
    """Linear radiance float32 [n,h,w,4] (alpha 1 on hit pixels, 0 elsewhere) of the split-sum model the networks were trained under:
    (1 - metallic) albedo Ld(n) + (F0 A + B) L(reflect(v, n), roughness), L from the prefiltered `pyramid` [L,ph,pw,3] at the roughness
    `levels` [L], Ld from `diffuse` [dh,dw,3], (A, B) from the shipped table.  No sampling, no visibility, no interreflection: a frame is
    its G-buffer pass and one resolve launch.  The Scene, cameras, G-buffer and hit list are relight_linear's; the result does not depend
    on `rows` / `images`, bit for bit.
    transfer: float32 [Nv,16] rows of transfer.bake_transfer for the mesh's vertices -- the frame then has contact shadows and
    self-occlusion: occlusion='ao' darkens the diffuse term by the ambient occlusion, 'sh' lights it with the transfer
    vector against env_sh [9,3] (environment.project_sh of the environment); None is the unshadowed path above, untouched.
    texture: as relight_linear's -- the hit rows take albedo, metallic and roughness from the atlas before the resolve (either one).
    normal_map: as relight_linear's; with transfer= the baked per-vertex transfer rows are used as they are."""
    import torch
    from .mask_render import _cams
    if images < 1 or (rows is not None and rows < 1):
        raise ValueError("rows and images must be >= 1")
    scene = _scene(V, F, materials)
    dev = scene.device
    pyr, lv = pack_pyramid(pyramid, levels)
    pyr, dif = torch.from_numpy(pyr).to(dev), torch.from_numpy(pack_env(diffuse)).to(dev)
    tr, sh = (None, None) if transfer is None else _transfer_args(scene, transfer, occlusion, env_sh)
    tex = _texture_of(scene, texture, normal_map)
    poses = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float64).reshape(-1, 3, 4)
    K = intrinsics(h, w) if K is None else np.asarray(K, np.float64)
    cams = _cams(K.astype(np.float32), poses.astype(np.float32), dev)
    n, rows = int(cams.shape[0]), int(rows or h)
    out = torch.zeros(n, h, w, 4, dtype=torch.float32, device=dev)
    for i0 in range(0, n, images):
        ni = min(images, n - i0)
        for y0 in range(0, h, rows):
            nr = min(rows, h - y0)
            face, gbuf = gbuffer(scene, cams[i0:i0 + ni], h, w, i0, y0, nr)
            piece = torch.zeros(ni * nr * w, 4, dtype=torch.float32, device=dev)
            pix = hit_pixels(face)
            if tex is not None:
                from .texture import texture_gbuffer
                texture_gbuffer(scene, face, gbuf, pix, tex, normals=bool(normal_map))
            if transfer is None:
                splitsum_resolve(gbuf, pix, pyr, lv, dif, piece)
            else:
                splitsum_resolve_occluded(scene, gbuf, face, pix, pyr, lv, dif, tr, sh, occlusion, piece)
            out[i0:i0 + ni, y0:y0 + nr] = piece.reshape(ni, nr, w, 4)
    return out


def relight_splitsum(V, F, materials, pyramid, levels, diffuse, poses, h, w, **kw):
    """uint8 [n,h,w,4] sRGB + alpha of relight_splitsum_linear (same arguments)."""
    return to_srgb8(relight_splitsum_linear(V, F, materials, pyramid, levels, diffuse, poses, h, w, **kw))


def load_pyramid_dir(directory):
    """(pyramid [L,h,w,3], levels [L], diffuse [dh,dw,3]) of a directory as extract_environment or prefilter_environment writes it:
    env_pyramid.npy, roughness.npy and, if present, env_diffuse.npy.  Without env_diffuse.npy the diffuse map is the level whose
    roughness is 1 (what the model's diffuse light queries); no such level is an error."""
    pyramid = np.load(os.path.join(directory, 'env_pyramid.npy'))
    levels = np.load(os.path.join(directory, 'roughness.npy')).reshape(-1)
    if pyramid.ndim != 4 or pyramid.shape[3] != 3 or pyramid.shape[0] != levels.shape[0]:
        raise ValueError(f"{directory}: env_pyramid.npy {pyramid.shape} and roughness.npy {levels.shape} are not [L,h,w,3] and [L]")
    path = os.path.join(directory, 'env_diffuse.npy')
    if os.path.exists(path):
        diffuse = np.load(path)
    else:
        one = np.flatnonzero(levels == 1.0)
        if one.size == 0:
            raise ValueError(f"{directory}: no env_diffuse.npy and no pyramid level of roughness 1 (levels {levels.tolist()}) to take the "
                             "diffuse map from")
        diffuse = pyramid[int(one[0])]
    order = np.argsort(levels, kind='stable')
    return np.ascontiguousarray(pyramid[order], np.float32), np.ascontiguousarray(levels[order], np.float32), np.asarray(diffuse, np.float32)


# ---- the nested object ------------------------------------------------------------------------------------------------
def load_env_sh(directory):
    """(env_sh float64 [9,3], the file it came from) of a pyramid directory: env_sh.npy if present, otherwise the projection
    (environment.project_sh) of env.npy or, without one, of the pyramid level of lowest roughness."""
    from .environment import project_sh
    path = os.path.join(directory, 'env_sh.npy')
    if os.path.exists(path):
        sh = np.asarray(np.load(path), np.float64)
        if sh.shape != (9, 3):
            raise ValueError(f"{path}: expected [9,3], got {sh.shape}")
        return sh, path
    path = os.path.join(directory, 'env.npy')
    if os.path.exists(path):
        return project_sh(np.load(path)), path + ' (projected)'
    pyramid, levels, _ = load_pyramid_dir(directory)
    return project_sh(pyramid[0]), os.path.join(directory, 'env_pyramid.npy') + f' level of roughness {float(levels[0]):g} (projected)'


MAX_SEGMENTS = 4                # NU_RLN_MAX_SEGMENTS: interior segments of a camera path before the pixel counts as dark
CHAIN = 12                      # floats per chain record (include/nu_nerf.h)
DARK, INNER, EXIT = 0, 1, 2     # terminal kinds of a pixel's interior chain
SEG, LIGHT_DUMP = 16, 20        # floats per dumped segment / light path


class NestedScene:
    """A transparent outer shell around an opaque inner mesh: two Scenes (each mesh + LBVH + vertex normals) and the per-vertex index
    of refraction of the shell.  ior: a scalar or [V_o] / [V_o,1], every value finite and >= 1.  The outer Scene's material table holds
    the index minus 1 in column 0, so that the G-buffer pass interpolates it with the barycentrics of the primary hit."""

    def __init__(self, V_o, F_o, ior, V_i, F_i, materials_i, device=None):
        import torch
        nv = int(V_o.shape[0])
        ior = np.asarray(ior.cpu() if torch.is_tensor(ior) else ior, np.float32)
        ior = np.full(nv, float(ior), np.float32) if ior.ndim == 0 else ior.reshape(-1)
        if ior.shape != (nv,):
            raise ValueError(f"ior must be a scalar or give one value for each of the {nv} outer vertices, got {ior.shape}")
        if not np.isfinite(ior).all() or (ior < 1.0).any():
            raise ValueError("ior must be finite and >= 1")
        mo = np.zeros((nv, 5), np.float32)
        mo[:, 0] = ior - 1.0
        self.outer = Scene(V_o, F_o, mo, device)
        self.inner = Scene(V_i, F_i, materials_i, self.outer.device)
        self.ior = torch.from_numpy(ior).to(self.outer.device)
        self.device = self.outer.device

    def _args(self):
        from . import _lib as L
        o, i = self.outer, self.inner
        return (L.ptr(o.bvh.buf), o.bvh.n_faces, L.ptr(o.V), L.ptr(o.F), L.ptr(o.normals), L.ptr(self.ior),
                L.ptr(i.bvh.buf), i.bvh.n_faces, L.ptr(i.V), L.ptr(i.F), L.ptr(i.normals), L.ptr(i.materials))


def nested_chain(ns, gbuf, pix, eps=ORIGIN_EPS, max_segments=MAX_SEGMENTS, dump=False):
    """The interior chain of the listed hit pixels of the OUTER G-buffer -> kind int32 [n], chain float32 [n, CHAIN], inner rows
    float32 [n, ROW]; with dump also seg [n, max_segments, SEG] and aux [n, 2, 8] (see include/nu_nerf.h)."""
    import torch
    from . import _lib as L
    n = int(pix.shape[0])
    kind = torch.empty(n, dtype=torch.int32, device=ns.device)
    chain = torch.empty(n, CHAIN, dtype=torch.float32, device=ns.device)
    irow = torch.empty(n, ROW, dtype=torch.float32, device=ns.device)
    if not dump:
        L.load().nu_relight_nested_chain(*ns._args(), L.ptr(gbuf), L.ptr(pix), n, float(eps), int(max_segments), L.ptr(kind), L.ptr(chain),
                                         L.ptr(irow), L.stream())
        return kind, chain, irow
    seg = torch.empty(n, int(max_segments), SEG, dtype=torch.float32, device=ns.device)
    aux = torch.empty(n, 2, 8, dtype=torch.float32, device=ns.device)
    L.load().nu_relight_nested_chain_dump(*ns._args(), L.ptr(gbuf), L.ptr(pix), n, float(eps), int(max_segments), L.ptr(kind), L.ptr(chain),
                                          L.ptr(irow), L.ptr(seg), L.ptr(aux), L.stream())
    return kind, chain, irow, seg, aux


def nested_light(ns, irow, sel, samples, s0, s_count, seed, eps=ORIGIN_EPS, dump=False):
    """rec float32 [n_sel, s_count, 4] = (exit direction, 1 - F_exit) of the light path of sample s0 + c of inner pixel sel[i], zero
    where it is dark; with dump also [n_sel * s_count, LIGHT_DUMP]."""
    import torch
    from . import _lib as L
    n = int(sel.shape[0])
    rec = torch.empty(n, int(s_count), 4, dtype=torch.float32, device=ns.device)
    if not dump:
        L.load().nu_relight_nested_light(*ns._args(), L.ptr(irow), L.ptr(sel), n, int(samples), int(s0), int(s_count), _seed(seed), float(eps),
                                         L.ptr(rec), L.stream())
        return rec
    d = torch.empty(n * int(s_count), LIGHT_DUMP, dtype=torch.float32, device=ns.device)
    L.load().nu_relight_nested_light_dump(*ns._args(), L.ptr(irow), L.ptr(sel), n, int(samples), int(s0), int(s_count), _seed(seed),
                                          float(eps), L.ptr(rec), L.ptr(d), L.stream())
    return rec, d


def nested_resolve(irow, chain, kind, opix, sel, samples, s0, s_count, seed, env, rec, last, out):
    """out [rows of the outer G-buffer, 4] += the samples [s0, s0 + s_count) of the listed pixels; last: also their reflection and
    exit terms (the call that ends these pixels)."""
    from . import _lib as L
    L.load().nu_relight_nested_resolve(L.ptr(irow), L.ptr(chain), L.ptr(kind), L.ptr(opix), L.ptr(sel), int(sel.shape[0]), int(samples),
                                       int(s0), int(s_count), _seed(seed), L.ptr(env), int(env.shape[0]), int(env.shape[1]), L.ptr(rec),
                                       2.0 / samples, 1 if last else 0, L.ptr(out), L.stream())
    return out


# ---- the thin shell ---------------------------------------------------------------------------------------------------
def _per_vertex(value, nv, what):
    import torch
    a = np.asarray(value.cpu() if torch.is_tensor(value) else value, np.float32)
    a = np.full(nv, float(a), np.float32) if a.ndim == 0 else a.reshape(-1)
    if a.shape != (nv,):
        raise ValueError(f"{what} must be a scalar or give one value for each of the {nv} outer vertices, got {a.shape}")
    return np.ascontiguousarray(a)


class ThinShellScene:
    """The nested object of the non-zero-thickness stage-2 model: the outer mesh is a glass wall with a per-vertex index `ior` (finite,
    > 0; the trained range is 0.6 .. 1.6) and `thickness` (finite, >= 0; trained 0 .. 0.01) around an air-like cavity with the opaque
    inner mesh.  Scalars or [V_o] / [V_o,1].  curvature: the per-vertex Gaussian curvature the wall's two spheres take their radius
    from; default lbvh.vertex_normals_and_curvature of the outer mesh (angle defect over vertex area, clipped to +-10: what the
    stage-2 model trains with).  The outer Scene's material table holds index - 1, thickness and curvature in columns 0..2, so that the
    G-buffer pass interpolates them with the barycentrics of the primary hit."""

    def __init__(self, V_o, F_o, ior, thickness, V_i, F_i, materials_i, curvature=None, device=None):
        import torch
        from .lbvh import vertex_normals_and_curvature
        nv = int(V_o.shape[0])
        ior, thickness = _per_vertex(ior, nv, 'ior'), _per_vertex(thickness, nv, 'thickness')
        if not np.isfinite(ior).all() or (ior <= 0.0).any():
            raise ValueError("ior must be finite and > 0")
        if not np.isfinite(thickness).all() or (thickness < 0.0).any():
            raise ValueError("thickness must be finite and >= 0")
        if curvature is None:
            Vt = torch.as_tensor(np.asarray(V_o) if not torch.is_tensor(V_o) else V_o).detach().cpu().to(torch.float32)
            Ft = torch.as_tensor(np.asarray(F_o) if not torch.is_tensor(F_o) else F_o).detach().cpu().to(torch.long)
            curvature = vertex_normals_and_curvature(Vt, Ft)[1]       # clipped to [-10, 10] there, as the stage-2 model trains with it
        curvature = _per_vertex(curvature, nv, 'curvature')
        if not np.isfinite(curvature).all():
            raise ValueError("curvature must be finite")
        mo = np.zeros((nv, 5), np.float32)
        mo[:, 0], mo[:, 1], mo[:, 2] = ior - 1.0, thickness, curvature
        self.outer = Scene(V_o, F_o, mo, device)
        self.inner = Scene(V_i, F_i, materials_i, self.outer.device)
        self.device = self.outer.device
        self.ior = torch.from_numpy(ior).to(self.device)
        self.thickness = torch.from_numpy(thickness).to(self.device)
        self.curvature = torch.from_numpy(curvature).to(self.device)

    def _args(self):
        from . import _lib as L
        return NestedScene._args(self) + (L.ptr(self.thickness), L.ptr(self.curvature))


def thin_chain(ts, gbuf, pix, eps=ORIGIN_EPS, dump=False):
    """nested_chain for a ThinShellScene (one cavity segment): kind int32 [n], chain float32 [n, CHAIN], inner rows float32 [n, ROW];
    with dump also seg [n, SEG] and aux [n, 2, 8]."""
    import torch
    from . import _lib as L
    n = int(pix.shape[0])
    kind = torch.empty(n, dtype=torch.int32, device=ts.device)
    chain = torch.empty(n, CHAIN, dtype=torch.float32, device=ts.device)
    irow = torch.empty(n, ROW, dtype=torch.float32, device=ts.device)
    if not dump:
        L.load().nu_relight_thin_chain(*ts._args(), L.ptr(gbuf), L.ptr(pix), n, float(eps), L.ptr(kind), L.ptr(chain), L.ptr(irow), L.stream())
        return kind, chain, irow
    seg = torch.empty(n, SEG, dtype=torch.float32, device=ts.device)
    aux = torch.empty(n, 2, 8, dtype=torch.float32, device=ts.device)
    L.load().nu_relight_thin_chain_dump(*ts._args(), L.ptr(gbuf), L.ptr(pix), n, float(eps), L.ptr(kind), L.ptr(chain), L.ptr(irow),
                                        L.ptr(seg), L.ptr(aux), L.stream())
    return kind, chain, irow, seg, aux


def thin_light(ts, irow, sel, samples, s0, s_count, seed, eps=ORIGIN_EPS, dump=False):
    """nested_light for a ThinShellScene: rec float32 [n_sel, s_count, 4] = (exit direction, keep of the leaving crossing), zero where
    the sample is dark; with dump also [n_sel * s_count, LIGHT_DUMP]."""
    import torch
    from . import _lib as L
    n = int(sel.shape[0])
    rec = torch.empty(n, int(s_count), 4, dtype=torch.float32, device=ts.device)
    if not dump:
        L.load().nu_relight_thin_light(*ts._args(), L.ptr(irow), L.ptr(sel), n, int(samples), int(s0), int(s_count), _seed(seed), float(eps),
                                       L.ptr(rec), L.stream())
        return rec
    d = torch.empty(n * int(s_count), LIGHT_DUMP, dtype=torch.float32, device=ts.device)
    L.load().nu_relight_thin_light_dump(*ts._args(), L.ptr(irow), L.ptr(sel), n, int(samples), int(s0), int(s_count), _seed(seed),
                                        float(eps), L.ptr(rec), L.ptr(d), L.stream())
    return rec, d


def thin_cross(d, normal, x, ior, thickness, curvature, inside):
    """The wall crossing row by row (tests): d, normal (outward), x [M,3], ior, thickness, curvature [M] float32 device tensors ->
    dict(refracts, tir_ok [M] bool, normal, end, next_start, next_dir [M,3], fresnel [M,2] = F of the first and the second face)."""
    import torch
    from . import _lib as L
    M = int(d.shape[0])
    ins = [t.to(torch.float32).contiguous() for t in (d, normal, x, ior, thickness, curvature)]
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=d.device)      # noqa: E731
    refr, ok = e(M, dt=torch.uint8), e(M, dt=torch.uint8)
    nrm, pend, ns, nd, fres = e(M, 3), e(M, 3), e(M, 3), e(M, 3), e(M, 2)
    L.load().nu_relight_thin_cross(*[L.ptr(t) for t in ins], M, 1 if inside else 0, L.ptr(refr), L.ptr(ok), L.ptr(nrm), L.ptr(pend),
                                   L.ptr(ns), L.ptr(nd), L.ptr(fres), L.stream())
    return dict(refracts=refr != 0, tir_ok=ok != 0, normal=nrm, end=pend, next_start=ns, next_dir=nd, fresnel=fres)


def relight_nested_linear(scene, env, poses, h, w, samples, seed=0, chunk=256, rows=None, images=1, K=None, img0=0, eps=ORIGIN_EPS,
                          max_segments=MAX_SEGMENTS):
    """relight_linear for a NestedScene or a ThinShellScene (the scene's type picks the shell's transport; max_segments applies to a
    NestedScene only): linear radiance float32 [n,h,w,4], alpha 1 where the primary ray hits the OUTER mesh.  The same
    piece / sample chunking with the same guarantee: the result does not depend on `images`, `rows` or `chunk`, bit for bit.  Device
    memory besides the meshes, the environment and the result: 232 bytes per pixel of a piece (outer row, face id, hit list, chain
    record, kind, inner row) plus at most VIS_BYTES of 16-byte sample records."""
    import torch
    from .mask_render import _cams
    samples, chunk = int(samples), int(chunk)
    if samples < 2 or samples % 2:
        raise ValueError(f"samples must be even and >= 2, got {samples}")
    if chunk < 1 or images < 1 or (rows is not None and rows < 1):
        raise ValueError("chunk, rows and images must be >= 1")
    thin = isinstance(scene, ThinShellScene)
    dev = scene.device
    poses = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float64).reshape(-1, 3, 4)
    K = intrinsics(h, w) if K is None else np.asarray(K, np.float64)
    cams = _cams(K.astype(np.float32), poses.astype(np.float32), dev)
    envd = torch.from_numpy(pack_env(env)).to(dev)
    n, rows = int(cams.shape[0]), int(rows or h)
    out = torch.zeros(n, h, w, 4, dtype=torch.float32, device=dev)
    sc_max = min(chunk, samples)
    per = max(1, min(VIS_BYTES // (16 * sc_max), (2 ** 31 - 1) // ((sc_max + 15) // 16)))
    for i0 in range(0, n, images):
        ni = min(images, n - i0)
        for y0 in range(0, h, rows):
            nr = min(rows, h - y0)
            face, gbuf = gbuffer(scene.outer, cams[i0:i0 + ni], h, w, img0 + i0, y0, nr)
            pix = hit_pixels(face)
            piece = torch.zeros(ni * nr * w, 4, dtype=torch.float32, device=dev)
            kind, chain, irow = thin_chain(scene, gbuf, pix, eps) if thin else nested_chain(scene, gbuf, pix, eps, max_segments)
            inner = (kind == INNER).nonzero().flatten().to(torch.int32)
            other = (kind != INNER).nonzero().flatten().to(torch.int32)
            nested_resolve(irow, chain, kind, pix, other, samples, 0, 0, seed, envd, None, True, piece)
            for p0 in range(0, int(inner.shape[0]), per):
                sel = inner[p0:p0 + per].contiguous()
                for s0 in range(0, samples, chunk):
                    sc = min(chunk, samples - s0)
                    rec = (thin_light if thin else nested_light)(scene, irow, sel, samples, s0, sc, seed, eps)
                    nested_resolve(irow, chain, kind, pix, sel, samples, s0, sc, seed, envd, rec, s0 + sc == samples, piece)
            out[i0:i0 + ni, y0:y0 + nr] = piece.reshape(ni, nr, w, 4)
    return out


def relight_nested(scene, env, poses, h, w, samples, seed=0, chunk=256, **kw):
    """uint8 [n,h,w,4] sRGB + alpha of relight_nested_linear (same arguments)."""
    return to_srgb8(relight_nested_linear(scene, env, poses, h, w, samples, seed, chunk, **kw))


def write_png(path, rgba):
    """RGBA uint8 [h,w,4] as a PNG (Pillow)."""
    from .mask_render import _pillow
    a = np.ascontiguousarray(rgba.cpu().numpy() if hasattr(rgba, 'cpu') else rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"write_png: expected [h,w,4], got {a.shape}")
    _pillow().fromarray(a, 'RGBA').save(path)
    return path


# ---- the command ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.relight", description=__doc__.split("\n\n")[1])
    ap.add_argument('--mesh', type=str, required=True, help="triangle mesh (PLY)")
    args = sys.argv[1:] if argv is None else list(argv)
    # only with --inner may --material be left out.  The exact spelling is enough: every shorter prefix (--inn, --inne) is also one of
    # --inner-material, which argparse refuses as ambiguous; abbreviations stay allowed, as the command without --inner always had them
    nested = any(a == '--inner' or a.startswith('--inner=') for a in args)
    textured = any(a == '--texture' or a.startswith('--texture=') for a in args)
    ap.add_argument('--material', type=str, required=not (nested or textured), help="directory with metallic.npy, roughness.npy, albedo.npy")
    ap.add_argument('--texture', type=str, default=None,
                    help="directory with atlas.npz of the mesh (bake_textures): materials from the texture atlas instead of per vertex")
    ap.add_argument('--normal-map', dest='normal_map', action='store_true', default=False,
                    help="with --texture: shade with the normals baked into the atlas (bake_textures --normals sdf) instead of the vertex normals")
    splitsum = any(a == '--splitsum' for a in args)
    ap.add_argument('--hdr', type=str, required=not splitsum, help="environment map: Radiance .hdr or .npy float [H,W,3]")
    ap.add_argument('--splitsum', action='store_true', default=False,
                    help="deterministic split-sum relighting from a prefiltered pyramid (no sampling, no shadows) instead of the Monte-Carlo path")
    ap.add_argument('--pyramid', type=str, default=None,
                    help="with --splitsum: a directory with env_pyramid.npy and roughness.npy (extract_environment, prefilter_environment) instead of --hdr")
    ap.add_argument('--levels', type=float, nargs='+', default=None, help="with --splitsum --hdr: roughness levels of the pyramid (default 0 .25 .5 .75 1)")
    ap.add_argument('--transfer', type=str, default=None,
                    help="with --splitsum: a directory with transfer.npy, ao.npy and bent_normal.npy of the mesh (bake_transfer): shadowed frames")
    ap.add_argument('--occlusion', choices=tuple(OCCLUSION), default=None,
                    help="with --transfer: ao (default) darkens the diffuse light by the ambient occlusion, sh lights it through the transfer vector")
    ap.add_argument('--name', type=str, required=True, help="frames go to data/relight/NAME")
    ap.add_argument('--trans', action='store_true', default=False, help="turn the mesh +90 degrees about x")
    ap.add_argument('--inner', type=str, default=None, help="inner mesh (PLY): --mesh is then the transparent shell around it")
    ap.add_argument('--inner-material', dest='inner_material', type=str, default=None, help="material directory of the inner mesh")
    ap.add_argument('--ior', type=str, default=None,
                    help="index of refraction of the shell: a number (default 1.5) or a directory with ior.npy [V,1]")
    ap.add_argument('--shell', type=str, default=None,
                    help="thin glass shell instead of --ior: a directory with shell_ior.npy and shell_thickness.npy [V,1], or \"IOR,THICKNESS\"")
    ap.add_argument('--shell-curvature', dest='shell_curvature', type=str, default=None,
                    help="with --shell: curvature.npy [V,1] of the shell's vertices (extract_curvature) instead of the mesh's angle defect")
    ap.add_argument('--output', type=str, default=None, help="output directory (default data/relight/NAME)")
    ap.add_argument('--width', type=int, default=800)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--cam_dist', type=float, default=3.0)
    ap.add_argument('--num', type=int, default=360)
    ap.add_argument('--azimuth', type=float, default=0.0)
    ap.add_argument('--elevation', type=float, default=45.0)
    ap.add_argument('--focal_mm', type=float, default=50.0)
    ap.add_argument('--sensor_mm', type=float, default=36.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--chunk', type=int, default=256, help="samples per pass")
    flags = ap.parse_args(argv)
    if flags.samples < 2 or flags.samples % 2:
        ap.error("--samples must be even and >= 2")
    if flags.num < 1 or flags.width < 1 or flags.height < 1 or flags.chunk < 1:
        ap.error("--num, --width, --height and --chunk must be >= 1")
    if not flags.splitsum and (flags.pyramid is not None or flags.levels is not None):
        ap.error("--pyramid and --levels need --splitsum")
    if flags.transfer is not None and (not flags.splitsum or flags.inner is not None):
        ap.error("--transfer shadows the split-sum frame of the plain object: it needs --splitsum and excludes --inner")
    if flags.occlusion is not None and flags.transfer is None:
        ap.error("--occlusion needs --transfer")
    if flags.texture is not None and flags.inner is not None:
        ap.error("--texture holds the materials of the plain object: nested and thin-shell scenes (--inner) are not textured")
    if flags.normal_map:
        if flags.texture is None:
            ap.error("--normal-map needs --texture: the normals are in the atlas")
        path = os.path.join(flags.texture, 'atlas.npz')
        if os.path.exists(path):                               # a missing file is load_textures' error, as without --normal-map
            with np.load(path) as z:
                if 'normal' not in z.files:
                    ap.error(f"--normal-map: {path} has no normals (bake_textures --normals sdf writes them)")
    if flags.splitsum:
        if flags.inner is not None:
            ap.error("--splitsum renders the plain object only: nested and thin-shell scenes (--inner) keep the Monte-Carlo path")
        if (flags.hdr is None) == (flags.pyramid is None):
            ap.error("--splitsum takes exactly one of --hdr and --pyramid")
        if flags.levels is not None and (flags.pyramid is not None or any(r < 0.0 for r in flags.levels)
                                         or sorted(set(flags.levels)) != flags.levels or len(flags.levels) > MAX_LEVELS):
            ap.error(f"--levels needs --hdr and at most {MAX_LEVELS} ascending roughness values >= 0")
    if flags.shell is not None and flags.ior is not None:
        ap.error("--shell and --ior exclude each other: the shell is either the thin wall or solid glass")
    if flags.shell_curvature is not None and flags.shell is None:
        ap.error("--shell-curvature needs --shell")
    if flags.ior is None:
        flags.ior = '1.5'
    if flags.inner is None:
        if flags.inner_material is not None:
            ap.error("--inner-material needs --inner")
        if flags.shell is not None:
            ap.error("--shell needs --inner")
    else:
        if flags.inner_material is None:
            ap.error("--inner needs --inner-material")
        try:
            if flags.shell is not None:
                parse_shell(flags.shell)
            else:
                parse_ior(flags.ior)
        except ValueError as e:
            ap.error(str(e))
    return flags


def parse_ior(text):
    """--ior: a number >= 1 -> float, anything else -> the path DIR/ior.npy (a directory as extract_materials writes it)."""
    try:
        value = float(text)
    except ValueError:
        return os.path.join(text, 'ior.npy')
    if not np.isfinite(value) or value < 1.0:
        raise ValueError(f"--ior must be >= 1, got {text}")
    return value


def load_ior(spec, n_verts):
    """float32 [n_verts] from what parse_ior returns: the scalar repeated, or the [V,1] array of the file."""
    if isinstance(spec, float):
        return np.full(n_verts, spec, np.float32)
    a = np.load(spec)
    if a.size != n_verts or a.shape not in ((n_verts,), (n_verts, 1)):
        raise ValueError(f"{spec}: expected [{n_verts},1] (one index of refraction per vertex of the shell), got {a.shape}")
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def parse_shell(text):
    """--shell: "IOR,THICKNESS" (index > 0, thickness >= 0) -> (float, float); anything else -> the paths (DIR/shell_ior.npy,
    DIR/shell_thickness.npy) of a directory as extract_materials writes it."""
    parts = text.split(',')
    try:
        values = [float(p) for p in parts]
    except ValueError:
        return os.path.join(text, 'shell_ior.npy'), os.path.join(text, 'shell_thickness.npy')
    if len(values) != 2:
        raise ValueError(f"--shell takes a directory or two numbers IOR,THICKNESS, got {text}")
    if not np.isfinite(values).all() or values[0] <= 0.0 or values[1] < 0.0:
        raise ValueError(f"--shell needs IOR > 0 and THICKNESS >= 0, got {text}")
    return values[0], values[1]


def load_shell(spec, n_verts):
    """(ior, thickness) float32 [n_verts] each from what parse_shell returns."""
    return tuple(load_ior(v, n_verts) for v in spec)


def load_shell_curvature(path, n_verts):
    """--shell-curvature: float32 [n_verts] of a curvature.npy as extract_curvature writes it, clipped to [-10, 10] like the curvature the
    stage-2 model trains with (lbvh.Scene)."""
    a = np.load(path)
    if a.size != n_verts or a.shape not in ((n_verts,), (n_verts, 1)):
        raise ValueError(f"{path}: expected [{n_verts},1] (one curvature per vertex of the shell), got {a.shape}")
    return np.clip(np.ascontiguousarray(a, np.float32).reshape(-1), -10.0, 10.0)


def output_dir(flags):
    return flags.output or os.path.join('data', 'relight', flags.name)


def frame_path(out, k):
    return os.path.join(out, f'{k}.png')


def frames_to_render(out, num):
    """The frame numbers without a file yet (relight_backend.py:82)."""
    return [k for k in range(num) if not os.path.exists(frame_path(out, k))]


def load_materials(directory):
    return {k: np.load(os.path.join(directory, k + '.npy')) for k in ('metallic', 'roughness', 'albedo')}


def main(argv=None):
    flags = parse_args(argv)
    out = output_dir(flags)
    os.makedirs(out, exist_ok=True)
    todo = frames_to_render(out, flags.num)
    if not todo:
        print(f'{out}: all {flags.num} frames exist')
        return out
    from . import mesh as M
    V, F = M.read_ply(flags.mesh)
    if flags.trans:
        V = (np.asarray(V, np.float64) @ TRANS.T).astype(np.float32)
    if flags.inner is None:
        texture = None
        if flags.texture is not None:
            from .texture import load_textures
            texture = load_textures(flags.texture, len(F))
        scene = Scene(V, F, None if flags.material is None else load_materials(flags.material), texture=texture)
    else:
        Vi, Fi = M.read_ply(flags.inner)
        if flags.trans:
            Vi = (np.asarray(Vi, np.float64) @ TRANS.T).astype(np.float32)
        if flags.shell is not None:
            ior, thickness = load_shell(parse_shell(flags.shell), len(V))
            curvature = None if flags.shell_curvature is None else load_shell_curvature(flags.shell_curvature, len(V))
            scene = ThinShellScene(V, F, ior, thickness, Vi, Fi, load_materials(flags.inner_material), curvature=curvature)
        else:
            scene = NestedScene(V, F, load_ior(parse_ior(flags.ior), len(V)), Vi, Fi, load_materials(flags.inner_material))
    if flags.splitsum:
        print('--splitsum: --samples, --seed and --chunk are not used (nothing is sampled)')
        if flags.pyramid is not None:
            pyramid, levels, diffuse = load_pyramid_dir(flags.pyramid)
        else:
            from .environment import DEFAULT_LEVELS, prefilter
            levels = np.asarray(flags.levels or DEFAULT_LEVELS, np.float32)
            pyramid, diffuse, _ = prefilter(read_hdr(flags.hdr), levels)
        kw = {}
        if flags.transfer is not None:
            from .transfer import load_transfer_dir
            kw = {'transfer': load_transfer_dir(flags.transfer, len(V)), 'occlusion': flags.occlusion or 'ao'}
            if kw['occlusion'] == 'sh':
                if flags.pyramid is not None:
                    kw['env_sh'], source = load_env_sh(flags.pyramid)
                else:
                    from .environment import project_sh
                    kw['env_sh'], source = project_sh(read_hdr(flags.hdr)), flags.hdr
                print(f'--occlusion sh: environment SH coefficients from {source}')
    else:
        env = read_hdr(flags.hdr)
    poses = camera_in_mesh_frame(relighting_poses(flags.num, flags.azimuth, flags.elevation, flags.cam_dist))
    K = intrinsics(flags.height, flags.width, flags.focal_mm, flags.sensor_mm)
    for k in todo:
        if flags.splitsum:
            img = relight_splitsum(scene, None, None, pyramid, levels, diffuse, poses[k:k + 1], flags.height, flags.width, K=K,
                                   normal_map=flags.normal_map, **kw)
        elif flags.inner is None:
            img = relight(scene, None, None, env, poses[k:k + 1], flags.height, flags.width, flags.samples, flags.seed, flags.chunk, K=K, img0=k,
                          normal_map=flags.normal_map)
        else:
            img = relight_nested(scene, env, poses[k:k + 1], flags.height, flags.width, flags.samples, flags.seed, flags.chunk, K=K, img0=k)
        write_png(frame_path(out, k), img[0])
    print(f'wrote {len(todo)} frames to {out} ({flags.num - len(todo)} existed)')
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
