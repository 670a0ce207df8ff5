"""Object-mask renderer on the HIP LBVH: drop-in for `utils/render_mask_synthetic.py:64-75`.

The reference builds, per training image, the pinhole rays of every pixel (`dirs = [(i - cx)/fx, -(j - cy)/fy, -1]` rotated by
the pose's 3x3, origin = the pose's translation; :52-66), traces them against the stage-1 mesh through OptiX
(`Scene.Dintersect`, :71) and writes `converged * 255` as an image (:72-74).  Here the tracing is `nu_lbvh_trace` (closest hit
with the semantics of cuda/triangle.cu:48-99); only the hit flag is needed, so no re-intersection runs.  Image files are
written without OpenCV (absent offline): binary PGM, or PNG/JPEG when Pillow is importable.

Real captures (utils/render_mask_real.py, mask_erosion.py): render_masks_real traces every pixel any-hit with the
rays made in registers (nu_mask_pinhole_trace), erode_masks is nu_mask_erode, and stage2_masks composes the two into the array the
non-zero-thickness stage 2 takes as imgs_info['mask'] under cfg get_mask.
"""
import os

import numpy as np
import torch

from .lbvh import LBVH


def pixel_directions(K, h, w, device):
    """Camera-space directions of every pixel, row-major [h*w, 3] (render_mask_synthetic.py:52-58: meshgrid over (w, h)
    transposed = x along columns, y along rows)."""
    K = torch.as_tensor(K, dtype=torch.float32, device=device)
    j, i = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device),
                          torch.arange(w, dtype=torch.float32, device=device), indexing='ij')
    return torch.stack([(i - K[0, 2]) / K[0, 0], -(j - K[1, 2]) / K[1, 1], -torch.ones_like(i)], -1).reshape(-1, 3)


@torch.no_grad()
def render_masks(vertices, faces, Ks, poses, h, w, bvh=None):
    """uint8 masks [n_img, h, w] (255 = the pixel's ray hits the mesh).  poses [n,3,4] camera-to-world (columns = axes,
    last column = centre), Ks [n,3,3] or one [3,3] shared by all images (the reference uses Ks[0] for every image, :57)."""
    dev = vertices.device
    bvh = bvh or LBVH(vertices, faces)
    poses = torch.as_tensor(poses, dtype=torch.float32, device=dev)
    Ks = torch.as_tensor(Ks, dtype=torch.float32, device=dev)
    K0 = Ks if Ks.dim() == 2 else Ks[0]
    dirs = pixel_directions(K0, h, w, dev)
    out = torch.empty(poses.shape[0], h, w, dtype=torch.uint8, device=dev)
    for n in range(poses.shape[0]):
        rays_d = dirs @ poses[n, :3, :3].T                       # sum(dirs[..., None, :] * R, -1)   (:66)
        rays_o = poses[n, :3, 3].expand_as(rays_d)
        hit, _ = bvh.intersect(torch.cat([rays_o, rays_d], 1))
        out[n] = (hit > 0).reshape(h, w).to(torch.uint8) * 255
    return out


def write_masks(masks, out_dir, names):
    """One image file per mask under out_dir (the reference writes <name>.jpg with cv2, :74)."""
    os.makedirs(out_dir, exist_ok=True)
    arr = masks.detach().cpu().numpy()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    paths = []
    for m, name in zip(arr, names):
        stem = os.path.splitext(name)[0]
        if Image is not None:
            path = os.path.join(out_dir, stem + '.png')
            Image.fromarray(np.repeat(m[:, :, None], 3, 2)).save(path)
        else:
            path = os.path.join(out_dir, stem + '.pgm')
            with open(path, 'wb') as fh:
                fh.write(b'P5\n%d %d\n255\n' % (m.shape[1], m.shape[0]))
                fh.write(m.tobytes())
        paths.append(path)
    return paths


# ---- real captures (render_mask.py -> utils/render_mask_real.py, then mask_erosion.py) ----------------------------------------------
def _cams(Ks, poses, device):
    """Per-image camera records of nu_mask_pinhole_trace: [n, 21] = Kinv (torch.inverse of the fp32 K, as render_mask_real.py:57 and
    renderer._construct_ray_batch compute it) then the world -> camera [R|t], both row-major."""
    Ks = torch.as_tensor(np.asarray(Ks) if not torch.is_tensor(Ks) else Ks).to(device=device, dtype=torch.float32)
    poses = torch.as_tensor(np.asarray(poses) if not torch.is_tensor(poses) else poses).to(device=device, dtype=torch.float32)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be [n,3,4] world-to-camera, got {tuple(poses.shape)}")
    if Ks.dim() == 2:
        Ks = Ks.expand(poses.shape[0], 3, 3)
    if tuple(Ks.shape) != (poses.shape[0], 3, 3):
        raise ValueError(f"Ks must be [3,3] or [n,3,3] for {poses.shape[0]} poses, got {tuple(Ks.shape)}")
    Kinv = torch.inverse(Ks)
    return torch.cat([Kinv.reshape(-1, 9), poses.reshape(-1, 12)], 1).contiguous()


def pinhole_rays(Ks, poses, h, w, device=None):
    """The rays nu_mask_pinhole_trace traces, as [n*h*w, 6] (origin, unit direction), pixel-major per image (tests)."""
    from . import _lib as L
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    cams = _cams(Ks, poses, dev)
    L.require_cuda(cams)
    rays = torch.empty(cams.shape[0] * h * w, 6, dtype=torch.float32, device=dev)
    L.load().nu_mask_pinhole_rays(L.ptr(cams), int(cams.shape[0]), int(h), int(w), L.ptr(rays), L.stream())
    return rays


@torch.no_grad()
def render_masks_real(vertices, faces, Ks, poses, h, w, bvh=None, chunk=None):
    """uint8 masks [n, h, w] of real captures (255 = the pixel's ray hits the mesh): utils/render_mask_real.py's rays -- pixel
    centres, K^-1, world -> camera poses [n,3,4], unit directions -- traced any-hit by nu_mask_pinhole_trace, rays made in registers.
    Ks [n,3,3] (or one [3,3] for all).  chunk=None renders every image in one launch and returns the masks on the mesh's device;
    chunk=c renders c images per launch and gathers them on the host, so at most c masks are on the device at a time."""
    from . import _lib as L
    dev = vertices.device
    bvh = bvh or LBVH(vertices, faces)
    cams = _cams(Ks, poses, dev)
    n, h, w = int(cams.shape[0]), int(h), int(w)
    lib = L.load()
    if chunk is None:
        out = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
        lib.nu_mask_pinhole_trace(L.ptr(bvh.buf), bvh.n_faces, L.ptr(cams), n, h, w, L.ptr(out), L.stream())
        return out
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    out = torch.empty(n, h, w, dtype=torch.uint8)
    part = torch.empty(min(chunk, n), h, w, dtype=torch.uint8, device=dev)
    for i in range(0, n, chunk):
        c = min(chunk, n - i)
        lib.nu_mask_pinhole_trace(L.ptr(bvh.buf), bvh.n_faces, L.ptr(cams[i:i + c]), c, h, w, L.ptr(part), L.stream())
        out[i:i + c].copy_(part[:c])
    return out


@torch.no_grad()
def erode_masks(masks, erosion=15):
    """mask_erosion.py on the GPU: uint8 [n,h,w] -> uint8 [n,h,w] = erode(m, erosion x erosion box) + (max(m) - m) per image
    (nu_mask_erode: anchor erosion // 2, outside positions left out -- OpenCV's default border, see csrc/mask.hip).  For a binary
    mask: 255 in the background and the eroded interior, 0 in the band just inside the silhouette; an all-zero mask stays all 0.
    A CPU input is eroded on the current device and returned on the CPU."""
    from . import _lib as L
    if not torch.is_tensor(masks):
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if masks.dtype != torch.uint8 or masks.dim() != 3:
        raise ValueError(f"erode_masks: masks must be uint8 [n,h,w], got {masks.dtype} {tuple(masks.shape)}")
    erosion = int(erosion)
    if erosion < 1:
        raise ValueError(f"erode_masks: the box size must be >= 1, got {erosion}")
    host = not masks.is_cuda
    m = (masks.to(torch.device('cuda', torch.cuda.current_device())) if host else masks).contiguous()
    n, h, w = (int(s) for s in m.shape)
    out = torch.empty_like(m)
    if n == 0 or h == 0 or w == 0:
        return out.cpu() if host else out
    lib = L.load()
    nbytes = lib.nu_mask_erode_workspace_bytes(n, h, w)
    work = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    lib.nu_mask_erode(L.ptr(m), n, h, w, erosion, L.ptr(work), nbytes, L.ptr(out), L.stream())
    return out.cpu() if host else out


@torch.no_grad()
def stage2_masks(vertices, faces, Ks, poses, h, w, erosion=15, bvh=None, chunk=None):
    """float32 [n,h,w,1] in [0,1]: erode_masks(render_masks_real(...)) / 255, the array the reference's get_mask returns
    (dataset/database.py:531-533) for the non-zero-thickness stage 2 (cfg get_mask).  The one deliberate difference: the reference
    goes through mask/*.jpg and mask_erosion/*.jpg on disk, so its values carry JPEG noise; these are exactly 0 or 1.
    chunk as render_masks_real (the result then lives on the host)."""
    bvh = bvh or LBVH(vertices, faces)
    if chunk is None:
        m = erode_masks(render_masks_real(vertices, faces, Ks, poses, h, w, bvh=bvh), erosion)
        return (m.to(torch.float32) / 255.0)[..., None]
    Ks_t = torch.as_tensor(np.asarray(Ks) if not torch.is_tensor(Ks) else Ks)
    poses_t = torch.as_tensor(np.asarray(poses) if not torch.is_tensor(poses) else poses)
    cams_n = int(poses_t.shape[0])
    out = torch.empty(cams_n, h, w, 1, dtype=torch.float32)
    for i in range(0, cams_n, int(chunk)):
        c = min(int(chunk), cams_n - i)
        K_i = Ks_t if Ks_t.dim() == 2 else Ks_t[i:i + c]
        m = erode_masks(render_masks_real(vertices, faces, K_i, poses_t[i:i + c], h, w, bvh=bvh), erosion)
        out[i:i + c, ..., 0].copy_(m.to(torch.float32) / 255.0)
    return out


def write_mask_jpegs(masks, out_dir, names):
    """<out_dir>/<stem>.jpg per mask, three equal channels at JPEG quality 95 (what cv2.imwrite writes by default,
    render_mask_real.py:76).  Needs Pillow."""
    Image = _pillow()
    os.makedirs(out_dir, exist_ok=True)
    arr = masks.detach().cpu().numpy() if torch.is_tensor(masks) else np.asarray(masks)
    paths = []
    for m, name in zip(arr, names):
        path = os.path.join(out_dir, os.path.splitext(name)[0] + '.jpg')
        Image.fromarray(np.repeat(m[:, :, None], 3, 2)).save(path, quality=95)
        paths.append(path)
    return paths


def _pillow():
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("writing and reading mask images needs Pillow (pip install pillow); cv2 is not used") from e
    return Image


def read_mask_image(path):
    """Channel 0 of a mask image as uint8 [h,w] (what the reference's get_mask reads, dataset/database.py:531-533)."""
    Image = _pillow()
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8:
        raise ValueError(f"{path}: expected an 8-bit image, got {a.dtype}")
    return np.ascontiguousarray(a[..., 0] if a.ndim == 3 else a)


def write_mask_image(path, m):
    """uint8 [h,w] as three equal channels; JPEG (by the file name) at quality 95, cv2.imwrite's default."""
    Image = _pillow()
    img = Image.fromarray(np.repeat(np.asarray(m, np.uint8)[:, :, None], 3, 2))
    if os.path.splitext(path)[1].lower() in ('.jpg', '.jpeg'):
        img.save(path, quality=95)
    else:
        img.save(path)
    return path


def load_database_split(cfg, module):
    """(database, train ids) from the user's NU-NeRF checkout: dataset/<module>.py imported at run time, as compat imports
    dataset.database.  module 'database_formask' -> CustomDatabase (render_mask_real.py:10-11), 'database' -> NeRFSyntheticDatabase
    (render_mask_synthetic.py:10-11)."""
    import importlib
    name = cfg['database_name']
    try:
        mod = importlib.import_module('dataset.' + module)          # the user's NU-NeRF checkout
    except ImportError as e:
        raise ImportError(f"the --cfg mode needs the NU-NeRF checkout on PYTHONPATH (its dataset/{module}.py loads the image "
                          f"database '{name}'): PYTHONPATH=<repo>:<NU-NeRF checkout>; or pass --cameras NPZ --out DIR") from e
    cls = mod.CustomDatabase if module == 'database_formask' else mod.NeRFSyntheticDatabase
    database = cls(name, cfg['dataset_dir'])
    train_ids, _ = mod.get_database_split(database)
    return database, list(train_ids)


def object_dir(cfg):
    """<dataset_dir>/<object>: the object name is database_name.split('/')[-1] for NeRF-synthetic data, [-2] for real captures
    (render_mask_*.py, mask_erosion.py:15-20)."""
    return os.path.join(cfg['dataset_dir'], cfg['database_name'].split('/')[-1 if cfg['is_nerf'] else -2])
