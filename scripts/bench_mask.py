"""Report aid: stage-2 mask rendering and erosion of real captures at 1080 x 1920.

  nu_mask_pinhole_trace   fused pixel rays + any-hit LBVH, uint8 mask out (mask_render.render_masks_real)
  baseline                the same rays made in torch as render_mask_real.py makes them, traced closest-hit by nu_lbvh_trace
                          (reported with and without the torch ray generation)
  nu_mask_erode           k = 15 (mask_render.erode_masks)
on icospheres of 20 480 and 327 680 faces seen by a ring of cameras; ms per image, GPU events, median of the repeats."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from nu_nerf_amd.lbvh import LBVH, icosphere
from nu_nerf_amd.mask_render import erode_masks, pinhole_rays, render_masks_real

H, W, N_IMG, REPS = 1080, 1920, 8, 5
dev = torch.device('cuda:0')


def ring_cameras(n):
    Ks, poses = [], []
    for i in range(n):
        a = 2 * np.pi * i / n
        eye = np.array([1.8 * np.cos(a), 0.4 * np.sin(3 * a), 1.8 * np.sin(a)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 1.0, 0.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        poses.append(np.concatenate([R, (-R @ eye)[:, None]], 1))
        Ks.append([[1600.0, 0, W / 2 + 13.0], [0, 1580.0, H / 2 - 7.0], [0, 0, 1]])
    return np.asarray(Ks, np.float32), np.asarray(poses, np.float32)


def torch_rays(Ks, poses):
    """render_mask_real.py:52-67 in torch on the device."""
    Ks, poses = torch.from_numpy(Ks).to(dev), torch.from_numpy(poses).to(dev)
    n = Ks.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    c = torch.cat([torch.stack([xs, ys], -1).float().reshape(1, H * W, 2) + 0.5, torch.ones(1, H * W, 1, device=dev)], 2)
    d = F.normalize((c @ torch.inverse(Ks).permute(0, 2, 1)) @ poses[:, :, :3], dim=-1)
    o = (-poses[:, :, :3].permute(0, 2, 1) @ poses[:, :, 3:]).permute(0, 2, 1).expand(n, H * W, 3)
    return torch.cat([o, d], 2).reshape(-1, 6).contiguous()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


Ks, poses = ring_cameras(N_IMG)
print(f"{N_IMG} images of {H} x {W} per launch; ms per image (median of {REPS})")
for sub in (5, 7):
    V, Fc = icosphere(sub, 0.5)
    Vt, Ft = torch.from_numpy(V).to(dev), torch.from_numpy(Fc).to(dev)
    bvh = LBVH(Vt, Ft)
    masks = render_masks_real(Vt, Ft, Ks, poses, H, W, bvh=bvh)
    hit, _ = bvh.intersect(pinhole_rays(Ks, poses, H, W, device=dev))           # the kernel's own rays, closest hit
    same = torch.equal(masks.reshape(-1), (hit > 0).to(torch.uint8) * 255)
    rays = torch_rays(Ks, poses)
    hit, _ = bvh.intersect(rays)
    n_diff = int((masks.reshape(-1) != (hit > 0).to(torch.uint8) * 255).sum())  # torch's rays round differently at the silhouette
    t_fused = timed(lambda: render_masks_real(Vt, Ft, Ks, poses, H, W, bvh=bvh))
    t_trace = timed(lambda: bvh.intersect(rays))
    t_both = timed(lambda: bvh.intersect(torch_rays(Ks, poses)))
    print(f"faces {Fc.shape[0]:6d}  hit frac {float((masks > 0).float().mean()):.3f}  fused any-hit {t_fused / N_IMG:7.3f}  "
          f"nu_lbvh_trace on torch rays {t_trace / N_IMG:7.3f} (+ ray generation {t_both / N_IMG:7.3f})  "
          f"masks equal nu_lbvh_trace on the same rays: {same}; pixels that differ on the torch rays: {n_diff}")
    del rays, hit
    torch.cuda.empty_cache()
t_erode = timed(lambda: erode_masks(masks, 15))
print(f"nu_mask_erode k = 15: {t_erode / N_IMG:7.3f} ms per image ({5 * H * W / (t_erode / N_IMG) / 1e6:6.1f} GB/s counting five "
      f"image-sized transfers: the row pass reads the mask and writes the workspace, the column pass reads both and writes the output)")
