"""Independent restatements for the stage-2 mask tests: the erosion of mask_erosion.py (a sliding-window minimum over a 255-padded
array, i.e. OpenCV's default constant border for erosion, anchor k // 2) and the pixel rays of utils/render_mask_real.py:52-67 in
float64."""
import numpy as np


def erode_oracle(m, k):
    """uint8 [h,w] or [n,h,w] -> eroded + (max(m) - m) per image, as mask_erosion.py composes it."""
    m = np.asarray(m, np.uint8)
    if m.ndim == 3:
        return np.stack([erode_oracle(x, k) for x in m], 0)
    a, b = k // 2, k - 1 - k // 2
    pad = np.pad(m, ((a, b), (a, b)), mode='constant', constant_values=255)
    eroded = np.lib.stride_tricks.sliding_window_view(pad, (k, k)).min(axis=(2, 3))
    return (eroded.astype(np.int32) + (int(m.max()) - m.astype(np.int32))).astype(np.uint8)


def pinhole_rays64(Kinv, pose, h, w):
    """[h*w, 6] (origin, unit direction) in float64 for one image: c = (x + 0.5, y + 0.5, 1), d = normalize(R^T Kinv c),
    o = -R^T t; Kinv and the world -> camera pose [3,4] as given (their fp32 values, widened)."""
    Kinv, pose = np.asarray(Kinv, np.float64), np.asarray(pose, np.float64)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    c = np.stack([xs + 0.5, ys + 0.5, np.ones_like(xs)], -1).reshape(-1, 3)
    R, t = pose[:, :3], pose[:, 3]
    d = c @ Kinv.T @ R
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(-R.T @ t, d.shape)
    return np.concatenate([o, d], 1)
