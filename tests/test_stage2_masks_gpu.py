"""Stage-2 masks of real captures on the GPU: nu_mask_pinhole_rays / nu_mask_pinhole_trace (render_mask_real.py's rays, any-hit
LBVH) against float64 rays, nu_lbvh_trace and nu_brute_trace bit for bit; nu_mask_erode against the numpy oracle byte for byte;
the get_mask path of the non-zero-thickness stage 2 (training and eval); the two command lines."""
import math
import os

import numpy as np
import pytest
import torch

from mask_oracle import erode_oracle, pinhole_rays64

pytestmark = pytest.mark.gpu


def _look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """World -> camera [R|t] (OpenCV axes: x right, y down, z forward) of a camera at `eye` looking at `target`."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(z, (1.0, 0.0, 0.0))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)
    return np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32)


def _cameras(n, h, w, seed, dist=(1.4, 2.5)):
    g = np.random.Generator(np.random.PCG64(seed))
    Ks, poses = [], []
    for i in range(n):
        fx = g.uniform(0.8, 1.4) * w
        fy = fx * g.uniform(0.7, 1.3)                          # non-square pixels
        cx, cy = w * g.uniform(0.3, 0.7), h * g.uniform(0.3, 0.7)   # off-centre principal point
        Ks.append(np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float32))
        v = g.normal(size=3)
        poses.append(_look_at(v / np.linalg.norm(v) * g.uniform(*dist), target=g.normal(size=3) * 0.05))
    return np.stack(Ks), np.stack(poses)


def _mesh(gpu, subdiv, radius=0.5):
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(subdiv, radius)
    return torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)


def _three_ways(gpu, V, F, Ks, poses, h, w):
    from nu_nerf_amd.lbvh import LBVH
    from nu_nerf_amd.mask_render import pinhole_rays, render_masks_real
    bvh = LBVH(V, F)
    m = render_masks_real(V, F, Ks, poses, h, w, bvh=bvh)
    rays = pinhole_rays(Ks, poses, h, w, device=gpu)
    hit_l, _ = bvh.intersect(rays)
    hit_b, _ = bvh.intersect_brute(rays)
    n = poses.shape[0]
    lb = ((hit_l > 0).to(torch.uint8) * 255).reshape(n, h, w)
    br = ((hit_b > 0).to(torch.uint8) * 255).reshape(n, h, w)
    assert m.dtype == torch.uint8 and m.shape == (n, h, w)
    assert torch.equal(m, lb)
    assert torch.equal(m, br)
    return m


def test_pinhole_rays_match_float64_restatement(gpu):
    from nu_nerf_amd.mask_render import _cams, pinhole_rays
    for (h, w), seed in (((13, 21), 1), ((7, 9), 2), ((31, 5), 3)):
        Ks, poses = _cameras(3, h, w, seed)
        rays = pinhole_rays(Ks, poses, h, w, device=gpu).cpu().numpy().astype(np.float64).reshape(3, h * w, 6)
        cams = _cams(Ks, poses, gpu).cpu().numpy()
        for i in range(3):
            ref = pinhole_rays64(cams[i, :9].reshape(3, 3), cams[i, 9:].reshape(3, 4), h, w)
            o_err = np.linalg.norm(rays[i, :, :3] - ref[:, :3], axis=1) / np.linalg.norm(ref[:, :3], axis=1)
            d_err = np.linalg.norm(rays[i, :, 3:] - ref[:, 3:], axis=1)
            assert o_err.max() <= 1e-6 and d_err.max() <= 1e-6, (h, w, i, o_err.max(), d_err.max())
        # Kinv is torch.inverse of the fp32 K, as the reference and renderer._construct_ray_batch compute it
        np.testing.assert_array_equal(cams[:, :9].reshape(-1, 3, 3), torch.inverse(torch.from_numpy(Ks).to(gpu)).cpu().numpy())


@pytest.mark.parametrize("subdiv,h,w", [(2, 37, 53), (5, 45, 61)])
def test_mask_trace_bit_exact_three_ways_icospheres(gpu, subdiv, h, w):
    V, F = _mesh(gpu, subdiv)
    Ks, poses = _cameras(3, h, w, seed=10 + subdiv)
    m = _three_ways(gpu, V, F, Ks, poses, h, w)
    frac = float((m > 0).float().mean())
    assert 0.05 < frac < 0.95                                   # silhouettes inside the frames


def test_mask_trace_bit_exact_three_ways_327680_faces(gpu):
    V, F = _mesh(gpu, 7)
    assert F.shape[0] == 327680
    Ks, poses = _cameras(1, 29, 43, seed=7)
    _three_ways(gpu, V, F, Ks, poses, 29, 43)


def test_mask_trace_bit_exact_three_ways_triangle_soup(gpu):
    from test_closest_point_gpu import _soup          # random triangles, exact duplicates (ties), zero-area kinds, slivers
    V, F = _soup()
    V, F = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    Ks, poses = _cameras(3, 41, 57, seed=5, dist=(1.2, 1.8))
    m = _three_ways(gpu, V, F, Ks, poses, 41, 57)
    assert bool((m > 0).any()) and bool((m == 0).any())


def test_mask_camera_looking_away_and_camera_inside(gpu):
    V, F = _mesh(gpu, 3)
    K = np.array([[30.0, 0, 16.0], [0, 28.0, 10.0], [0, 0, 1.0]], np.float32)
    away = _look_at((0.0, 0.0, 2.0), target=(0.0, 0.0, 5.0))
    inside = _look_at((0.05, -0.02, 0.1), target=(1.0, 0.3, 0.0))
    m = _three_ways(gpu, V, F, np.stack([K, K]), np.stack([away, inside]), 23, 33)
    assert not bool(m[0].any())
    assert bool((m[1] == 255).all())


def test_mask_trace_matches_the_sphere_away_from_the_silhouette(gpu):
    from nu_nerf_amd.mask_render import pinhole_rays, render_masks_real
    r = 0.5
    V, F = _mesh(gpu, 5, r)
    Vn, Fn = V.double().cpu().numpy(), F.long().cpu().numpy()
    tri = Vn[Fn]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs((nrm * tri[:, 0]).sum(1)) / np.linalg.norm(nrm, axis=1)
    chord = r - plane.min()                                     # the inscribed mesh lies within `chord` inside the sphere
    h, w = 64, 80
    Ks, poses = _cameras(2, h, w, seed=21)
    m = render_masks_real(V, F, Ks, poses, h, w).cpu().numpy().reshape(-1)
    rays = pinhole_rays(Ks, poses, h, w, device=gpu).double().cpu().numpy()
    rho = np.linalg.norm(np.cross(rays[:, :3], rays[:, 3:]), axis=1)        # distance of the ray's line from the centre
    front = (-(rays[:, :3] * rays[:, 3:]).sum(1)) > 0                        # the centre lies ahead of every camera here
    assert front.all()
    inside, outside = rho < r - 2 * chord, rho > r * (1 + 1e-5)
    assert inside.sum() > 100 and outside.sum() > 100
    assert (m[inside] == 255).all() and (m[outside] == 0).all()


def _erosion_batch(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    ys, xs = np.mgrid[:h, :w]
    disk = ((((xs - w * 0.45) / (w * 0.3)) ** 2 + ((ys - h * 0.55) / (h * 0.35)) ** 2) < 1).astype(np.uint8) * 255
    binary = (g.uniform(size=(h, w)) < 0.8).astype(np.uint8) * 255
    return np.stack([disk, binary, g.integers(0, 256, (h, w), dtype=np.uint8), np.zeros((h, w), np.uint8),
                     g.integers(0, 120, (h, w), dtype=np.uint8)])


@pytest.mark.parametrize("h,w", [(37, 53), (9, 11), (67, 1031)])
@pytest.mark.parametrize("k", [1, 2, 3, 15, 31])
def test_erode_equals_the_oracle_byte_for_byte(gpu, h, w, k):
    from nu_nerf_amd.mask_render import erode_masks
    m = _erosion_batch(h, w, seed=h * 1000 + w + k)
    out = erode_masks(torch.from_numpy(m).to(gpu), k)
    assert out.is_cuda and out.dtype == torch.uint8
    np.testing.assert_array_equal(out.cpu().numpy(), erode_oracle(m, k))


@pytest.mark.parametrize("n,h,w,k", [(2, 150, 19, 101), (1, 3, 4200, 4099), (3, 1, 1, 5)])
def test_erode_windows_beyond_one_lds_chunk(gpu, n, h, w, k):
    """Windows longer than one LDS chunk of either pass (columns: 64 rows, rows: 4096 bytes), and 1 x 1 images."""
    from nu_nerf_amd.mask_render import erode_masks
    m = _erosion_batch(h, w, seed=k)[:n]
    np.testing.assert_array_equal(erode_masks(torch.from_numpy(m).to(gpu), k).cpu().numpy(), erode_oracle(m, k))


def test_erode_rejects_an_empty_box(gpu):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd.mask_render import erode_masks
    m = torch.zeros(1, 4, 4, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        erode_masks(m, 0)
    lib = L.load()
    nbytes = lib.nu_mask_erode_workspace_bytes(1, 4, 4)
    work = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    out = torch.empty_like(m)
    with pytest.raises(L.NuNerfLibraryError):
        lib.nu_mask_erode(L.ptr(m), 1, 4, 4, 0, L.ptr(work), nbytes, L.ptr(out), L.stream())


def test_stage2_masks_is_the_eroded_render_over_255(gpu):
    from nu_nerf_amd.mask_render import erode_masks, render_masks_real, stage2_masks
    V, F = _mesh(gpu, 4)
    Ks, poses = _cameras(3, 47, 59, seed=31)
    s = stage2_masks(V, F, Ks, poses, 47, 59, erosion=7)
    ref = erode_masks(render_masks_real(V, F, Ks, poses, 47, 59), 7).to(torch.float32) / 255.0
    assert s.dtype == torch.float32 and s.shape == (3, 47, 59, 1)
    assert torch.equal(s[..., 0], ref)
    assert set(torch.unique(s).tolist()) == {0.0, 1.0}
    chunked = stage2_masks(V, F, torch.from_numpy(Ks), torch.from_numpy(poses), 47, 59, erosion=7, chunk=2)
    assert not chunked.is_cuda and torch.equal(chunked, s.cpu())
    assert torch.equal(render_masks_real(V, F, Ks, poses, 47, 59, chunk=2), render_masks_real(V, F, Ks, poses, 47, 59).cpu())


# ---- get_mask in the non-zero-thickness stage 2 --------------------------------------------------------------------------------
def _thick_net(gpu, get_mask, seed=0, downsample=1.0, rgb_loss='charbonier'):
    from nu_nerf_amd.stage2_thick import name2renderer
    from nu_nerf_amd.lbvh import icosphere
    shader = {'sphere_direction': True, 'human_light': False, 'light_exp_max': 5.0}
    cfg = {'name': 's2t', 'network': 'stage2', 'get_mask': get_mask, 'database_name': 'real/bear', 'is_nerf': False,
           'shader_config': shader, 'train_ray_num': 32, 'test_ray_num': 64, 'downsample_ratio': downsample, 'rgb_loss': rgb_loss,
           'stage1_cfg': {'name': 's1', 'network': 'shape', 'get_mask': False, 'is_nerf': False, 'shader_config': shader},
           'stage1_mesh_arrays': icosphere(2, 0.5)}
    torch.manual_seed(seed)
    return name2renderer['stage2'](cfg, training=True).to(gpu)


def _real_store(gpu, mask, n=2, h=6, w=8):
    g = torch.Generator().manual_seed(4)
    K = torch.tensor([[7.0, 0, 4.0], [0, 7.5, 3.0], [0, 0, 1.0]])
    poses = torch.stack([torch.from_numpy(_look_at((0.3 * i, 0.2, 2.5))) for i in range(n)])
    info = {'imgs': torch.rand(n, 3, h, w, generator=g).to(gpu), 'Ks': K.expand(n, 3, 3).clone().to(gpu), 'poses': poses.to(gpu)}
    if mask is not None:
        info['mask'] = mask.to(gpu)
    return info


def _pixel_parity_mask(n=2, h=6, w=8):
    return (torch.arange(n * h * w).reshape(n, h, w, 1) % 2).float()


@pytest.mark.parametrize("rgb_loss", ['l2', 'charbonier'])
def test_all_zero_mask_gives_zero_rgb_loss_and_gradient(gpu, rgb_loss):
    net = _thick_net(gpu, True, rgb_loss=rgb_loss)
    net.set_ray_store(_real_store(gpu, torch.zeros(2, 6, 8, 1)))
    net.zero_grad(set_to_none=True)
    out = net({'step': 6000})
    # every ray's residual is 0: l2 gives 0, the default Charbonnier its constant sqrt(0 + 0.001)
    floor = 0.0 if rgb_loss == 'l2' else float(torch.sqrt(torch.zeros(1, device=gpu) + 0.001))
    assert bool((out['loss_rgb'] == floor).all())
    out['loss_rgb'].mean().backward()
    for name, p in net.named_parameters():
        assert p.grad is None or float(p.grad.abs().sum()) == 0.0, name


def test_half_zero_mask_weights_the_rgb_loss_as_the_reference(gpu):
    net = _thick_net(gpu, True)
    net.set_ray_store(_real_store(gpu, _pixel_parity_mask()))
    i, rn = net.train_batch_i, net.cfg['train_ray_num']
    mask = net.train_batch['mask'][i:i + rn].clone()
    rgbs = net.train_batch['rgbs'][i:i + rn].clone()
    assert bool((mask == 0).any()) and bool((mask == 1).any())
    out = net({'step': 6000})
    tir = out['tir_mask'].detach().float()
    ref = net.compute_rgb_loss(out['ray_rgb'] * tir * mask, rgbs * tir * mask)       # renderer.py:1326-1330
    assert torch.equal(out['loss_rgb'], ref)
    floor = net.compute_rgb_loss(torch.zeros(1, 3, device=gpu), torch.zeros(1, 3, device=gpu))     # a zero residual
    assert bool((out['loss_rgb'][mask[:, 0] == 0] == floor).all())


def test_get_mask_false_ignores_a_present_mask_bit_for_bit(gpu):
    outs = []
    for with_mask in (True, False):
        net = _thick_net(gpu, False, seed=3)
        net.set_ray_store(_real_store(gpu, _pixel_parity_mask() if with_mask else None))
        assert 'mask' not in net.train_batch
        torch.manual_seed(9)
        net.zero_grad(set_to_none=True)
        out = net({'step': 6000})
        out['loss_rgb'].mean().backward()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        outs.append((out['ray_rgb'].detach().clone(), out['loss_rgb'].detach().clone(), grads))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2]) and len(outs[0][2]) > 0
    for n in outs[0][2]:
        torch.testing.assert_close(outs[0][2][n], outs[1][2][n], rtol=1e-5, atol=0.0, msg=n)


@pytest.mark.parametrize("ratio", [1.0, 0.5])
def test_eval_masks_ray_rgb_and_gt_rgb_with_the_test_mask(gpu, ratio):
    import torch.nn.functional as F
    net = _thick_net(gpu, True, downsample=ratio)
    mask = _pixel_parity_mask(h=12, w=16)
    mask[1, :6] = 1.0
    info = _real_store(gpu, mask, h=12, w=16)
    net.set_ray_store(info, test_imgs_info=info)
    with torch.no_grad():
        ev = net({'index': 1, 'eval': True, 'step': 0})
    h, w = int(12 * ratio), int(16 * ratio)
    m = F.interpolate(mask[1:2].reshape(1, 1, 12, 16), size=(h, w), mode='nearest').reshape(h, w).to(gpu)
    assert ev['ray_rgb'].shape == (h, w, 3) and ev['gt_rgb'].shape == (h, w, 3)
    assert bool((ev['ray_rgb'][m == 0] == 0).all()) and bool((ev['gt_rgb'][m == 0] == 0).all())
    assert bool((ev['gt_rgb'][m == 1] != 0).any())


# ---- command lines ----------------------------------------------------------------------------------------------------------
def test_render_mask_and_mask_erosion_command_lines(gpu, tmp_path):
    from PIL import Image
    from nu_nerf_amd import mesh, render_mask, mask_erosion
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import erode_masks, render_masks_real
    V, F = icosphere(4, 0.5)
    mesh.write_ply(str(tmp_path / 'mesh.ply'), V, F)
    h, w = 45, 67
    Ks, poses = _cameras(3, h, w, seed=41)
    names = np.array(['img_000.png', 'img_001.png', 'img_002.png'])
    np.savez(tmp_path / 'cams.npz', Ks=Ks, poses=poses, names=names, h=h, w=w)
    render_mask.main(['--cameras', str(tmp_path / 'cams.npz'), '--mesh_path', str(tmp_path / 'mesh.ply'),
                      '--out', str(tmp_path / 'mask'), '--chunk', '2'])
    Vt, Ft = torch.from_numpy(V).to(gpu), torch.from_numpy(F).to(gpu)
    ref = render_masks_real(Vt, Ft, Ks, poses, h, w).cpu().numpy()
    assert sorted(os.listdir(tmp_path / 'mask')) == ['img_000.jpg', 'img_001.jpg', 'img_002.jpg']
    dec = []
    for i in range(3):
        a = np.asarray(Image.open(tmp_path / 'mask' / f'img_00{i}.jpg'))
        assert a.shape == (h, w, 3)
        assert np.abs(a[..., 0].astype(int) - ref[i]).max() <= 24          # JPEG error of a 0 / 255 image at quality 95
        dec.append(a[..., 0])
    mask_erosion.main(['--mask-dir', str(tmp_path / 'mask'), '--out-dir', str(tmp_path / 'mask_erosion'), '--erosion', '5'])
    want = erode_masks(torch.from_numpy(np.stack(dec)).to(gpu), 5).cpu().numpy()
    for i in range(3):
        a = np.asarray(Image.open(tmp_path / 'mask_erosion' / f'img_00{i}.jpg'))[..., 0]
        assert np.abs(a.astype(int) - want[i]).max() <= 24
