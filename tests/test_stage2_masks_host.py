"""Stage-2 masks of real captures, host side: the erosion oracle against hand-worked cases, the compat dataset hook's get_mask
branch, and the per-ray mask of the non-zero-thickness model's ray store (no GPU)."""
import sys
import types

import numpy as np
import pytest
import torch

from mask_oracle import erode_oracle


def test_erosion_oracle_even_box_uses_the_asymmetric_anchor():
    # k = 2: anchor 1, window [x - 1, x]: the band lands right of (and below) the hole, not left of it
    m = np.array([[255, 0, 255, 255]], np.uint8)
    assert erode_oracle(m, 2).tolist() == [[255, 255, 0, 255]]
    assert erode_oracle(m.T, 2).T.tolist() == [[255, 255, 0, 255]]
    # k = 4: anchor 2, window [x - 2, x + 1]
    m = np.array([[255, 255, 255, 0, 255, 255, 255, 255]], np.uint8)
    assert erode_oracle(m, 4).tolist() == [[255, 255, 0, 255, 0, 0, 255, 255]]


def test_erosion_oracle_box_larger_than_the_image():
    m = np.full((3, 3), 255, np.uint8)
    m[0, 0] = 0
    out = erode_oracle(m, 7)                      # every window covers the whole image: eroded = 0 -> out = 255 - m
    assert out.tolist() == [[255, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert erode_oracle(np.full((2, 3), 255, np.uint8), 9).tolist() == [[255] * 3] * 2     # the border is 255, not 0


def test_erosion_oracle_box_of_one_gives_the_maximum_everywhere():
    m = np.array([[0, 7, 255], [3, 0, 9]], np.uint8)
    assert erode_oracle(m, 1).tolist() == [[255] * 3] * 2


def test_erosion_oracle_all_zero_image_stays_zero():
    assert not erode_oracle(np.zeros((5, 4), np.uint8), 3).any()


def test_erosion_oracle_non_binary_image():
    m = np.array([[10, 200], [50, 100]], np.uint8)
    # k = 3 covers the image from every pixel: eroded = 10, max = 200 -> 10 + 200 - m
    assert erode_oracle(m, 3).tolist() == [[200, 10], [160, 110]]
    # k = 2, window [y - 1, y] x [x - 1, x]
    assert erode_oracle(m, 2).tolist() == [[200, 10], [160, 110]]
    m = np.array([[9, 4, 7]], np.uint8)
    assert erode_oracle(m, 2).tolist() == [[9, 4 + 5, 4 + 2]]


class _MaskDatabase:
    """Interface double of dataset/database.py's CustomDatabase with get_mask (database.py:531-533: [h,w,1] in [0,1])."""
    h, w, n = 3, 4, 5

    def __init__(self, name, dataset_dir):
        self.name = name

    def get_img_ids(self): return [str(i) for i in range(self.n)]
    def get_image(self, i): return np.full((self.h, self.w, 3), 10 * int(i), np.uint8)
    def get_K(self, i): return np.array([[10.0, 0, 2.0], [0, 10.0, 1.5], [0, 0, 1.0]])
    def get_pose(self, i): return np.concatenate([np.eye(3), np.array([[0.0], [0.0], [3.0]])], 1)
    def get_depth(self, i): return np.ones((self.h, self.w), np.float32), np.ones((self.h, self.w), np.bool_)

    def get_mask(self, i):
        return ((np.arange(self.h * self.w).reshape(self.h, self.w, 1) + int(i)) % 2 * 255) / 255.0


def test_compat_build_imgs_info_returns_the_eroded_mask():
    from nu_nerf_amd.compat._dataset import build_imgs_info, imgs_info_to_torch
    db = _MaskDatabase('custom/fake/8', '.')
    ids = db.get_img_ids()
    info = build_imgs_info(db, ids, False, s2_mask=True)
    assert info['mask'].dtype == np.float32 and info['mask'].shape == (5, 3, 4, 1)
    np.testing.assert_array_equal(info['mask'], np.stack([db.get_mask(i) for i in ids]).astype(np.float32))
    assert 'mask' not in build_imgs_info(db, ids, False)                      # the default keeps today's keys
    assert imgs_info_to_torch(info)['mask'].shape == (5, 3, 4, 1)


@pytest.mark.parametrize("get_mask", [True, False, None])
def test_compat_init_dataset_passes_get_mask(monkeypatch, get_mask):
    from nu_nerf_amd.compat._dataset import ReferenceDatasetMixin
    mod = types.ModuleType('dataset.database')
    mod.parse_database_name = lambda name, d: _MaskDatabase(name, d)
    mod.get_database_split = lambda db, split_type='validation': (db.get_img_ids()[:3], db.get_img_ids()[3:])
    pkg = types.ModuleType('dataset')
    pkg.database = mod
    monkeypatch.setitem(sys.modules, 'dataset', pkg)
    monkeypatch.setitem(sys.modules, 'dataset.database', mod)

    class Base:
        def _init_dataset(self):
            pass

        def set_ray_store(self, train, test, device=None):
            self.stored = (train, test, device)

    class Module(ReferenceDatasetMixin, Base):
        pass

    m = Module()
    m.cfg = {'database_name': 'custom/fake/8', 'dataset_dir': '.'}
    if get_mask is not None:
        m.cfg['get_mask'] = get_mask
    m.is_nerf = False
    m._init_dataset()
    train, test, _ = m.stored
    assert ('mask' in train) == bool(get_mask) and ('mask' in test) == bool(get_mask)
    if get_mask:
        assert tuple(train['mask'].shape) == (3, 3, 4, 1) and tuple(test['mask'].shape) == (2, 3, 4, 1)


def _thick(get_mask):
    from nu_nerf_amd.stage2_thick import Stage2Renderer
    from nu_nerf_amd.lbvh import icosphere
    shader = {'sphere_direction': True, 'human_light': False, 'light_exp_max': 5.0}
    cfg = {'name': 's2t', 'network': 'stage2', 'get_mask': get_mask, 'database_name': 'real/x/raw_1024', 'is_nerf': False,
           'shader_config': shader, 'stage1_cfg': {'name': 's1', 'network': 'shape', 'get_mask': False, 'is_nerf': False,
                                                   'shader_config': shader},
           'stage1_mesh_arrays': icosphere(1, 0.5)}
    return Stage2Renderer(cfg, training=False)


def _coded_store(n=3, h=5, w=7, mask_shape='nhw1'):
    """Images whose red channel codes (image, pixel); the mask is a known function of that code."""
    code = torch.arange(n * h * w, dtype=torch.float32).reshape(n, h, w)
    imgs = torch.stack([code / 1000.0, torch.zeros_like(code), torch.zeros_like(code)], 1)        # [n,3,h,w]
    mask = ((code.long() * 7) % 3 == 0).float()
    Ks = torch.tensor([[10.0, 0, 3.5], [0, 10.0, 2.5], [0, 0, 1.0]]).expand(n, 3, 3).clone()
    poses = torch.cat([torch.eye(3).expand(n, 3, 3), torch.tensor([0.0, 0.0, 3.0]).reshape(1, 3, 1).expand(n, 3, 1)], 2).clone()
    info = {'imgs': imgs, 'Ks': Ks, 'poses': poses, 'mask': mask[..., None] if mask_shape == 'nhw1' else mask}
    return info, code, mask


@pytest.mark.parametrize("mask_shape", ['nhw1', 'nhw'])
def test_real_capture_store_carries_the_mask_through_a_shuffle(mask_shape):
    net = _thick(True)
    info, code, mask = _coded_store(mask_shape=mask_shape)
    torch.manual_seed(0)
    net.set_ray_store(info, device='cpu')
    b = net.train_batch
    assert set(b) == {'dirs', 'rgbs', 'idxs', 'mask'} and b['mask'].shape == (net.tbn, 1)
    got_code = torch.round(b['rgbs'][:, 0] * 1000.0).long()
    assert not torch.equal(got_code, torch.arange(net.tbn))                               # shuffled
    assert torch.equal(b['mask'][:, 0], mask.reshape(-1)[got_code])                       # aligned with rgbs
    assert torch.equal(b['idxs'][:, 0], got_code // (5 * 7))                              # and with idxs
    net._shuffle_train_batch()
    got_code = torch.round(net.train_batch['rgbs'][:, 0] * 1000.0).long()
    assert torch.equal(net.train_batch['mask'][:, 0], mask.reshape(-1)[got_code])


def test_store_without_get_mask_or_without_a_mask_is_unchanged():
    info, _, _ = _coded_store()
    plain = {k: v for k, v in info.items() if k != 'mask'}
    stores = []
    for get_mask, inf in ((False, info), (True, plain), (False, plain)):
        net = _thick(get_mask)
        torch.manual_seed(0)
        net.set_ray_store(inf, device='cpu')
        stores.append(net.train_batch)
    for s in stores:
        assert set(s) == {'dirs', 'rgbs', 'idxs'}
        for k in s:
            assert torch.equal(s[k], stores[0][k])


def test_test_image_mask_is_resized_nearest_with_the_images():
    net = _thick(True)
    n, H, W = 2, 8, 6
    m = (torch.arange(n * H * W).reshape(n, H, W, 1) % 5 == 0).float()
    r = net._ray_mask(m, 4, 3)
    ref = torch.nn.functional.interpolate(m.reshape(n, 1, H, W), size=(4, 3), mode='nearest')
    assert torch.equal(r, ref.reshape(-1, 1))
    assert torch.equal(net._ray_mask(m, H, W), m.reshape(-1, 1))
