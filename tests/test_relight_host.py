"""Relighting, host side (no GPU): the camera orbit against the reference's recorded poses, the frame change, the intrinsics, the
Radiance reader, the command line, the PNG writer -- and the numpy oracle's own check of the convex-body argument the GPU test uses."""
import os

import numpy as np
import pytest

import relight_oracle as O
from nu_nerf_amd import relight as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'relight_poses.npz')


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def test_poses_match_the_reference_recording():
    g = np.load(GOLDEN)
    assert len(g['cases']) >= 4
    for i, (num, az, el, dist) in enumerate(g['cases']):
        got = R.relighting_poses(int(num), az, el, dist)
        assert got.shape == (int(num), 3, 4) and got.dtype == np.float64
        assert np.abs(got - g[f'poses_{i}']).max() <= 1e-12


def test_frame_change_gives_the_z_up_look_at_orbit():
    g = np.load(GOLDEN)
    for i, (num, az, el, dist) in enumerate(g['cases']):
        m = R.camera_in_mesh_frame(g[f'poses_{i}'])
        Rm, t = m[:, :, :3], m[:, :, 3]
        assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.allclose(np.linalg.det(Rm), 1.0)
        centre = -np.einsum('nji,nj->ni', Rm, t)
        assert np.abs(np.linalg.norm(centre, axis=1) - dist).max() < 1e-12
        assert np.abs(np.degrees(np.arcsin(centre[:, 2] / dist)) - el).max() < 1e-9
        want_az = np.deg2rad(az) + np.linspace(-np.pi / 2, np.pi / 2, int(num))
        got_az = np.arctan2(centre[:, 1], centre[:, 0])
        assert np.abs(np.angle(np.exp(1j * (got_az - want_az)))).max() < 1e-9
        # optical axis (row 2) through the origin; image x horizontal; image y pointing down (negative z component)
        assert np.abs(Rm[:, 2] + centre / dist).max() < 1e-12
        assert np.abs(Rm[:, 0, 2]).max() < 1e-12 and (Rm[:, 1, 2] < 0).all()
        # R_trans and R_blender cancel: the frame change undoes the last factor of the reference's composition
        assert np.abs(Rm @ R.R_BLENDER - g[f'poses_{i}'][:, :, :3]).max() < 1e-12


def test_intrinsics_are_blenders_default_camera():
    K = R.intrinsics(600, 800)
    assert np.array_equal(K, np.array([[50 / 36 * 800, 0, 400.0], [0, 50 / 36 * 800, 300.0], [0, 0, 1.0]]))
    K = R.intrinsics(800, 640, focal_mm=35.0, sensor_mm=32.0)
    assert K[0, 0] == K[1, 1] == 35.0 / 32.0 * 800 and (K[0, 2], K[1, 2]) == (320.0, 400.0)


def test_trans_turns_the_mesh_about_x():
    assert np.array_equal(np.array([1.0, 2.0, 3.0]) @ R.TRANS.T, np.array([1.0, -3.0, 2.0]))      # (x, y, z) -> (x, -z, y): +90 degrees


# ---- Radiance files --------------------------------------------------------------------------------------------------------------------
def _rgbe_encode(rgb):
    """float [H,W,3] -> uint8 [H,W,4] (Ward's float2rgbe)."""
    m = rgb.max(-1)
    mant, ex = np.frexp(m)
    scale = np.where(m > 1e-32, mant * 256.0 / np.where(m > 0, m, 1.0), 0.0)
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = (rgb * scale[..., None]).astype(np.uint8)
    out[..., 3] = np.where(m > 1e-32, ex + 128, 0).astype(np.uint8)
    return out


def _rgbe_decode(rgbe):
    e = rgbe[..., 3].astype(np.int64)
    v = rgbe[..., :3].astype(np.float64) * (2.0 ** (e - 136))[..., None]
    v[e == 0] = 0.0
    return v.astype(np.float32)


def _rle_channel(row):
    out, x, n = bytearray(), 0, len(row)
    while x < n:
        run = 1
        while x + run < n and run < 127 and row[x + run] == row[x]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, int(row[x])])
            x += run
        else:
            lit = x
            while x < n and x - lit < 128:
                if x + 2 < n and row[x] == row[x + 1] == row[x + 2]:
                    break
                x += 1
            out += bytes([x - lit]) + bytes(row[lit:x].tolist())
    return bytes(out)


def _write_hdr(path, rgbe, rle, header=b'#?RADIANCE\n# made by a test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n'):
    h, w = rgbe.shape[:2]
    with open(path, 'wb') as fh:
        fh.write(header + b'-Y %d +X %d\n' % (h, w))
        for y in range(h):
            if rle:
                fh.write(bytes([2, 2, w >> 8, w & 255]))
                for c in range(4):
                    fh.write(_rle_channel(rgbe[y, :, c]))
            else:
                fh.write(rgbe[y].tobytes())


def _hdr_image(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    img = g.random((h, w, 3)) * 10.0 ** g.uniform(-3, 3, (h, w, 1))
    img[:, w // 3: w // 3 + 20] = 0.75                     # constant stretches: runs for the encoder
    img[0, :4] = 0.0                                       # e = 0
    return img


@pytest.mark.parametrize("rle", [False, True])
def test_read_hdr_round_trip_is_exact(tmp_path, rle):
    rgbe = _rgbe_encode(_hdr_image(9, 61, 3))
    path = tmp_path / ('rle.hdr' if rle else 'flat.hdr')
    _write_hdr(path, rgbe, rle)
    if rle:
        assert os.path.getsize(path) < 9 * 61 * 4 + 80        # the runs were coded
    got = R.read_hdr(path)
    assert got.dtype == np.float32 and got.shape == (9, 61, 3)
    assert np.array_equal(got, _rgbe_decode(rgbe))
    assert (got[0, :4] == 0).all() and got.max() > 100.0 and 0 < got[got > 0].min() < 1e-2


def test_read_hdr_extreme_exponents_and_narrow_images(tmp_path):
    rgbe = np.zeros((2, 5, 4), np.uint8)                    # narrower than 8: always flat
    rgbe[0, :, :3], rgbe[0, :, 3] = 255, (1, 2, 128, 254, 255)
    rgbe[1, :, :3], rgbe[1, :, 3] = 1, (1, 0, 136, 137, 255)
    _write_hdr(tmp_path / 'e.hdr', rgbe, False)
    got = R.read_hdr(tmp_path / 'e.hdr')
    assert np.array_equal(got, _rgbe_decode(rgbe)) and got[1, 2, 0] == 1.0 and got[1, 1, 0] == 0.0 and np.isfinite(got).all()


def test_read_hdr_npy_and_malformed_files(tmp_path):
    a = np.random.Generator(np.random.PCG64(1)).random((4, 8, 3))
    np.save(tmp_path / 'e.npy', a)
    assert np.array_equal(R.read_hdr(tmp_path / 'e.npy'), a.astype(np.float32))
    np.save(tmp_path / 'bad.npy', a[..., :2])
    with pytest.raises(ValueError):
        R.read_hdr(tmp_path / 'bad.npy')
    rgbe = _rgbe_encode(_hdr_image(3, 9, 5))
    for name, header in (('sig', b'RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n'), ('fmt', b'#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n'),
                         ('nofmt', b'#?RADIANCE\n\n')):
        _write_hdr(tmp_path / (name + '.hdr'), rgbe, False, header)
        with pytest.raises(ValueError):
            R.read_hdr(tmp_path / (name + '.hdr'))
    with open(tmp_path / 'res.hdr', 'wb') as fh:
        fh.write(b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+X 9 -Y 3\n' + rgbe.tobytes())
    with pytest.raises(ValueError):
        R.read_hdr(tmp_path / 'res.hdr')
    _write_hdr(tmp_path / 'ok.hdr', rgbe, True)
    data = open(tmp_path / 'ok.hdr', 'rb').read()
    with open(tmp_path / 'short.hdr', 'wb') as fh:
        fh.write(data[:-7])
    with pytest.raises(ValueError):
        R.read_hdr(tmp_path / 'short.hdr')


def test_pack_env_is_rgba():
    e = R.pack_env(np.arange(24, dtype=np.float64).reshape(2, 4, 3))
    assert e.dtype == np.float32 and e.shape == (2, 4, 4) and (e[..., 3] == 1).all() and e[1, 2, 1] == 19.0
    with pytest.raises(ValueError):
        R.pack_env(np.zeros((2, 4)))


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_command_line_defaults_are_the_references():
    f = R.parse_args(['--mesh', 'm.ply', '--material', 'mat', '--hdr', 'e.hdr', '--name', 'bell'])
    assert (f.width, f.height, f.samples, f.cam_dist, f.num, f.azimuth, f.elevation, f.trans) == (800, 800, 1024, 3.0, 360, 0.0, 45.0, False)
    assert (f.focal_mm, f.sensor_mm) == (50.0, 36.0)
    assert R.output_dir(f) == os.path.join('data', 'relight', 'bell')
    assert R.frame_path(R.output_dir(f), 7) == os.path.join('data', 'relight', 'bell', '7.png')
    f = R.parse_args(['--mesh', 'm.ply', '--material', 'mat', '--hdr', 'e.hdr', '--name', 'bell', '--trans', '--num', '4', '--output', 'o'])
    assert f.trans and f.num == 4 and R.output_dir(f) == 'o'
    for bad in (['--samples', '7'], ['--samples', '0'], ['--blender', 'b'], ['--num', '0']):
        with pytest.raises(SystemExit):
            R.parse_args(['--mesh', 'm.ply', '--material', 'mat', '--hdr', 'e.hdr', '--name', 'bell'] + bad)
    with pytest.raises(SystemExit):
        R.parse_args(['--mesh', 'm.ply'])


def test_existing_frames_are_skipped(tmp_path):
    assert R.frames_to_render(str(tmp_path), 4) == [0, 1, 2, 3]
    for k in (0, 2):
        open(R.frame_path(str(tmp_path), k), 'wb').close()
    assert R.frames_to_render(str(tmp_path), 4) == [1, 3]


def test_png_round_trip_keeps_alpha(tmp_path):
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(2))
    img = g.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    img[..., 3] = 255
    img[1:3, 2:5] = 0                                     # miss pixels
    R.write_png(str(tmp_path / 'a.png'), img)
    with Image.open(tmp_path / 'a.png') as im:
        assert im.mode == 'RGBA'
        back = np.asarray(im)
    assert np.array_equal(back, img) and (back[1:3, 2:5, 3] == 0).all()
    with pytest.raises(ValueError):
        R.write_png(str(tmp_path / 'b.png'), img[..., :3])


def test_srgb8_of_the_oracle_matches_the_projects_transfer():
    import torch
    x = np.concatenate([np.linspace(0, 0.01, 50), np.linspace(0.01, 1.5, 200)])
    lin = torch.from_numpy(np.stack([x, x, x, np.ones_like(x)], -1)).float()
    got = R.to_srgb8(lin).numpy().astype(np.int64)
    want = O.to_srgb8(lin[:, :3].double().numpy())
    assert np.abs(got[:, :3] - want).max() <= 1 and (got[:, 3] == 255).all() and got[-1, 0] == 255


# ---- the oracle's own checks -----------------------------------------------------------------------------------------------------------
def test_sample_sequence_is_a_shifted_hammersley_set():
    S = 64
    lobe, b1, b2 = O.sample_bits(3, 1234, 7, S, np.arange(S))
    assert (lobe[:32] == 0).all() and (lobe[32:] == 1).all() and b1.max() < 2 ** 24 and b2.max() < 2 ** 24 and b1.min() >= 0
    for lo in (0, 32):                                   # per lobe: one point per stratum of 1/32 in both coordinates
        assert sorted(((b1[lo:lo + 32] - b1[lo]) % 2 ** 24) >> 19) == list(range(32))
        assert sorted(((b2[lo:lo + 32] - b2[lo]) % 2 ** 24) >> 19) == list(range(32))
    other = O.sample_bits(3, 1235, 7, S, np.arange(S))
    assert (other[1] != b1).any() and (O.sample_bits(3, 1234, 8, S, np.arange(S))[1] != b1).any()


def test_convex_body_has_no_occluded_sample_above_the_geometric_horizon():
    """For a convex polyhedron the offset origin lies outside the hit face's half-space and a direction with n_g . l > 0 moves away
    from it, so no sample above the geometric horizon is occluded: float64 brute force over every triangle."""
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(2, 0.5)
    V, F = V.astype(np.float64), F.astype(np.int64)
    VN = O.vertex_normals(V, F)
    mat = np.tile(np.array([0.8, 0.7, 0.6, 0.5, 0.4]), (len(V), 1))
    h = w = 12
    pose = R.camera_in_mesh_frame(R.relighting_poses(3, 20.0, 35.0, 2.0))[1]
    o, d = O.pinhole_rays(R.intrinsics(h, w), pose, h, w)
    hit, face, _ = O.brute_trace(V, F, o, d)
    assert 20 < hit.sum() < h * w
    pixel = np.nonzero(hit)[0]
    rows = O.gbuffer_rows(V, F, VN, mat, o[hit], d[hit], face[hit], 0, pixel)
    S, traced = 32, 0
    for s in range(S):
        lobe, b1, b2 = O.sample_bits(0, pixel, 5, S, np.full(len(pixel), s))
        ro, rd, nsl, ngl, ok = O.shadow_rays(rows, lobe, b1, b2, R.ORIGIN_EPS)
        go = ok & (nsl > 0) & (ngl > 0)
        occluded, _, _ = O.brute_trace(V, F, ro[go], rd[go])
        assert not occluded.any()
        traced += int(go.sum())
    assert traced > 0.5 * S * len(pixel)
