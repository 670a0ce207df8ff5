"""SDF normal maps, host side: the ABI of the new entries and the resources of sdf_grad_fwd_kernel, the flat tangent frames of
the export, the tangent-space encoding read back through the written glTF, the refusals, and a float64 model of what the normal map
gains over vertex normals.

Bounds.  Orthonormality 1e-12: float64 products of unit vectors.  Round trip 0.4 degrees: each of the three encoded components is off
by at most 1 / 255 (half a step of 1 / 255 on 0.5 c + 0.5), the vector by at most sqrt(3) / 255, the angle by asin of that = 0.389
degrees; the float32 frame of the file adds 1e-7."""
import json
import os
import sys

import numpy as np
import pytest

import texture_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 150800                                    # 66 576 + 10 240 + 73 728 + 256


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def sphere_mesh(degenerate=True):
    """The 80-face icosphere of radius 0.5, plus (81st face) a face of zero area."""
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(1, 0.5)
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int32)
    if degenerate:
        F = np.concatenate([F, [[F[0, 0], F[0, 1], F[0, 0]]]]).astype(np.int32)
    return V, F


def sphere_atlas(V, F, T, pad):
    """An atlas dict whose 'normal' is x / |x| at the float64 texel points (zero where unowned)."""
    from nu_nerf_amd.texture import atlas_layout, atlas_uv
    lay = atlas_layout(len(F), T, pad)
    face = TO.owner_map(lay)[0]
    points = TO.atlas_f64(lay, V.astype(np.float64)[F])
    own = face >= 0
    normal = np.zeros((T, T, 3))
    normal[own] = unit(points[own])
    z = np.zeros((T, T), np.float32)
    return {'albedo': np.zeros((T, T, 3), np.float32), 'metallic': z, 'roughness': z, 'face': face, 'uv': atlas_uv(lay, F), 'layout': lay,
            'normal': normal.astype(np.float32)}


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_and_kernel_resources():
    from nu_nerf_amd import _lib
    sig = {n: a for n, _, a in _lib._signatures()}
    assert len(sig['nu_sdf_grad_fwd']) == 8
    assert len(sig['nu_atlas_sample_normal']) == 9 and len(sig['nu_atlas_gbuffer_normal']) == 12
    assert not any(s.startswith('Sg') for s in _lib.STRUCTS)            # the kernel-argument blocks are not part of the ABI
    lib = _lib.load()
    assert len(lib.nu_sdf_grad_fwd.argtypes) == 8
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    from kernel_regs import kernel_table
    table = dict(kernel_table(os.path.join(ROOT, 'nu_nerf_amd', 'build', 'sdf_grad.o')))
    (name, r), = [(k, v) for k, v in table.items() if k.startswith('sdf_grad_fwd_kernel')]
    print(name, r)
    assert r['vgpr_spill'] == 0 and r['scratch'] == 0 and r['lds'] == LDS_BYTES


# ---- the tangent frame -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', (0, 1))
def test_tangent_frames(pad):
    """Orthonormal, right-handed, and laid along the atlas: Tn points where u grows across the face, B where v grows.  (For a lower
    face that is B . e2 > 0; the upper face's frame is point-mirrored, its corner 2 lies at SMALLER v, so there B . e2 < 0 -- both are
    B . e2 having the sign of the v step from corner 0 to corner 2, which is what is asserted.)"""
    from nu_nerf_amd.texture import atlas_layout, atlas_uv, tangent_frames
    V, F = sphere_mesh()
    Tn, B, N, flat = tangent_frames(V, F)
    assert flat.tolist() == [False] * 80 + [True]
    assert np.array_equal(N[80], [0, 0, 1]) and np.array_equal(Tn[80], [1, 0, 0]) and np.array_equal(B[80], [0, 1, 0])
    for a, b in ((Tn, Tn), (B, B), (N, N)):
        assert np.abs((a * b).sum(1) - 1).max() <= 1e-12
    for a, b in ((Tn, B), (Tn, N), (B, N)):
        assert np.abs((a * b).sum(1)).max() <= 1e-12
    assert np.abs(np.cross(N, Tn) - B).max() == 0 and (np.einsum('ij,ij->i', np.cross(Tn, B), N) > 0.999999).all()      # w = +1
    uv = atlas_uv(atlas_layout(len(F), 128, pad), F).astype(np.float64)
    Vd = V.astype(np.float64)
    e1, e2 = Vd[F[:, 1]] - Vd[F[:, 0]], Vd[F[:, 2]] - Vd[F[:, 0]]
    du, dv = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
    ok = ~flat
    assert (np.sign(du[ok]) == np.where(np.arange(81) & 1, -1, 1)[ok]).all() and (np.sign(dv[ok]) == np.sign(du[ok])).all()
    assert ((Tn * e1).sum(1) * du > 0)[ok].all()
    assert ((B * e2).sum(1) * dv > 0)[ok].all()
    assert ((B * e2).sum(1) > 0)[ok & (np.arange(81) % 2 == 0)].all()
    assert np.abs((N * unit(np.cross(e1, e2) + flat[:, None]))[ok].sum(1) - 1).max() <= 1e-12


# ---- encode -> files -> decode -------------------------------------------------------------------------------------------------------------
def read_gltf(path):
    doc = json.load(open(path))
    blob = open(os.path.join(os.path.dirname(path), doc['buffers'][0]['uri']), 'rb').read()
    out = {}
    for key, i in doc['meshes'][0]['primitives'][0]['attributes'].items():
        a = doc['accessors'][i]
        bv = doc['bufferViews'][a['bufferView']]
        width = {'VEC4': 4, 'VEC3': 3, 'VEC2': 2}[a['type']]
        assert a['componentType'] == 5126 and bv['byteLength'] == a['count'] * width * 4 and bv['byteOffset'] + bv['byteLength'] <= len(blob)
        out[key] = np.frombuffer(blob, '<f4', a['count'] * width, bv['byteOffset']).reshape(-1, width)
    return doc, blob, out


@pytest.mark.parametrize('pad', (0, 1))
def test_encode_round_trip(tmp_path, pad):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.lbvh import vertex_normals_and_curvature
    from nu_nerf_amd.mask_render import _pillow
    import torch
    V, F = sphere_mesh()
    T = 128
    atlas = sphere_atlas(V, F, T, pad)
    vn = vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F[:80]).long())[0].numpy()
    image, backfacing = X.tangent_normal_image(atlas, V, F, count=True)
    assert backfacing == 0                                              # asserted for this input, not assumed
    assert image.dtype == np.uint8 and image.shape == (T, T, 3) and np.array_equal(image, X.tangent_normal_image(atlas, V, F))
    d = tmp_path / 'asset'
    X.write_textures(str(d), atlas)
    path, _ = X.write_gltf(str(d / 'mesh.gltf'), V, F, atlas['uv'], vn, str(d), normal_map=atlas)
    doc, _, attr = read_gltf(path)
    uri = doc['images'][doc['textures'][doc['materials'][0]['normalTexture']['index']]['source']]['uri']
    png = np.asarray(_pillow().open(os.path.join(os.path.dirname(path), uri)))
    assert png.tobytes() == image.tobytes()
    # the viewer's reconstruction, from the file alone: frame of the texel's face = its first corner's NORMAL / TANGENT
    Nf, Tf = attr['NORMAL'].astype(np.float64)[::3], attr['TANGENT'].astype(np.float64)[::3]
    for k in (1, 2):                                                     # constant per face
        assert np.array_equal(attr['NORMAL'][k::3], attr['NORMAL'][::3]) and np.array_equal(attr['TANGENT'][k::3], attr['TANGENT'][::3])
    assert (Tf[:, 3] == 1).all()
    Bf = np.cross(Nf, Tf[:, :3]) * Tf[:, 3:]
    face = atlas['face']
    own = (face >= 0) & (face != 80)
    assert own.sum() > 0.3 * T * T
    c = png.astype(np.float64) / 255.0 * 2.0 - 1.0
    f = face[own]
    got = c[own][:, 0:1] * Tf[f, :3] + c[own][:, 1:2] * Bf[f] + c[own][:, 2:3] * Nf[f]
    want = atlas['normal'][own].astype(np.float64)
    assert np.abs(got - want).max() <= np.sqrt(3) / 255 + 1e-6
    cosang = np.clip((unit(got) * want).sum(1), -1, 1)
    worst = float(np.degrees(np.arccos(cosang)).max())
    print(f"normal.png round trip (pad {pad}): worst angle {worst:.4f} deg over {int(own.sum())} texels")
    assert worst <= 0.4
    assert (png[~own] == (128, 128, 255)).all()                          # unowned texels and the zero-area face
    # atlas.npz carries the normal; a directory without one reads back without one
    back = X.load_textures(str(d), len(F))
    assert back['normal'].dtype == np.float32 and np.array_equal(back['normal'], atlas['normal'])
    plain = {k: v for k, v in atlas.items() if k != 'normal'}
    X.write_textures(str(tmp_path / 'plain'), plain)
    assert 'normal' not in X.load_textures(str(tmp_path / 'plain')) and 'normal' not in np.load(str(tmp_path / 'plain' / 'atlas.npz')).files
    assert sorted(os.listdir(tmp_path / 'plain')) == ['albedo.png', 'atlas.npz', 'orm.png']
    with pytest.raises(ValueError):
        X.tangent_normal_image(plain, V, F)
    # a normal that faces away from its face is counted
    flipped = dict(atlas, normal=-atlas['normal'])
    assert X.tangent_normal_image(flipped, V, F, count=True)[1] == int(own.sum())


def test_gltf_structure(tmp_path):
    from nu_nerf_amd import texture as X
    V, F = sphere_mesh(degenerate=False)
    atlas = sphere_atlas(V, F, 64, 1)
    vn = unit(V).astype(np.float32)
    d = tmp_path
    os.makedirs(d / 'a')
    path, _ = X.write_gltf(str(d / 'a' / 'm.gltf'), V, F, atlas['uv'], vn, normal_map=atlas)
    doc, blob, attr = read_gltf(path)
    prim = doc['meshes'][0]['primitives'][0]
    assert set(prim['attributes']) == {'POSITION', 'NORMAL', 'TEXCOORD_0', 'TANGENT'}
    tan = doc['accessors'][prim['attributes']['TANGENT']]
    assert tan['type'] == 'VEC4' and tan['count'] == 3 * len(F) and tan['componentType'] == 5126
    pos = doc['accessors'][prim['attributes']['POSITION']]
    assert np.array_equal(np.asarray(pos['min'], np.float32), attr['POSITION'].min(0)) and np.array_equal(np.asarray(pos['max'], np.float32), attr['POSITION'].max(0))
    mat = doc['materials'][0]
    assert mat['normalTexture'] == {'index': 2, 'scale': 1.0} and doc['images'][doc['textures'][2]['source']]['uri'] == 'normal.png'
    assert os.path.exists(d / 'a' / 'normal.png') and len(blob) == 3 * len(F) * (12 + 12 + 8 + 16)
    # NORMAL is the flat face normal, not the vertex normal
    Vd = V.astype(np.float64)
    flatn = unit(np.cross(Vd[F[:, 1]] - Vd[F[:, 0]], Vd[F[:, 2]] - Vd[F[:, 0]]))
    assert np.abs(attr['NORMAL'][::3] - flatn).max() < 1e-6
    # normal_map=None: the bytes of a call without the argument
    os.makedirs(d / 'b')
    os.makedirs(d / 'c')
    p1, b1 = X.write_gltf(str(d / 'b' / 'm.gltf'), V, F, atlas['uv'], vn)
    p2, b2 = X.write_gltf(str(d / 'c' / 'm.gltf'), V, F, atlas['uv'], vn, None, None)
    assert open(p1, 'rb').read() == open(p2, 'rb').read() and open(b1, 'rb').read() == open(b2, 'rb').read()
    assert os.listdir(d / 'c') == os.listdir(d / 'b') and 'normalTexture' not in open(p1).read() and 'TANGENT' not in open(p1).read()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_pack_and_refusals():
    import torch
    from nu_nerf_amd import relight as R, texture as X
    V, F = sphere_mesh(degenerate=False)
    atlas = sphere_atlas(V, F, 64, 0)
    packed = X.pack_atlas(atlas, device='cpu')
    assert packed.has_normal and tuple(packed.tex.shape) == (2, 64, 64, 4)
    assert np.array_equal(packed.tex[1, ..., 1:4].numpy(), atlas['normal']) and np.array_equal(packed.tex[1, ..., 0].numpy(), atlas['roughness'])
    plain = X.pack_atlas({k: v for k, v in atlas.items() if k != 'normal'}, device='cpu')
    assert not plain.has_normal and not plain.tex[1, ..., 1:4].any()
    assert not X.pack_atlas(np.zeros((64, 64, 5), np.float32), atlas['layout'], device='cpu').has_normal
    with pytest.raises(ValueError):
        X.pack_atlas(dict(atlas, normal=atlas['normal'][:-1]), device='cpu')
    scene = R.Scene.__new__(R.Scene)                                    # what the refusals read of a Scene; nothing reaches a device
    scene.device, scene.V, scene.F, scene.texture = torch.device('cpu'), torch.from_numpy(V), torch.from_numpy(F), plain
    gbuf, face, pix = torch.zeros(4, 20), torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match='normal'):
        X.texture_gbuffer(scene, face, gbuf, pix, plain, normals=True)
    poses = np.eye(4)[None, :3]
    env = np.ones((4, 8, 3), np.float32)
    with pytest.raises(ValueError, match='normal_map'):                 # the Scene's own atlas has no normals
        R.relight_linear(scene, None, None, env, poses, 8, 8, 4, normal_map=True)
    with pytest.raises(ValueError, match='normal_map'):
        R.relight(scene, None, None, env, poses, 8, 8, 4, normal_map=True)
    with pytest.raises(ValueError, match='normal_map'):
        R.relight_splitsum_linear(scene, None, None, env[None], [0.0], env, poses, 8, 8, normal_map=True)
    with pytest.raises(ValueError, match='normal_map'):
        R.relight_splitsum(scene, None, None, env[None], [0.0], env, poses, 8, 8, normal_map=True)
    scene.texture = None                                                # no texture at all
    with pytest.raises(ValueError, match='normal_map'):
        R.relight_linear(scene, None, None, env, poses, 8, 8, 4, normal_map=True)
    with pytest.raises(ValueError):
        X.bake_textures(None, V, F, normals='mesh')


def test_command_arguments(tmp_path):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.bake_textures import parse_args as bake_args
    from nu_nerf_amd.relight import parse_args
    assert bake_args(['--cfg', 'c.yaml']).normals is None
    f = bake_args(['--cfg', 'c.yaml', '--normals', 'sdf', '--decimate', '1000'])
    assert f.normals == 'sdf' and f.decimate == 1000
    with pytest.raises(SystemExit):
        bake_args(['--cfg', 'c.yaml', '--normals', 'mesh'])
    V, F = sphere_mesh(degenerate=False)
    atlas = sphere_atlas(V, F, 64, 0)
    X.write_textures(str(tmp_path / 'with'), atlas)
    X.write_textures(str(tmp_path / 'without'), {k: v for k, v in atlas.items() if k != 'normal'})
    base = ['--mesh', 'm.ply', '--hdr', 'sky.hdr', '--name', 'n']
    assert parse_args(base + ['--texture', str(tmp_path / 'with'), '--normal-map']).normal_map is True
    assert parse_args(base + ['--texture', str(tmp_path / 'with')]).normal_map is False
    for bad in (base + ['--material', 'mat', '--normal-map'],                                   # without --texture
                base + ['--texture', str(tmp_path / 'without'), '--normal-map'],               # a directory without normals
                base + ['--texture', str(tmp_path / 'with'), '--normal-map', '--inner', 'i.ply', '--inner-material', 'im']):
        with pytest.raises(SystemExit):
            parse_args(bad)


# ---- what the map gains: a float64 model ---------------------------------------------------------------------------------------------------
def test_float64_model_of_the_gain():
    """f = |x| - 0.5 on the 80-face icosphere of radius 0.5, T = 256: the maximum angle to x / |x| at 20 000 random points of the mesh
    of (a) the renormalised barycentric mix of the angle-weighted vertex normals, (b) the renormalised bilinear lookup of texel normals.
    Printed; DESIGN.md 32 records the figures.  The model's answer is not the one hoped for: on a sphere about the origin the mix
    sum_k w_k v_k / |v_k| of the vertex normals IS x / 0.5, so (a) is exact up to rounding (1.5e-6 degrees), while (b) carries the
    bilinear interpolation error of a unit field (2.4e-3 degrees at L = 33 texels a leg).  A sphere cannot show the gain; what is
    asserted is what the model does establish: (a) is exact, and (b) stays below L^-2 radians -- linear interpolation of a unit field
    over an angular step h errs by at most h^2 / 8 per axis, two axes, and h < 1 / L because a face's edges subtend less than one
    radian (0.55 .. 0.65).  The device test measures a network."""
    from nu_nerf_amd.texture import atlas_layout
    V, F = sphere_mesh(degenerate=False)
    Vd, F = V.astype(np.float64), F.astype(np.int64)
    lay = atlas_layout(len(F), 256, 0)
    tri = Vd[F]
    # angle-weighted vertex normals
    fn = unit(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    vn = np.zeros_like(Vd)
    for k in range(3):
        a, b = unit(tri[:, (k + 1) % 3] - tri[:, k]), unit(tri[:, (k + 2) % 3] - tri[:, k])
        np.add.at(vn, F[:, k], np.arccos(np.clip((a * b).sum(1), -1, 1))[:, None] * fn)
    vn = unit(vn)
    face, u, v = TO.triangle_points(len(F), 20000, 11, n_edge=0)
    face, u, v = face[:20000], u[:20000], v[:20000]
    w = np.stack([1 - u - v, u, v], -1)
    x = np.einsum('nk,nkc->nc', w, tri[face])
    want = unit(x)
    angle = lambda n: float(np.degrees(np.arccos(np.clip((unit(n) * want).sum(1), -1, 1))).max())      # noqa: E731
    a = angle(np.einsum('nk,nkc->nc', w, vn[F[face]]))
    own = TO.owner_map(lay)[0] >= 0
    texel = np.zeros((256, 256, 3))
    texel[own] = unit(TO.atlas_f64(lay, tri)[own])
    b = angle(TO.lookup_f64(lay, texel, face, u, v)[0])
    print(f"float64 model, 80 faces, T = 256 (L = {lay['L']}): vertex normals {a:.4f} deg, normal map {b:.5f} deg, ratio {a / b:.1f} x")
    assert a < 1e-4 and np.radians(b) < 1.0 / lay['L'] ** 2
