"""The texture atlas without a GPU: the layout arithmetic, the three properties of the construction on the float64 oracle
(disjoint UV triangles; a bilinear lookup anywhere in a face's triangle touches only texels that face owns; affine attributes come back
to rounding), the file writers read back, the commands' argument handling, and the public surface."""
import json
import os

import numpy as np
import pytest

import texture_oracle as TO

FACES = (1, 7, 20, 320)
SIZES = (64, 128, 256)
PADS = (0, 1, 2)
AFFINE_TOL = 1e-12
SENTINEL = 1e30


def _cols(nf):
    cells = (nf + 1) // 2
    return next(k for k in range(1, cells + 1) if k * k >= cells)


# ---- 1. layout arithmetic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", FACES)
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("pad", PADS)
def test_layout_arithmetic(nf, T, pad):
    from nu_nerf_amd.texture import atlas_layout
    cols = _cols(nf)
    assert cols == {1: 1, 7: 2, 20: 4, 320: 13}[nf]
    c = T // cols
    if c - 3 - 3 * pad < 2:
        with pytest.raises(ValueError, match=r"smallest size that works is (\d+)") as e:
            atlas_layout(nf, T, pad)
        works = int(str(e.value).rsplit(' ', 1)[1])
        assert works > T and atlas_layout(nf, works, pad)['L'] == 2
        with pytest.raises(ValueError):
            atlas_layout(nf, works - 1, pad)
        return
    lay = atlas_layout(nf, T, pad)
    assert lay == {'size': T, 'n_faces': nf, 'pad': pad, 'cols': cols, 'cell': c, 'L': c - 3 - 3 * pad}
    face, s, t = TO.owner_map(lay)
    # every face owns the same number of texels: the half cell below the diagonal
    counts = np.bincount(face[face >= 0], minlength=nf)
    assert (counts == c * (c - 1) // 2).all()
    if nf % 2:                                                                 # odd: the last cell has only its lower half
        k = nf >> 1
        cell = face[(k // cols) * c:(k // cols + 1) * c, (k % cols) * c:(k % cols + 1) * c]
        assert set(np.unique(cell)) == {-1, nf - 1}
    assert (face[cols * c:] == -1).all() and (face[:, cols * c:] == -1).all()  # outside the cells
    assert face.max() == nf - 1


def test_layout_rejects_bad_numbers():
    from nu_nerf_amd.texture import atlas_layout, atlas_uv
    for args in ((0, 64), (-3, 64), (4, 0), (4, 64, -1), (4, 64, 65), (4, 40000)):
        with pytest.raises(ValueError):
            atlas_layout(*args)
    with pytest.raises(ValueError):
        atlas_uv(atlas_layout(4, 64), np.zeros((5, 3), np.int32))
    with pytest.raises(ValueError):
        atlas_uv(dict(atlas_layout(4, 64), cell=31))


# ---- 2. the three properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,T,pad", [(nf, T, pad) for nf in FACES for T in SIZES for pad in PADS
                                      if T // _cols(nf) - 3 - 3 * pad >= 2])
def test_three_properties(nf, T, pad):
    from nu_nerf_amd.texture import atlas_layout, atlas_uv
    lay = atlas_layout(nf, T, pad)
    # 1. disjoint, inside the atlas
    uv = atlas_uv(lay)
    assert uv.dtype == np.float32 and uv.shape == (nf, 3, 2) and TO.uv_area_checks(lay, uv) == nf
    # 2. + 3. an attribute affine over each face (any three corner values), a sentinel everywhere a face does not own
    g = np.random.Generator(np.random.PCG64(1000 * nf + 10 * T + pad))
    corners = g.uniform(-1.0, 1.0, (nf, 3, 5))
    atlas = TO.atlas_f64(lay, corners, SENTINEL)
    owner = TO.owner_map(lay)[0]
    assert (atlas[owner < 0] == SENTINEL).all()
    face, u, v = TO.triangle_points(nf, 20000, seed=7 + nf)
    got, taps, weights = TO.lookup_f64(lay, atlas, face, u, v)
    used = weights != 0
    assert (taps >= 0).all() and (taps < T).all()
    assert (owner[taps[..., 1], taps[..., 0]][used] == np.broadcast_to(face[:, None], used.shape)[used]).all()     # property 2
    want = np.einsum('nk,nkc->nc', np.stack([1 - u - v, u, v], -1), corners[face])
    err = float(np.abs(got - want).max())
    assert err <= AFFINE_TOL, err                                                                                  # property 3; no 1e30 leaked
    # pad texels of margin on every side: the taps keep that distance from the cell's border and from the diagonal
    _, s, t = TO.owner_map(lay)
    st = np.stack([s[taps[..., 1], taps[..., 0]], t[taps[..., 1], taps[..., 0]]], -1)[used]
    assert st.min() >= pad and st.sum(-1).max() <= lay['cell'] - 2 - pad


def test_points_outside_the_triangle_are_clamped_into_it():
    from nu_nerf_amd.texture import atlas_layout
    lay = atlas_layout(7, 64, 1)
    corners = np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, (7, 3, 2))
    atlas = TO.atlas_f64(lay, corners, SENTINEL)
    face = np.arange(7)
    for (u, v), (cu, cv) in (((-0.5, -2.0), (0.0, 0.0)), ((3.0, 0.2), (1.0, 0.0)), ((0.25, 5.0), (0.25, 0.75)), ((-1.0, 0.5), (0.0, 0.5))):
        got = TO.lookup_f64(lay, atlas, face, np.full(7, u), np.full(7, v))[0]
        want = (1 - cu - cv) * corners[:, 0] + cu * corners[:, 1] + cv * corners[:, 2]
        assert np.abs(got - want).max() <= AFFINE_TOL


# ---- 3. writers --------------------------------------------------------------------------------------------------------------------------
def _asset(T=64, pad=1):
    from nu_nerf_amd.lbvh import icosphere, vertex_normals_and_curvature
    from nu_nerf_amd.texture import atlas_layout, atlas_uv
    import torch
    V, F = icosphere(1, 0.5)
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int32)
    lay = atlas_layout(len(F), T, pad)
    g = np.random.Generator(np.random.PCG64(5))
    owner = TO.owner_map(lay)[0]
    own = (owner >= 0)
    atlas = {'albedo': (g.uniform(-0.1, 1.1, (T, T, 3)) * own[..., None]).astype(np.float32),
             'metallic': (g.uniform(-0.1, 1.1, (T, T)) * own).astype(np.float32), 'roughness': (g.uniform(0, 1, (T, T)) * own).astype(np.float32),
             'face': owner, 'uv': atlas_uv(lay, F), 'layout': lay}
    normals = vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F).long())[0].numpy()
    return V, F, normals, atlas


def test_write_textures_round_trip(tmp_path):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.mask_render import _pillow
    V, F, normals, atlas = _asset()
    paths = X.write_textures(str(tmp_path / 'tex'), atlas)
    assert sorted(os.listdir(tmp_path / 'tex')) == ['albedo.png', 'atlas.npz', 'orm.png']
    back = X.load_textures(str(tmp_path / 'tex'), len(F))
    for k in ('albedo', 'metallic', 'roughness', 'face', 'uv'):
        assert back[k].dtype == atlas[k].dtype and np.array_equal(back[k], atlas[k]), k
    assert back['layout'] == atlas['layout']
    with pytest.raises(ValueError):
        X.load_textures(str(tmp_path / 'tex'), len(F) + 1)
    albedo = np.asarray(_pillow().open(paths['albedo.png']))
    orm = np.asarray(_pillow().open(paths['orm.png']))
    # the quantisation rules restated: sRGB (relight.to_srgb8's transfer) for the albedo, linear for roughness / metallic
    x = atlas['albedo'].astype(np.float64)
    srgb = np.where(x <= 0.0031308, 323 / 25 * x, (211 * np.maximum(x, np.finfo(np.float32).eps) ** (5 / 12) - 11) / 200)
    want = np.floor(np.clip(srgb, 0, 1) * 255 + 0.5)
    assert albedo.dtype == np.uint8 and albedo.shape == (64, 64, 3) and np.abs(albedo.astype(np.float64) - want).max() <= 1
    assert (albedo.astype(np.float64) == want).mean() > 0.99                   # float32 against float64 at a rounding boundary
    assert np.array_equal(albedo, X.srgb8(atlas['albedo']))
    lin = lambda a: np.floor(np.clip(a, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)     # noqa: E731
    assert (orm[..., 0] == 255).all() and np.array_equal(orm[..., 1], lin(atlas['roughness'])) and np.array_equal(orm[..., 2], lin(atlas['metallic']))
    assert X.linear8(np.asarray([-1.0, 0.0, 0.5, 1.0, 2.0])).tolist() == [0, 0, 128, 255, 255]
    assert X.srgb8(np.asarray([0.0, 0.0031308, 0.5, 1.0, 7.0])).tolist() == [0, 10, 188, 255, 255]


def test_srgb_rule_is_to_srgb8s():
    import torch
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.relight import to_srgb8
    x = np.random.Generator(np.random.PCG64(8)).uniform(-0.2, 1.2, (4096, 3)).astype(np.float32)
    want = to_srgb8(torch.cat([torch.from_numpy(x), torch.ones(4096, 1)], 1))[:, :3].numpy()
    got = X.srgb8(x)
    assert np.abs(got.astype(np.int64) - want).max() <= 1 and (got == want).mean() > 0.999      # numpy's and torch's pow differ by an ulp


def test_gltf_read_back(tmp_path):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.mask_render import _pillow
    V, F, normals, atlas = _asset()
    d = tmp_path / 'asset'
    X.write_textures(str(d / 'texture'), atlas)
    path, bin_path = X.write_gltf(str(d / 'mesh.gltf'), V, F, atlas['uv'], normals, str(d / 'texture'))
    doc = json.load(open(path))
    assert doc['asset']['version'] == '2.0' and doc['scenes'][doc['scene']]['nodes'] == [0] and doc['nodes'][0]['mesh'] == 0
    blob = open(os.path.join(os.path.dirname(path), doc['buffers'][0]['uri']), 'rb').read()
    assert bin_path.endswith('mesh.bin') and len(blob) == doc['buffers'][0]['byteLength'] == 3 * len(F) * (12 + 12 + 8)
    prim = doc['meshes'][0]['primitives'][0]
    assert prim['mode'] == 4 and 'indices' not in prim

    def accessor(i):
        a = doc['accessors'][i]
        bv = doc['bufferViews'][a['bufferView']]
        width = {'VEC3': 3, 'VEC2': 2}[a['type']]
        assert a['componentType'] == 5126 and a['count'] == 3 * len(F) and bv['byteLength'] == a['count'] * width * 4
        assert bv['byteOffset'] % 4 == 0 and bv['byteOffset'] + bv['byteLength'] <= len(blob)
        arr = np.frombuffer(blob, '<f4', a['count'] * width, bv['byteOffset']).reshape(-1, width)
        assert np.array_equal(np.asarray(a['min'], np.float32), arr.min(0)) and np.array_equal(np.asarray(a['max'], np.float32), arr.max(0))
        return arr
    pos, nrm, tex = (accessor(prim['attributes'][k]) for k in ('POSITION', 'NORMAL', 'TEXCOORD_0'))
    assert np.array_equal(pos, V[F.reshape(-1)]) and np.array_equal(nrm, normals[F.reshape(-1)])
    assert np.array_equal(tex, atlas['uv'].reshape(-1, 2)) and tex.min() >= 0 and tex.max() <= 1
    # the UVs address texel centres: corner k of face f is texel atlas_corners(layout)[f, k]
    xy = tex.astype(np.float64) * 64 - 0.5
    assert np.abs(xy - X.atlas_corners(atlas['layout']).reshape(-1, 2)).max() < 1e-4
    mat = doc['materials'][prim['material']]['pbrMetallicRoughness']
    assert mat['baseColorFactor'] == [1, 1, 1, 1] and mat['metallicFactor'] == 1 and mat['roughnessFactor'] == 1
    smp = doc['samplers'][0]
    assert smp == {'magFilter': 9729, 'minFilter': 9729, 'wrapS': 33071, 'wrapT': 33071}                  # LINEAR, LINEAR, CLAMP_TO_EDGE
    images = []
    for key in ('baseColorTexture', 'metallicRoughnessTexture'):
        t = doc['textures'][mat[key]['index']]
        assert t['sampler'] == 0
        uri = doc['images'][t['source']]['uri']
        assert not os.path.isabs(uri) and '\\' not in uri
        images.append(np.asarray(_pillow().open(os.path.join(os.path.dirname(path), uri))))
    albedo8, orm8 = X.texture_images(atlas)
    assert images[0].tobytes() == albedo8.tobytes() and images[1].tobytes() == orm8.tobytes()
    with pytest.raises(ValueError):
        X.write_gltf(str(d / 'bad.gltf'), V, F, atlas['uv'][:-1], normals)
    with pytest.raises(ValueError):
        X.write_gltf(str(d / 'bad.gltf'), V, F, atlas['uv'], normals[:-1])


def test_obj_read_back(tmp_path):
    from nu_nerf_amd import texture as X
    V, F, normals, atlas = _asset()
    path, mtl = X.write_obj(str(tmp_path / 'mesh.obj'), V, F, atlas['uv'], normals)
    rows = {'v': [], 'vt': [], 'vn': [], 'f': []}
    lines = open(path).read().split('\n')
    assert lines[0] == 'mtllib mesh.mtl' and 'usemtl baked' in lines
    for line in lines:
        tok = line.split()
        if tok and tok[0] in rows:
            rows[tok[0]].append(tok[1:])
    assert np.array_equal(np.asarray(rows['v'], np.float64).astype(np.float32), V)
    vt = np.asarray(rows['vt'], np.float64).astype(np.float32)
    uv = atlas['uv'].reshape(-1, 2)
    assert np.array_equal(vt[:, 0], uv[:, 0]) and np.array_equal(vt[:, 1], np.float32(1.0) - uv[:, 1])            # OBJ's v runs upward
    assert np.array_equal(np.asarray(rows['vn'], np.float64).astype(np.float32), normals[F.reshape(-1)])
    f = np.asarray([[[int(x) for x in corner.split('/')] for corner in face] for face in rows['f']])
    assert np.array_equal(f[..., 0] - 1, F) and np.array_equal(f[..., 1].reshape(-1), np.arange(3 * len(F)) + 1)
    assert np.array_equal(f[..., 1], f[..., 2])
    text = open(mtl).read()
    assert 'newmtl baked' in text and 'map_Kd albedo.png' in text and 'map_Pr orm.png' in text and 'map_Pm orm.png' in text
    _, mtl2 = X.write_obj(str(tmp_path / 'm2.obj'), V, F, atlas['uv'], normals, str(tmp_path / 'tex'))
    assert 'map_Kd tex/albedo.png' in open(mtl2).read()


# ---- 4. commands -------------------------------------------------------------------------------------------------------------------------
def test_bake_textures_command_arguments():
    from nu_nerf_amd.bake_textures import output_paths, parse_args, which_of
    f = parse_args(['--cfg', 'c.yaml'])
    assert (f.size, f.pad, which_of(f)) == (2048, 0, 'outer')
    assert output_paths(f, 'bear', 300000) == (os.path.join('data', 'meshes', 'bear-300000.ply'),
                                               os.path.join('data', 'materials', 'bear-300000', 'texture'), 'bear-300000')
    f = parse_args(['--cfg', 'c.yaml', '--stage2'])
    assert which_of(f) == 'inner'
    assert which_of(parse_args(['--cfg', 'c.yaml', '--stage2', '--which', 'outer'])) == 'outer'
    f = parse_args(['--cfg', 'c.yaml', '--mesh', 'm/x_simplified.ply', '--out', 'o/dir', '--size', '512', '--pad', '2'])
    assert output_paths(f, 'bear', 7) == ('m/x_simplified.ply', 'o/dir', 'x_simplified') and (f.size, f.pad) == (512, 2)
    for bad in (['--mesh', 'm.ply'], ['--cfg', 'c.yaml', '--which', 'inner'], ['--cfg', 'c.yaml', '--stage2', '--which', 'both'],
                ['--cfg', 'c.yaml', '--size', '0'], ['--cfg', 'c.yaml', '--size', '40000'], ['--cfg', 'c.yaml', '--pad', '-1'],
                ['--cfg', 'c.yaml', '--pad', '65']):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_relight_command_texture_arguments():
    from nu_nerf_amd.relight import parse_args
    base = ['--mesh', 'm.ply', '--hdr', 'sky.hdr', '--name', 'n']
    f = parse_args(base + ['--material', 'mat'])
    assert f.texture is None
    f = parse_args(base + ['--texture', 'tex'])                                # the atlas stands in for the per-vertex arrays
    assert f.texture == 'tex' and f.material is None
    f = parse_args(base + ['--material', 'mat', '--texture', 'tex'])
    assert f.texture == 'tex' and f.material == 'mat'
    f = parse_args(['--mesh', 'm.ply', '--name', 'n', '--splitsum', '--pyramid', 'p', '--texture=tex', '--transfer', 'tr'])
    assert f.texture == 'tex' and f.transfer == 'tr'
    with pytest.raises(SystemExit):
        parse_args(base)                                                       # still needs one of the two
    with pytest.raises(SystemExit):
        parse_args(base + ['--texture', 'tex', '--inner', 'i.ply', '--inner-material', 'im'])


# ---- 5. the public surface ---------------------------------------------------------------------------------------------------------------
def test_every_renderer_class_has_predict_textures():
    from nu_nerf_amd import stage2, stage2_thick
    from nu_nerf_amd.compat.network import renderer as c_std, renderer_zerothick as c_zero
    seen = 0
    for reg in (stage2.name2renderer, stage2_thick.name2renderer, c_std.name2renderer, c_zero.name2renderer):
        for cls in reg.values():
            assert callable(getattr(cls, 'predict_textures', None)), cls
            seen += 1
    assert seen == 8


def test_entries_are_declared_and_constants_agree():
    from nu_nerf_amd import _lib, texture as X
    names = {n for n, _, _ in _lib._signatures()}
    assert {'nu_atlas_texels', 'nu_atlas_sample', 'nu_atlas_gbuffer'} <= names
    assert (_lib.NU_ATLAS_CH, _lib.NU_ATLAS_MAX_SIZE, _lib.NU_ATLAS_MAX_PAD) == (X.CH, X.MAX_SIZE, X.MAX_PAD)
    sig = {n: a for n, _, a in _lib._signatures()}
    assert len(sig['nu_atlas_texels']) == 12 and len(sig['nu_atlas_sample']) == 9 and len(sig['nu_atlas_gbuffer']) == 12
