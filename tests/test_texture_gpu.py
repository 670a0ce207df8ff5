"""The texture atlas on the GPU (csrc/texture.hip, nu_nerf_amd/texture.py): nu_atlas_texels bit for bit against the numpy
fp32 oracle, nu_atlas_sample against the float64 oracle, bake_textures against the bake kernel it feeds, nu_atlas_gbuffer on a frame, the
two relighting paths with texture=, the relight command, and the argument errors.

Bounds.  TOL_AFFINE (tests 2 and 4) is four times the largest absolute error of the 5-channel affine lookup measured on an MI355X against
float64 (8.022e-08 at 4096 points, corners and edges included; run to run there is no spread, the margin is for another compiler's
contraction choices) and may not exceed 1e-5.  The sentinel lookup is held to 4 units in the last place of the face's constant (measured:
0, the lerp of equal texels is exact).  The end-to-end frames are held to the bounds tests/test_relight_gpu.py and
tests/test_splitsum_gpu.py hold the resolves to against their float64 oracles.  Every test prints its figure before it asserts."""
import os

import numpy as np
import pytest
import torch

import texture_oracle as TO
from helpers import golden

pytestmark = pytest.mark.gpu

MEASURED_AFFINE = 8.022e-08
TOL_AFFINE = 4 * MEASURED_AFFINE
assert TOL_AFFINE <= 1e-5
SENTINEL = 1e30
PARITY_ATOL = 2.3e-6            # the bake kernel against float64 (tests/test_materials_gpu.py)
TOL_LINEAR = 4 * 3.606e-6       # Monte-Carlo linear radiance, relative to max(|reference|, 1e-2) (tests/test_relight_gpu.py)
TOL_RESOLVE = 4 * 1.886e-6      # split-sum resolve, same measure (tests/test_splitsum_gpu.py)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.int32)


def rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-2)).max())


def ico(subdiv, radius=0.5):
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(subdiv, radius)
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def vertex_normals(V, F):
    from nu_nerf_amd.lbvh import vertex_normals_and_curvature
    return vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F).long())[0].numpy()


def mesh(name):
    """(V, F, vertex normals).  'flat': a regular face, a face with two equal vertices, three collinear vertices, and a regular face whose
    vertex normals are all zero (the geometric fallback); the degenerate faces' vertex normals are zero too (the zero fallback)."""
    if name == 'ico2':
        V, F = ico(2)
        return V, F, vertex_normals(V, F)
    if name == 'seven':
        V, F = ico(1)
        F = np.ascontiguousarray(F[:7])
        return V, F, vertex_normals(*ico(1))
    if name == 'one':
        V = np.asarray([[0.1, 0.2, 0.3], [0.7, -0.2, 0.25], [0.15, 0.9, -0.4]], np.float32)
        n = np.asarray([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0]], np.float32)
        return V, np.asarray([[0, 1, 2]], np.int32), n
    if name == 'flat':
        V = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0.5], [0.3, 0.3, 0.3], [0.6, 0.6, 0.6], [-1, -1, -1], [0, -1, 0.25], [1, -1, 0], [0.5, -2, 1]],
                       np.float32)
        F = np.asarray([[0, 1, 2], [3, 3, 4], [5, 3, 4], [6, 7, 8]], np.int32)
        n = np.zeros((9, 3), np.float32)
        n[:3] = [[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]]
        return V, F, n
    raise KeyError(name)


# ---- 1. nu_atlas_texels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['ico2', 'seven', 'one', 'flat'])
@pytest.mark.parametrize("T", [64, 128, 256])
@pytest.mark.parametrize("pad", [0, 2])
def test_texels_bit_for_bit(gpu, name, T, pad):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd import texture as X
    V, F, VN = mesh(name)
    try:
        lay = X.atlas_layout(len(F), T, pad)
    except ValueError as e:
        # 320 faces need 13 x 13 cells of >= 5 + 3 pad texels: no such atlas at this size.  Both layers say so, nothing is launched
        assert name == 'ico2' and 'smallest size that works is ' + str(13 * (5 + 3 * pad)) in str(e) and T < 13 * (5 + 3 * pad)
        out = torch.empty(T, T, 4, device=gpu)
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_texels failed with code -1"):
            L.load().nu_atlas_texels(L.ptr(dev(V, gpu)), len(V), L.ptr(dev(F, gpu)), len(F), None, T, pad, 0, T, L.ptr(out), None, L.stream())
        return
    face, points, normals = TO.texels_f32(V, F, lay, VN)
    p, f, n = X.atlas_texels(dev(V, gpu), dev(F, gpu), lay, vnormals=dev(VN, gpu))
    assert f.dtype == torch.int32 and tuple(p.shape) == (T, T, 3) and tuple(n.shape) == (T, T, 3)
    assert np.array_equal(f.cpu().numpy(), face)                                # ids: equal as integers
    assert np.array_equal(bits(p), bits(points)), np.abs(p.cpu().numpy() - points).max()
    assert np.array_equal(bits(n), bits(normals)), np.abs(n.cpu().numpy() - normals).max()
    own = face >= 0
    assert np.array_equal(np.unique(face[own]), np.arange(len(F)))
    if name != 'flat':
        ln = np.linalg.norm(normals[own].astype(np.float64), axis=1)
        assert np.abs(ln - 1).max() < 1e-6
    else:
        assert (normals[face == 1] == 0).all() and (normals[face == 2] == 0).all()            # no area, no vertex normal: zero
        geo = np.cross(V[7] - V[6], V[8] - V[6]).astype(np.float64)
        assert np.abs(normals[face == 3] - geo / np.linalg.norm(geo)).max() < 1e-6            # the geometric fallback
        assert np.abs(np.linalg.norm(normals[face == 0].astype(np.float64), axis=1) - 1).max() < 1e-6
    # a corner texel holds its vertex's bits
    xy = X.atlas_corners(lay).astype(np.int64)
    got = p.cpu().numpy()[xy[..., 1], xy[..., 0]]
    assert np.array_equal(bits(got), bits(V[F])) and np.array_equal(face[xy[..., 1], xy[..., 0]], np.repeat(np.arange(len(F))[:, None], 3, 1))
    # without normals: the same points; row chunkings and a second run: the same bits
    p2, f2, n2 = X.atlas_texels(dev(V, gpu), dev(F, gpu), lay)
    assert n2 is None and torch.equal(p2, p) and torch.equal(f2, f)
    for step in (1, 5):
        if step == 1 and T > 64:
            continue                                                            # T launches of one row: once is enough
        parts = [X.atlas_texels(dev(V, gpu), dev(F, gpu), lay, vnormals=dev(VN, gpu), y0=y0, rows=min(step, T - y0)) for y0 in range(0, T, step)]
        for k, whole in enumerate((p, f, n)):
            assert torch.equal(torch.cat([q[k] for q in parts]), whole), (step, k)
    again = X.atlas_texels(dev(V, gpu), dev(F, gpu), lay, vnormals=dev(VN, gpu))
    assert all(torch.equal(a, b) for a, b in zip(again, (p, f, n)))


# ---- 2. nu_atlas_sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,T,pad", [(320, 128, 0), (7, 64, 2), (1, 64, 0), (21, 64, 1)])
def test_sample_sentinel(gpu, nf, T, pad):
    """Every face's texels hold one constant per channel, every other texel 1e30: a lookup anywhere in the triangle -- corners and edges
    included -- returns the constant.  Held to 4 ulp; the lerp of equal values is exact, so the measured distance is 0."""
    from nu_nerf_amd import texture as X
    lay = X.atlas_layout(nf, T, pad)
    owner = TO.owner_map(lay)[0]
    g = np.random.Generator(np.random.PCG64(nf))
    const = g.uniform(0.05, 0.95, (nf, 5)).astype(np.float32)
    tex = np.full((T, T, 5), SENTINEL, np.float32)
    tex[owner >= 0] = const[owner[owner >= 0]]
    atlas = X.pack_atlas(dev(tex, gpu), lay)
    face, u, v = TO.triangle_points(nf, 4096, seed=3)
    got = X.sample_atlas(atlas, face.astype(np.int32), np.stack([u, v], -1).astype(np.float32)).cpu().numpy()
    want = const[face]
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
    print(f"sentinel atlas ({nf} faces, T = {T}, pad {pad}, {len(face)} points): largest distance {ulps} ulp (bound 4)")
    assert ulps <= 4
    # outside the triangle: clamped into it; outside the atlas: zeros
    far = X.sample_atlas(atlas, np.asarray([0, nf - 1, 0, nf - 1], np.int32), np.asarray([[-3, -3], [7, 0.5], [0.5, 9], [np.nan, np.nan]], np.float32))
    assert np.array_equal(far.cpu().numpy(), const[[0, nf - 1, 0, nf - 1]])
    none = X.sample_atlas(atlas, np.asarray([-1, nf, 2 ** 31 - 1], np.int32), np.zeros((3, 2), np.float32))
    assert (none == 0).all()


def _affine_case(gpu, nf=80, T=128, pad=1):
    from nu_nerf_amd import texture as X
    lay = X.atlas_layout(nf, T, pad)
    g = np.random.Generator(np.random.PCG64(17))
    corners = g.uniform(0.05, 0.95, (nf, 3, 5))
    tex = TO.atlas_f64(lay, corners, SENTINEL).astype(np.float32)
    return lay, corners, X.pack_atlas(dev(tex, gpu), lay)


def test_sample_affine(gpu):
    """A 5-channel attribute affine over every face, texels rounded to fp32, 1e30 on unowned texels: 4096 lookups (every corner, five
    points on every edge, the rest uniform in the triangles) against the float64 value at the same fp32 (u, v).  Measured on an MI355X:
    8.022e-08 (the values are below 1, one ulp there is 6e-8); bound 4 x that = 3.209e-07."""
    from nu_nerf_amd import texture as X
    lay, corners, atlas = _affine_case(gpu)
    nf = lay['n_faces']
    face, u, v = TO.triangle_points(nf, 4096 - 18 * nf, seed=5)
    assert len(face) == 4096
    uv = np.stack([u, v], -1).astype(np.float32)
    got = X.sample_atlas(atlas, face.astype(np.int32), uv).cpu().numpy().astype(np.float64)
    u64, v64 = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    v64 = np.minimum(v64, (np.float32(1.0) - uv[:, 0]).astype(np.float64))     # the kernel's clamp, for edge points whose fp32 (u, v) sum past 1
    want = np.einsum('nk,nkc->nc', np.stack([1 - u64 - v64, u64, v64], -1), corners[face])
    err = float(np.abs(got - want).max())
    print(f"affine atlas lookup vs float64 ({len(face)} points): max abs err {err:.3e} (bound {TOL_AFFINE:.3e})")
    assert err <= TOL_AFFINE
    # corners: the texel's bits
    tex = atlas.tex.cpu().numpy()
    xy = X.atlas_corners(lay).astype(np.int64)
    c_face = np.repeat(np.arange(nf), 3).astype(np.int32)
    c_uv = np.tile(np.asarray([[0, 0], [1, 0], [0, 1]], np.float32), (nf, 1))
    at = X.sample_atlas(atlas, c_face, c_uv).cpu().numpy().reshape(nf, 3, 5)
    assert np.array_equal(bits(at[..., :4]), bits(tex[0][xy[..., 1], xy[..., 0]])) and np.array_equal(bits(at[..., 4]), bits(tex[1][xy[..., 1], xy[..., 0], 0]))
    assert torch.equal(X.sample_atlas(atlas, face.astype(np.int32), uv), X.sample_atlas(atlas, face.astype(np.int32), uv))


# ---- 3. bake_textures --------------------------------------------------------------------------------------------------------------------
def overrides_of(g):
    return {k[len('override__'):]: v for k, v in g.items() if k.startswith('override__')}


def stage1_net(gpu, overrides=None):
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    arrays = randomize_for_parity(init_stage1_params(6033), seed=1)
    arrays.update(overrides or {})
    net = NeROShapeRenderer({'name': 'golden'}, training=False)
    net.load_param_dict(arrays)
    return net.to(gpu), arrays


def stage2_net(gpu, overrides=None):
    from nu_nerf_amd.params import init_stage1_params, init_stage2_params, randomize_for_parity
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.stage2 import Stage2Renderer
    s1 = randomize_for_parity(init_stage1_params(6033), seed=1)
    s1cfg = {'is_nerf': True, 'apply_occ_loss': True, 'occ_loss_step': 15000, 'freeze_inv_s_step': 15000}
    cfg = {'name': 's2', 'network': 'stage2', 'is_nerf': True, 'shader_config': {'sphere_direction': False, 'human_light': False},
           'stage1_cfg': s1cfg, 'stage1_mesh_arrays': icosphere(3, 0.5)}
    net = Stage2Renderer(cfg, training=False)
    p2 = randomize_for_parity(init_stage2_params(6033, 7044, {'sphere_direction': False}), seed=3)
    for k, v in s1.items():
        p2['stage1_network.' + k] = v
    p2.update(overrides or {})
    sd = net.state_dict()
    for k in [k for k in p2 if k.startswith('stage1_network.')]:      # the aliases of the same tensors, where the model has them
        if 'color_network.' + k in sd:
            p2['color_network.' + k] = p2[k]
    net.load_param_dict(p2)
    return net.to(gpu), p2


def five(out):
    return torch.cat([out['albedo'], out['metallic'], out['roughness']], 1)


def test_bake_textures_stage1(gpu):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.materials import bake_materials
    from oracle import stage1_oracle as O
    g = golden('materials_stage1.npz')
    net, arrays = stage1_net(gpu, overrides_of(g))
    V, F = ico(3)
    T = 256
    atlas = X.bake_textures(net, V, F, size=T)
    lay = atlas['layout']
    assert lay == X.atlas_layout(1280, T) and lay['cell'] == 9
    assert tuple(atlas['albedo'].shape) == (T, T, 3) and tuple(atlas['metallic'].shape) == (T, T) and tuple(atlas['roughness'].shape) == (T, T)
    assert atlas['face'].dtype == torch.int32 and np.array_equal(atlas['uv'], X.atlas_uv(lay, F))
    p, f, _ = X.atlas_texels(dev(V, gpu), dev(F, gpu), lay)
    assert torch.equal(atlas['face'], f) and np.array_equal(f.cpu().numpy(), TO.owner_map(lay)[0])
    own = f >= 0
    got = torch.cat([atlas['albedo'], atlas['metallic'][..., None], atlas['roughness'][..., None]], -1)
    # owned texels: the bits of the bake kernel at the same points; the others: zero
    pts = p[own].contiguous()
    assert torch.equal(got[own], five(bake_materials(net, pts))) and (got[~own] == 0).all() and int(own.sum()) == 1280 * 36
    for rows in (7, 100, T):
        other = X.bake_textures(net, V, F, size=T, rows_per_pass=rows)
        assert all(torch.equal(other[k], atlas[k]) for k in ('albedo', 'metallic', 'roughness', 'face')), rows
    # the three corners of every face: predict_materials at the vertices, bit for bit
    pm = net.predict_materials((V, F))
    want = np.concatenate([pm['albedo'], pm['metallic'], pm['roughness']], 1)[F.reshape(-1)]
    c_face = np.repeat(np.arange(len(F)), 3).astype(np.int32)
    c_uv = np.tile(np.asarray([[0, 0], [1, 0], [0, 1]], np.float32), (len(F), 1))
    at = X.sample_atlas(atlas, c_face, c_uv).cpu().numpy()
    assert np.array_equal(bits(at), bits(want))
    # 512 texels against the float64 evaluation of the networks
    pick = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).choice(int(own.sum()), 512, replace=False)).to(gpu)
    p64 = {k: torch.from_numpy(np.asarray(v)).double().to(gpu) for k, v in arrays.items() if not k.endswith('FG_LUT')}
    with torch.no_grad():
        x64 = pts[pick].double()
        inp = torch.cat([O.sdf_forward(p64, x64)[:, 1:], x64], -1)
        ref = torch.cat([O.predictor(p64, 'color_network.' + n, inp, 'sigmoid') for n in
                         ('albedo_predictor', 'metallic_predictor', 'roughness_predictor')], 1)
    err = float((got[own][pick].double() - ref).abs().max())
    span = (ref.max(0).values - ref.min(0).values).cpu().numpy()
    print(f"baked texels vs float64 (512 texels): max abs err {err:.3e} (bound {PARITY_ATOL:.1e}); channel spans {np.round(span, 4)}")
    assert (span >= 0.02).all() and err <= PARITY_ATOL
    # predict_textures: the same arrays as numpy
    pt = net.predict_textures((V, F), size=T)
    assert isinstance(pt['albedo'], np.ndarray) and np.array_equal(pt['albedo'], atlas['albedo'].cpu().numpy()) and pt['layout'] == lay
    assert np.array_equal(pt['face'], f.cpu().numpy()) and np.array_equal(pt['roughness'], atlas['roughness'].cpu().numpy())


def test_bake_textures_stage2_inner(gpu):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.materials import bake_materials
    g = golden('materials_stage2_inner.npz')
    net, _ = stage2_net(gpu, overrides_of(g))
    V, F = ico(2)
    T = 128
    atlas = X.bake_textures(net, V, F, size=T, which='inner')
    p, f, _ = X.atlas_texels(dev(V, gpu), dev(F, gpu), atlas['layout'])
    own = f >= 0
    got = torch.cat([atlas['albedo'], atlas['metallic'][..., None], atlas['roughness'][..., None]], -1)
    pts = p[own].contiguous()
    assert torch.equal(got[own], five(bake_materials(net, pts, which='inner')))
    assert not torch.equal(got[own], five(bake_materials(net, pts, which='outer')))
    assert torch.equal(X.bake_textures(net, V, F, size=T)['albedo'], atlas['albedo'])                     # the stage-2 default
    pt = net.predict_textures((V, F), size=T)
    assert np.array_equal(pt['metallic'], atlas['metallic'].cpu().numpy())


# ---- 4. nu_atlas_gbuffer -----------------------------------------------------------------------------------------------------------------
A5 = np.asarray([[0.3, -0.2, 0.1], [-0.25, 0.3, 0.2], [0.1, 0.15, -0.3], [0.4, -0.3, 0.35], [-0.3, 0.4, 0.3]])
B5 = np.asarray([0.5, 0.45, 0.55, 0.5, 0.5])


def affine5(x):
    return np.asarray(x, np.float64) @ A5.T + B5


def wavy(x):
    x = np.asarray(x, np.float64)
    return 0.5 + 0.5 * np.sin(12.0 * x[..., 0]) * np.cos(9.0 * x[..., 1])


def _frame(gpu, scene, h, w, n=1):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.mask_render import _cams
    poses = R.camera_in_mesh_frame(R.relighting_poses(n, 20.0, 45.0, 2.0))
    face, gbuf = R.gbuffer(scene, _cams(R.intrinsics(h, w).astype(np.float32), poses.astype(np.float32), gpu), h, w)
    return poses, face, gbuf


def _affine_scene(gpu, T=128, pad=0):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import texture as X
    V, F = ico(1)
    lay = X.atlas_layout(len(F), T, pad)
    vals = affine5(V)
    assert vals.min() > 0.05 and vals.max() < 0.95
    tex = TO.atlas_f64(lay, vals[F], SENTINEL).astype(np.float32)
    scene = R.Scene(V, F, vals.astype(np.float32), device=gpu)
    return scene, X.pack_atlas(dev(tex, gpu), lay)


def test_gbuffer_affine(gpu):
    """Measured on an MI355X: 1.907e-07 over 512 listed pixels (the barycentrics of the stored hit point are part of it), against the
    bound of test 2, 3.209e-07; the per-vertex columns of the same rows are 2.980e-07 from the same float64 values."""
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import texture as X
    scene, atlas = _affine_scene(gpu)
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    assert 500 < int(pix.shape[0]) < 64 * 64
    some = pix[::3].contiguous()
    before = gbuf.clone()
    out = X.texture_gbuffer(scene, face, gbuf, some, atlas)
    assert out is gbuf
    rows, old = gbuf.reshape(-1, R.ROW), before.reshape(-1, R.ROW)
    listed = torch.zeros(rows.shape[0], dtype=torch.bool, device=gpu)
    listed[some.long()] = True
    assert torch.equal(rows[~listed].view(torch.int32), old[~listed].view(torch.int32))                   # unlisted rows: untouched
    keep = [c for c in range(R.ROW) if not 10 <= c <= 14]
    assert torch.equal(rows[listed][:, keep].view(torch.int32), old[listed][:, keep].view(torch.int32))   # the other columns too
    got = rows[listed][:, 10:15].cpu().numpy().astype(np.float64)
    want = affine5(rows[listed][:, 1:4].cpu().numpy())
    err = float(np.abs(got - want).max())
    vert = float(np.abs(old[listed][:, 10:15].cpu().numpy() - want).max())
    print(f"textured G-buffer, affine materials ({int(listed.sum())} pixels): max abs err {err:.3e} (bound {TOL_AFFINE:.3e}); "
          f"per-vertex columns {vert:.3e}")
    assert err <= TOL_AFFINE
    # a listed miss row is left alone
    miss = (face.reshape(-1) == R.MISS).nonzero().flatten().to(torch.int32)[:5].contiguous()
    g2 = before.clone()
    X.texture_gbuffer(scene, face, g2, miss, atlas)
    assert torch.equal(g2, before)
    # twice: the same bits
    g3 = before.clone()
    X.texture_gbuffer(scene, face, g3, some, atlas)
    assert torch.equal(g3, gbuf)


def test_gbuffer_detail_beyond_the_mesh(gpu):
    """Albedo 0.5 + 0.5 sin(12 x) cos(9 y) on the 80-face icosphere: the rms error of the G-buffer's albedo against the function at the
    stored hit point, per-vertex materials against a 128^2 atlas.  The float64 model gives 104 x; asserted: at least 10 x.  Measured on an
    MI355X over the 1535 hit pixels of the frame: 1.5636e-01 against 1.4679e-03, a ratio of 106.5."""
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import texture as X
    V, F = ico(1)
    T = 128
    lay = X.atlas_layout(len(F), T)
    p, f, _ = X.atlas_texels(dev(V, gpu), dev(F, gpu), lay)
    tex = np.zeros((T, T, 5), np.float32)
    tex[..., 0] = np.where(f.cpu().numpy() >= 0, wavy(p.cpu().numpy()), 0.0)
    atlas = X.pack_atlas(dev(tex, gpu), lay)
    mat = np.zeros((len(V), 5), np.float32)
    mat[:, 0] = wavy(V)
    scene = R.Scene(V, F, mat, device=gpu)
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    rows = gbuf.reshape(-1, R.ROW)
    truth = wavy(rows[pix.long()][:, 1:4].cpu().numpy())
    rms_v = float(np.sqrt(np.mean((rows[pix.long()][:, 10].cpu().numpy() - truth) ** 2)))
    X.texture_gbuffer(scene, face, gbuf, pix, atlas)
    rms_t = float(np.sqrt(np.mean((rows[pix.long()][:, 10].cpu().numpy() - truth) ** 2)))
    print(f"non-affine albedo, 64 x 64 frame ({int(pix.shape[0])} pixels): rms error per-vertex {rms_v:.4e}, 128^2 atlas {rms_t:.4e}, "
          f"ratio {rms_v / rms_t:.1f} (asserted >= 10)")
    assert rms_v >= 10 * rms_t and rms_v > 0.05


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def _env(h=16, w=32):
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing='ij')
    return np.stack([1.0 + 0.3 * np.sin(2 * np.pi * x), 0.8 + 0.4 * y, 1.0 + 0.3 * np.cos(2 * np.pi * x) * (1 - y)], -1).astype(np.float32)


def test_relight_paths_with_texture(gpu):
    from nu_nerf_amd import relight as R
    scene, atlas = _affine_scene(gpu)
    h = w = 32
    poses = R.camera_in_mesh_frame(R.relighting_poses(2, 20.0, 45.0, 2.0))
    env = _env()
    g = np.random.Generator(np.random.PCG64(13))
    pyramid = (1.0 + g.random((3, 8, 16, 3))).astype(np.float32)
    levels = np.asarray([0.0, 0.4, 1.0], np.float32)
    diffuse = (0.5 + g.random((4, 8, 3))).astype(np.float32)
    # Monte-Carlo
    plain = R.relight_linear(scene, None, None, env, poses, h, w, 64, seed=2)
    assert torch.equal(plain, R.relight_linear(scene, None, None, env, poses, h, w, 64, seed=2, texture=None))
    tex = R.relight_linear(scene, None, None, env, poses, h, w, 64, seed=2, texture=atlas)
    hit = plain[..., 3] > 0
    assert torch.equal(tex[..., 3], plain[..., 3]) and 400 < int(hit.sum()) < 2 * h * w
    e = rel(tex[hit][:, :3].cpu().numpy().astype(np.float64), plain[hit][:, :3].cpu().numpy().astype(np.float64))
    print(f"relight_linear, texture vs per-vertex on affine materials ({int(hit.sum())} pixels): max relative deviation {e:.3e} (bound {TOL_LINEAR:.3e})")
    assert e <= TOL_LINEAR and not torch.equal(tex, plain)
    assert torch.equal(tex, R.relight_linear(scene, None, None, env, poses, h, w, 64, seed=2, texture=atlas))
    assert torch.equal(tex, R.relight_linear(scene, None, None, env, poses, h, w, 64, seed=2, texture=atlas, rows=7, chunk=24))
    # split sum, plain and shadowed
    ss = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w)
    assert torch.equal(ss, R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, texture=None))
    ss_t = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, texture=atlas)
    e = rel(ss_t[hit][:, :3].cpu().numpy().astype(np.float64), ss[hit][:, :3].cpu().numpy().astype(np.float64))
    print(f"relight_splitsum_linear, texture vs per-vertex on affine materials: max relative deviation {e:.3e} (bound {TOL_RESOLVE:.3e})")
    assert e <= TOL_RESOLVE and not torch.equal(ss_t, ss) and torch.equal(ss_t[..., 3], ss[..., 3])
    assert torch.equal(ss_t, R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, texture=atlas))
    assert torch.equal(ss_t, R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, texture=atlas, rows=5, images=2))
    tr = np.zeros((int(scene.V.shape[0]), 16), np.float32)
    tr[:, 9] = g.uniform(0.3, 1.0, len(tr))
    tr[:, 10:13] = vertex_normals(*ico(1))
    sh = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, transfer=tr)
    sh_t = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, transfer=tr, texture=atlas)
    e = rel(sh_t[hit][:, :3].cpu().numpy().astype(np.float64), sh[hit][:, :3].cpu().numpy().astype(np.float64))
    print(f"shadowed split sum, texture vs per-vertex: max relative deviation {e:.3e} (bound {TOL_RESOLVE:.3e})")
    assert e <= TOL_RESOLVE and not torch.equal(sh, ss)
    # a Scene that carries the atlas shades from it by default; a dict as load_textures returns it packs to the same texture
    five_ch = torch.cat([atlas.tex[0], atlas.tex[1][..., :1]], -1).cpu().numpy()
    as_dict = {'albedo': five_ch[..., :3], 'metallic': five_ch[..., 3], 'roughness': five_ch[..., 4], 'layout': atlas.layout}
    own = R.Scene(scene.V, scene.F, None, device=gpu, texture=as_dict)
    assert torch.equal(own.texture.tex, atlas.tex)
    assert torch.equal(R.relight_splitsum_linear(own, None, None, pyramid, levels, diffuse, poses, h, w), ss_t)
    with pytest.raises(ValueError):
        R.Scene(*ico(2), np.zeros((162, 5), np.float32), device=gpu, texture=as_dict)                    # an atlas of another mesh


def test_relight_command_with_texture(gpu, tmp_path, monkeypatch):
    from nu_nerf_amd import relight
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.mask_render import _pillow
    from nu_nerf_amd.mesh import write_ply
    monkeypatch.chdir(tmp_path)
    scene, atlas = _affine_scene(gpu, T=64)
    V, F = ico(1)
    write_ply('mesh.ply', V, F)
    five_ch = torch.cat([atlas.tex[0], atlas.tex[1][..., :1]], -1).cpu().numpy()
    owner = TO.owner_map(atlas.layout)[0]
    five_ch[owner < 0] = 0.0
    X.write_textures('tex', {'albedo': five_ch[..., :3], 'metallic': five_ch[..., 3], 'roughness': five_ch[..., 4], 'face': owner,
                             'uv': X.atlas_uv(atlas.layout), 'layout': atlas.layout})
    np.save('sky.npy', _env())
    base = ['--mesh', 'mesh.ply', '--texture', 'tex', '--hdr', 'sky.npy', '--num', '1', '--width', '24', '--height', '24', '--cam_dist', '2.0']
    poses = relight.camera_in_mesh_frame(relight.relighting_poses(1, 0.0, 45.0, 2.0))
    got = np.asarray(_pillow().open(relight.frame_path(relight.main(base + ['--samples', '16', '--name', 'mc']), 0)))
    want = relight.relight(relight.Scene(V, F, None, device=gpu, texture=X.load_textures('tex', len(F))), None, None, _env(), poses, 24, 24, 16)
    assert np.array_equal(got, want.cpu().numpy()[0]) and got[..., 3].max() == 255
    from nu_nerf_amd.environment import DEFAULT_LEVELS, prefilter
    pyramid, diffuse, _ = prefilter(_env(), np.asarray(DEFAULT_LEVELS, np.float32))
    got = np.asarray(_pillow().open(relight.frame_path(relight.main(base + ['--splitsum', '--name', 'ss']), 0)))
    want = relight.relight_splitsum(V, F, np.zeros((len(V), 5), np.float32), pyramid, np.asarray(DEFAULT_LEVELS, np.float32), diffuse, poses, 24, 24,
                                    texture=X.load_textures('tex'))
    assert np.array_equal(got, want.cpu().numpy()[0])
    with pytest.raises(SystemExit):
        relight.main(base + ['--name', 'x', '--inner', 'mesh.ply', '--inner-material', 'tex'])


def test_bake_textures_command(gpu, tmp_path, monkeypatch, capsys):
    import yaml
    from nu_nerf_amd import bake_textures as B
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.mesh import write_ply
    g = golden('materials_stage1.npz')
    net, _ = stage1_net(gpu, overrides_of(g))
    V, F = ico(1)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    os.makedirs('data/meshes')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 'data/model/tiny/model.pth')
    write_ply('data/meshes/tiny-1234.ply', V, F)
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = B.main(['--cfg', 'tiny.yaml', '--size', '64', '--pad', '1'])
    assert out == os.path.join('data', 'materials', 'tiny-1234', 'texture')
    assert sorted(os.listdir(out)) == ['albedo.png', 'atlas.npz', 'orm.png', 'tiny-1234.bin', 'tiny-1234.gltf', 'tiny-1234.mtl', 'tiny-1234.obj']
    assert '80 faces' in capsys.readouterr().out
    want = X.bake_textures(net, V, F, size=64, pad=1)
    back = X.load_textures(out, len(F))
    for k in ('albedo', 'metallic', 'roughness', 'face'):
        assert np.array_equal(back[k], want[k].cpu().numpy()), k
    with pytest.raises(SystemExit, match="smallest size that works is 35"):
        B.main(['--cfg', 'tiny.yaml', '--size', '32'])


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd import relight as R
    from nu_nerf_amd import texture as X
    lib = L.load()
    scene, atlas = _affine_scene(gpu, T=64)
    V, F = scene.V, scene.F
    nv, nf, T = int(V.shape[0]), int(F.shape[0]), 64
    tex4 = torch.empty(T, T, 4, device=gpu)
    nrm4 = torch.empty(T, T, 4, device=gpu)
    vn = dev(vertex_normals(*ico(1)), gpu)
    null = L.ptr(None)

    def texels(v=None, n_verts=nv, f=None, n_faces=nf, vnp=null, size=T, pad=0, y0=0, rows=T, t=None, n=null):
        return lib.nu_atlas_texels(L.ptr(V) if v is None else v, n_verts, L.ptr(F) if f is None else f, n_faces, vnp, size, pad, y0, rows,
                                   L.ptr(tex4) if t is None else t, n, L.stream())
    assert texels() == 0 and texels(vnp=L.ptr(vn), n=L.ptr(nrm4)) == 0 and texels(rows=0, v=null, f=null, t=null) == 0
    for kw in (dict(v=null), dict(f=null), dict(t=null), dict(n_verts=0), dict(n_faces=0), dict(n_faces=-1), dict(size=0), dict(size=32),
               dict(size=32769), dict(pad=-1), dict(pad=65), dict(pad=2), dict(y0=-1), dict(rows=-1), dict(y0=1), dict(y0=60, rows=5),
               dict(vnp=L.ptr(vn)), dict(n=L.ptr(nrm4))):
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_texels failed with code -1"):
            texels(**kw)
    fi, uv, out = torch.zeros(4, dtype=torch.int32, device=gpu), torch.zeros(4, 2, device=gpu), torch.empty(4, 5, device=gpu)

    def sample(a=None, size=T, n_faces=nf, pad=0, f=None, u=None, n=4, o=None):
        return lib.nu_atlas_sample(L.ptr(atlas.tex) if a is None else a, size, n_faces, pad, L.ptr(fi) if f is None else f,
                                   L.ptr(uv) if u is None else u, n, L.ptr(out) if o is None else o, L.stream())
    assert sample() == 0 and sample(n=0, f=null, u=null, o=null) == 0
    for kw in (dict(a=null), dict(f=null), dict(u=null), dict(o=null), dict(n=-1), dict(size=32), dict(n_faces=0), dict(pad=2), dict(pad=-1)):
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_sample failed with code -1"):
            sample(**kw)
    _, face, gbuf = _frame(gpu, scene, 8, 8)
    pix = R.hit_pixels(face)

    def gb(g=None, fa=None, p=None, n=None, v=None, n_verts=nv, f=None, n_faces=nf, a=None, size=T, pad=0):
        return lib.nu_atlas_gbuffer(L.ptr(gbuf) if g is None else g, L.ptr(face) if fa is None else fa, L.ptr(pix) if p is None else p,
                                    int(pix.shape[0]) if n is None else n, L.ptr(V) if v is None else v, n_verts, L.ptr(F) if f is None else f,
                                    n_faces, L.ptr(atlas.tex) if a is None else a, size, pad, L.stream())
    assert gb() == 0 and gb(p=null, n=0) == 0
    for kw in (dict(g=null), dict(fa=null), dict(p=null), dict(n=-1), dict(v=null), dict(n_verts=0), dict(f=null), dict(n_faces=0), dict(a=null),
               dict(size=32), dict(pad=2)):
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_gbuffer failed with code -1"):
            gb(**kw)
    # the Python layer
    with pytest.raises(ValueError):
        X.atlas_texels(V, F, X.atlas_layout(nf + 1, T))
    with pytest.raises(ValueError):
        X.atlas_texels(V, F, atlas.layout, y0=60, rows=5)
    with pytest.raises(ValueError):
        X.pack_atlas(torch.zeros(T, T, 4, device=gpu), atlas.layout)
    with pytest.raises(ValueError):
        X.sample_atlas(atlas, np.zeros(3, np.int32), np.zeros((4, 2), np.float32))
    with pytest.raises(TypeError):
        X.texture_gbuffer(scene, face, gbuf, pix, {'albedo': None})
