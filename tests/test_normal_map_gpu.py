"""SDF normal maps on the GPU: the first-order jet kernel nu_sdf_grad_fwd (csrc/sdf_grad.hip) against the kernels whose
bits it restates and against float64, the normal lanes of the atlas (texture.bake_textures(normals='sdf'), nu_atlas_sample_normal,
nu_atlas_gbuffer_normal), normal-mapped relighting and the two commands.

Bounds.  Test 3 holds gradient and normal to the bounds tests/test_curvature_gpu.py holds the jet kernel to (BOUND['gradient'] = 3.05e-6
absolute, 4 x the 7.62e-7 measured there against float64; normal 2 BOUND / G_MIN): test 1 shows the bits are the jet's, so its bounds
carry over unchanged (measured here: gradient 7.30e-7, normal 9.27e-7).  Test 6: per-face constants within 4 ulp (measured 1: the
division by the constant's own fp32 length); the smooth field 4 x its first measurement, capped at 1e-5 (DESIGN.md 30's convention).
Test 7: the frames within the bounds tests/test_texture_gpu.py takes from DESIGN.md 20 / 28 (measured 3.7e-7 and 2.3e-7).  Test 8: the
ratio of maximum angular errors >= 10 x, the normal-mapped error 4 x its first measurement.  Every test prints its figure before it
asserts; the figures are in DESIGN.md 32."""
import ctypes
import os

import numpy as np
import pytest
import torch

import curvature_oracle as CO
import texture_oracle as TO
from test_curvature_gpu import BOUND, G_MIN, shell_points, stage1_net, stage2_net
from test_texture_gpu import TOL_LINEAR, TOL_RESOLVE, _env, _frame, bits, dev, ico, rel, vertex_normals

pytestmark = pytest.mark.gpu

T = 16                                               # points per tile of sdf_grad_fwd_kernel


def bake(net, x, which=None):
    from nu_nerf_amd.curvature import bake_normals
    return bake_normals(net, x, which=which)


def flat(out):
    return torch.cat([out['sdf'][:, None], out['gradient'], out['normal']], 1)


@pytest.fixture(scope='module')
def parity(gpu):
    """(net, arrays, x [4096,3], the kernel's outputs) of the parity network: computed once, never modified."""
    net, arrays = stage1_net(gpu)
    x = shell_points(4096, 64, gpu)
    return net, arrays, x, bake(net, x)


# ---- 1. the bits of nu_sdf_fused_fwd (sdf) and nu_sdf_jet_fwd (grad, normal) -----------------------------------------------------------
def test_bit_identity(gpu, parity):
    from nu_nerf_amd.curvature import bake_curvature
    from nu_nerf_amd.engine import addr
    net, _, x, full = parity
    eng = net.engine()
    eng.pack()
    for n in (1, T - 1, T, T + 1, 2 * T + 1, 4096):
        for x_ld in (3, 5):
            xs = x[:n].contiguous()
            if x_ld == 5:
                wide = torch.full((n, 5), float('nan'), device=gpu)    # the other columns are never read
                wide[:, :3] = xs
                xs = wide
            out = bake(net, xs)
            fused = eng.sdf_forward(addr(xs), x_ld, n, keep=False, want_feat=False)['sdf']       # nu_sdf_fused_fwd
            jet = bake_curvature(net, xs)                                                       # nu_sdf_jet_fwd
            assert torch.equal(out['sdf'], fused), (n, x_ld)
            assert torch.equal(out['gradient'], jet['gradient']) and torch.equal(out['normal'], jet['normal']), (n, x_ld)
            assert torch.equal(flat(out), flat(full)[:n]), (n, x_ld)


# ---- 2. row independence -----------------------------------------------------------------------------------------------------------
def test_row_independence_bits(gpu, parity):
    net, _, x, full = parity
    ref = flat(full)
    assert torch.equal(flat(bake(net, x)), ref)                         # two runs, equal bits
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(4096)).to(gpu)
    assert torch.equal(flat(bake(net, x[perm].contiguous())), ref[perm])
    rolled = torch.roll(torch.arange(4096, device=gpu), 1)             # every point in the next slot of its tile (or the next tile)
    assert torch.equal(flat(bake(net, x[rolled].contiguous())), ref[rolled])
    for n in (7, 100, 1001):                                            # prefixes
        assert torch.equal(flat(bake(net, x[:n].contiguous())), ref[:n]), n
    # more tiles than workgroups: the grid-stride tail (258 tiles of 16 points on at most 256 workgroups) repeats the points' bits
    assert torch.equal(flat(bake(net, torch.cat([x, x[:17]]).contiguous())), torch.cat([ref, ref[:17]]))
    for i in np.linspace(0, 4095, 32).astype(int):                      # a point alone against the same point inside 4096
        assert torch.equal(flat(bake(net, x[i:i + 1].contiguous()))[0], ref[i]), i
    for pos in range(T + 1):                                            # every slot of a tile (and the next tile's first), other neighbours
        batch = shell_points(T + 1, 100 + pos, gpu)
        batch[pos] = x[77]
        assert torch.equal(flat(bake(net, batch))[pos], ref[77]), pos


# ---- 3. float64 ----------------------------------------------------------------------------------------------------------------------
def check_float64(name, out, ref):
    g = float(np.abs(out['gradient'].cpu().numpy().astype(np.float64) - ref['gradient']).max())
    n = float(np.abs(out['normal'].cpu().numpy().astype(np.float64) - ref['normal']).max())
    gn = np.linalg.norm(ref['gradient'], axis=1)
    print(f"sdf grad vs float64 ({name}): gradient {g:.3e}  normal {n:.3e}   |g| {gn.min():.3f} .. {gn.max():.3f}")
    assert gn.min() >= G_MIN
    assert g <= BOUND['gradient'], (name, g)
    assert n <= 2 * BOUND['gradient'] / G_MIN, (name, n)                # n = g / |g|: |dn| <= 2 |dg| / |g|


def test_float64(gpu, parity):
    net, arrays, x, out = parity
    check_float64('parity', out, CO.sdf_jet64(arrays, x.cpu().numpy(), device=gpu))
    net, arrays = stage1_net(gpu, init_only=True)
    x = shell_points(4096, 65, gpu)
    check_float64('init', bake(net, x), CO.sdf_jet64(arrays, x.cpu().numpy(), device=gpu))
    net, p2 = stage2_net(gpu)
    x = shell_points(4096, 66, gpu)
    out = bake(net, x)                                                  # a stage-2 renderer's default is its inner SDF
    assert torch.equal(flat(out), flat(bake(net, x, which='inner')))
    check_float64('stage-2 inner', out, CO.sdf_jet64(p2, x.cpu().numpy(), prefix='sdf_network_inner', device=gpu))


# ---- 4. nullable outputs, P = 0, argument errors ---------------------------------------------------------------------------------------
def test_arguments(gpu, parity):
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.engine import addr
    net, _, x, full = parity
    eng = net.engine()
    eng.pack()
    n = 1000
    e = lambda *s: torch.full(s, -7.0, device=gpu)                      # noqa: E731
    want = {'sdf': full['sdf'][:n], 'grad': full['gradient'][:n], 'normal': full['normal'][:n]}
    for keys in (('sdf',), ('grad',), ('normal',), ('sdf', 'normal'), ('grad', 'normal'), ('sdf', 'grad')):
        bufs = {k: e(*want[k].shape) for k in keys}
        eng.sdf_grad(addr(x), 3, n, **bufs)
        assert all(torch.equal(bufs[k], want[k]) for k in keys), keys
    eng.sdf_grad(addr(x), 3, n)                                         # nothing asked for: still a valid call
    only = e(n, 3)
    eng.sdf_grad(addr(x), 3, 0, normal=only)                            # P == 0: nothing launched, nothing written
    assert bool((only == -7.0).all())
    assert {k: tuple(v.shape) for k, v in bake(net, x[:0]).items()} == {'sdf': (0,), 'gradient': (0, 3), 'normal': (0, 3)}
    lib, net_ref, S = eng.lib, ctypes.byref(eng._sdf_net), eng.stream()
    for args in ((None, addr(x), 3, n), (net_ref, None, 3, n), (net_ref, addr(x), 3, -1), (net_ref, addr(x), 2, n), (None, None, 3, 0)):
        with pytest.raises(NuNerfLibraryError, match=r"nu_sdf_grad_fwd failed with code -1"):
            lib.nu_sdf_grad_fwd(*args, None, None, addr(only), S)
    torch.cuda.synchronize()
    assert bool((only == -7.0).all())
    with pytest.raises(ValueError):
        bake(net, x, which='inner')


# ======================================================================================================================================
# The atlas: bake, lookup, G-buffer, relighting, commands
# ======================================================================================================================================
SENTINEL = 1e30
MEASURED_SMOOTH = 9.475e-08     # test 6: largest abs error of the smooth-field lookup against float64, first measurement on an MI355X
CAP_SMOOTH = 1e-5               # DESIGN.md 30's convention: 4 x the first measurement, never above this
MEASURED_GAIN = {'init': 0.01742, 'parity': 0.22330}      # test 8: normal-mapped max angular error (degrees), first measurement on an MI355X
MATERIAL = (0.6, 0.5, 0.4, 0.3, 0.5)


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def pyramid_inputs():
    g = np.random.Generator(np.random.PCG64(13))
    return ((1.0 + g.random((3, 8, 16, 3))).astype(np.float32), np.asarray([0.0, 0.4, 1.0], np.float32),
            (0.5 + g.random((4, 8, 3))).astype(np.float32))


# ---- 5. bake_textures(normals='sdf') ---------------------------------------------------------------------------------------------------
def check_bake(gpu, net, V, F, T, which):
    from nu_nerf_amd import texture as X
    from nu_nerf_amd.curvature import bake_normals
    plain = X.bake_textures(net, V, F, size=T, which=which)
    atlas = X.bake_textures(net, V, F, size=T, which=which, normals='sdf')
    assert set(atlas) == set(plain) | {'normal'} and 'normal' not in plain
    for k in ('albedo', 'metallic', 'roughness', 'face'):
        assert torch.equal(atlas[k], plain[k]), k
    assert np.array_equal(atlas['uv'], plain['uv']) and atlas['layout'] == plain['layout']
    p, f, _ = X.atlas_texels(dev(V, gpu), dev(F, gpu), atlas['layout'])
    own = f >= 0
    n = atlas['normal']
    assert n.dtype == torch.float32 and tuple(n.shape) == (T, T, 3)
    want = bake_normals(net, p[own].contiguous(), which=which)['normal']
    assert torch.equal(n[own], want) and not n[~own].any()
    assert float((n[own].norm(dim=1) - 1).abs().max()) < 1e-6           # the raw SDF normal: unit, nothing flipped
    for rows in (7, 100, T):
        other = X.bake_textures(net, V, F, size=T, which=which, rows_per_pass=rows, normals='sdf')
        assert all(torch.equal(other[k], atlas[k]) for k in ('albedo', 'metallic', 'roughness', 'face', 'normal')), rows
    return atlas


def test_bake_textures_normals_stage1(gpu, parity):
    from nu_nerf_amd import texture as X
    net = parity[0]
    V, F = ico(3)
    atlas = check_bake(gpu, net, V, F, 256, None)
    packed = X.pack_atlas(atlas)
    assert packed.has_normal and torch.equal(packed.tex[1, ..., 1:4], atlas['normal']) and torch.equal(packed.tex[1, ..., 0], atlas['roughness'])
    plain = X.pack_atlas({k: v for k, v in atlas.items() if k != 'normal'})
    assert not plain.has_normal and not plain.tex[1, ..., 1:4].any() and torch.equal(plain.tex[0], packed.tex[0])
    pt = net.predict_textures((V, F), size=256, normals='sdf')
    assert isinstance(pt['normal'], np.ndarray) and np.array_equal(pt['normal'], atlas['normal'].cpu().numpy())
    assert 'normal' not in net.predict_textures((V, F), size=256)
    with pytest.raises(ValueError):
        X.bake_textures(net, V, F, size=256, normals='mesh')


def test_bake_textures_normals_stage2_inner(gpu):
    net, _ = stage2_net(gpu)
    V, F = ico(2)
    atlas = check_bake(gpu, net, V, F, 128, 'inner')
    from nu_nerf_amd import texture as X
    assert torch.equal(X.bake_textures(net, V, F, size=128, normals='sdf')['normal'], atlas['normal'])      # the stage-2 default
    assert not torch.equal(X.bake_textures(net, V, F, size=128, which='outer', normals='sdf')['normal'], atlas['normal'])


# ---- 6. nu_atlas_sample_normal -----------------------------------------------------------------------------------------------------------
def packed_normals(gpu, lay, normal, fill=0.0):
    """A PackedAtlas whose material lanes are `fill` and whose normal lanes are normal [T,T,3]."""
    from nu_nerf_amd import texture as X
    T = lay['size']
    tex = np.full((2, T, T, 4), fill, np.float32)
    tex[1, ..., 1:4] = normal
    return X.PackedAtlas(dev(tex, gpu), lay, True)


@pytest.mark.parametrize("nf,T,pad", [(320, 128, 0), (7, 64, 2), (1, 64, 0)])
def test_sample_normal_sentinel(gpu, nf, T, pad):
    """Every face's texels hold one unit normal, every other texel 1e30 (in all eight lanes): a lookup anywhere in the triangle returns
    the face's normal.  The mix of equal texels is exact, so what remains is the division by the constant's own fp32 length: held to
    4 ulp per component of the constant."""
    from nu_nerf_amd import texture as X
    lay = X.atlas_layout(nf, T, pad)
    owner = TO.owner_map(lay)[0]
    const = unit(np.random.Generator(np.random.PCG64(nf)).standard_normal((nf, 3))).astype(np.float32)
    normal = np.full((T, T, 3), SENTINEL, np.float32)
    normal[owner >= 0] = const[owner[owner >= 0]]
    atlas = packed_normals(gpu, lay, normal, SENTINEL)
    face, u, v = TO.triangle_points(nf, 4096, seed=3)
    assert len(face) >= 4000 + 18 * nf
    got = X.sample_atlas_normal(atlas, face.astype(np.int32), np.stack([u, v], -1).astype(np.float32)).cpu().numpy()
    want = const[face]
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0 + 1e-6   # never the sentinel
    ulp = np.spacing(np.abs(want))
    worst = float((np.abs(got.astype(np.float64) - want) / np.maximum(ulp, np.spacing(np.float32(2.0 ** -20)))).max())
    print(f"sentinel normals ({nf} faces, T = {T}, pad {pad}, {len(face)} points): largest distance {worst:.2f} ulp (bound 4)")
    assert worst <= 4
    far = X.sample_atlas_normal(atlas, np.asarray([0, nf - 1, 0, nf - 1], np.int32), np.asarray([[-3, -3], [7, 0.5], [0.5, 9], [np.nan, np.nan]], np.float32))
    assert np.abs(far.cpu().numpy() - const[[0, nf - 1, 0, nf - 1]]).max() <= 1e-6
    none = X.sample_atlas_normal(atlas, np.asarray([-1, nf, 2 ** 31 - 1], np.int32), np.zeros((3, 2), np.float32))
    assert (none == 0).all()
    zero = packed_normals(gpu, lay, np.zeros((T, T, 3), np.float32), 0.5)         # an atlas without normals: zeros, whatever the materials
    assert not X.sample_atlas_normal(zero, face[:64].astype(np.int32), np.stack([u, v], -1)[:64].astype(np.float32)).any()


def test_sample_normal_smooth(gpu):
    """Texel normals x / |x| (rounded to fp32) at the float64 texel points of the 80-face icosphere, T = 128, pad 1, 1e30 on unowned
    texels: 4096 lookups (every corner, five points per edge, the rest uniform) against the float64 restatement of the same lookup on
    the same fp32 texels and (u, v), renormalised.  Measured on an MI355X: 9.475e-08 (components are below 1, one ulp there is 6e-8);
    bound 4 x that = 3.790e-07, below the cap of 1e-5."""
    from nu_nerf_amd import texture as X
    V, F = ico(1)
    nf = len(F)
    lay = X.atlas_layout(nf, 128, 1)
    owner = TO.owner_map(lay)[0]
    pts = TO.atlas_f64(lay, V.astype(np.float64)[F])
    normal = np.full((128, 128, 3), SENTINEL, np.float32)
    normal[owner >= 0] = unit(pts[owner >= 0]).astype(np.float32)
    atlas = packed_normals(gpu, lay, normal, SENTINEL)
    face, u, v = TO.triangle_points(nf, 4096 - 18 * nf, seed=5)
    uv = np.stack([u, v], -1).astype(np.float32)
    got = X.sample_atlas_normal(atlas, face.astype(np.int32), uv).cpu().numpy().astype(np.float64)
    u64 = uv[:, 0].astype(np.float64)
    v64 = np.minimum(uv[:, 1].astype(np.float64), (np.float32(1.0) - uv[:, 0]).astype(np.float64))      # the kernel's clamp in fp32
    want = unit(TO.lookup_f64(lay, normal.astype(np.float64), face, u64, v64)[0])
    err = float(np.abs(got - want).max())
    bound = min(4 * MEASURED_SMOOTH, CAP_SMOOTH)
    print(f"smooth normal lookup vs float64 ({len(face)} points): max abs err {err:.3e} (bound {bound:.3e})")
    assert np.abs(want).max() <= 1.0 and err <= bound
    assert torch.equal(X.sample_atlas_normal(atlas, face.astype(np.int32), uv), X.sample_atlas_normal(atlas, face.astype(np.int32), uv))


# ---- 7. nu_atlas_gbuffer_normal ----------------------------------------------------------------------------------------------------------
def plane_mesh(n=4):
    """z = 0 over [-0.5, 0.5]^2 as n x n quads, counter-clockwise seen from +z."""
    t = np.linspace(-0.5, 0.5, n + 1)
    x, y = np.meshgrid(t, t, indexing='xy')
    V = np.stack([x.reshape(-1), y.reshape(-1), np.zeros((n + 1) ** 2)], -1).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None]).reshape(-1)
    F = np.concatenate([np.stack([i, i + 1, i + n + 2], -1), np.stack([i, i + n + 2, i + n + 1], -1)]).astype(np.int32)
    return V, F


def plane_scene(gpu, normal, T=128, zero_faces=()):
    """(scene, atlas): the plane with constant materials per vertex and in the atlas, atlas normal = `normal` on every owned texel
    (zero on the texels of zero_faces), 1e30-free: unowned texels are zero as bake_textures leaves them."""
    from nu_nerf_amd import relight as R, texture as X
    V, F = plane_mesh()
    lay = X.atlas_layout(len(F), T, 0)
    owner = TO.owner_map(lay)[0]
    own = owner >= 0
    T_ = lay['size']
    a = {'albedo': np.zeros((T_, T_, 3), np.float32), 'metallic': np.zeros((T_, T_), np.float32), 'roughness': np.zeros((T_, T_), np.float32),
         'normal': np.zeros((T_, T_, 3), np.float32), 'face': owner, 'uv': X.atlas_uv(lay), 'layout': lay}
    a['albedo'][own], a['metallic'][own], a['roughness'][own] = MATERIAL[:3], MATERIAL[3], MATERIAL[4]
    a['normal'][own & ~np.isin(owner, list(zero_faces))] = normal
    scene = R.Scene(V, F, np.tile(np.asarray(MATERIAL, np.float32), (len(V), 1)), device=gpu)
    scene.normals = dev(np.tile(np.asarray([0.0, 0.0, 1.0], np.float32), (len(V), 1)), gpu)
    return scene, X.pack_atlas(a, device=gpu)


def frames(scene, atlas, normal_map, **kw):
    from nu_nerf_amd import relight as R
    poses = R.camera_in_mesh_frame(R.relighting_poses(1, 20.0, 45.0, 2.0))
    pyramid, levels, diffuse = pyramid_inputs()
    mc = R.relight_linear(scene, None, None, _env(), poses, 64, 64, 64, seed=2, texture=atlas, normal_map=normal_map, **kw.get('mc', {}))
    ss = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, 64, 64, texture=atlas, normal_map=normal_map, **kw.get('ss', {}))
    return mc, ss


def test_gbuffer_normal_identity(gpu):
    """(a) the plane z = 0 with vertex normals (0,0,1) and atlas normal (0,0,1): nothing changes, bit for bit."""
    from nu_nerf_amd import relight as R, texture as X
    scene, atlas = plane_scene(gpu, (0.0, 0.0, 1.0))
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    assert 300 < int(pix.shape[0]) < 64 * 64
    g0, g1 = gbuf.clone(), gbuf.clone()
    X.texture_gbuffer(scene, face, g0, pix, atlas)
    X.texture_gbuffer(scene, face, g1, pix, atlas, normals=True)
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    for a, b in zip(frames(scene, atlas, False), frames(scene, atlas, True)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a[..., 3].sum()) == int(pix.shape[0])


def test_gbuffer_normal_constant(gpu):
    """(b) the same plane, atlas normal unit(0.3, 0.2, 1) everywhere: columns 7..9 of the listed hit rows hold that normal's bits
    (divided by its own fp32 length, on the geometric normal's side), nothing else changes, and the frames are those of the scene
    that has this normal at every vertex, within the bounds of the resolves.  (c) faces whose texels hold a zero
    normal keep their shading normal."""
    from nu_nerf_amd import relight as R, texture as X
    n0 = unit(np.asarray([0.3, 0.2, 1.0])).astype(np.float32)
    ln = np.sqrt((n0[0] * n0[0] + n0[1] * n0[1]) + n0[2] * n0[2], dtype=np.float32)
    want = (n0 / ln).astype(np.float32)
    scene, atlas = plane_scene(gpu, n0)
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    some = pix[::3].contiguous()
    miss = (face.reshape(-1) == R.MISS).nonzero().flatten().to(torch.int32)[:5]
    listed_ix = torch.cat([some, miss]).contiguous()                    # a few miss rows are listed too
    X.texture_gbuffer(scene, face, gbuf, pix, atlas)                    # the materials first, as relight does
    before = gbuf.clone()
    assert X.texture_gbuffer(scene, face, gbuf, listed_ix, atlas, normals=True) is gbuf
    rows, old = gbuf.reshape(-1, R.ROW), before.reshape(-1, R.ROW)
    listed = torch.zeros(rows.shape[0], dtype=torch.bool, device=gpu)
    listed[some.long()] = True
    assert torch.equal(rows[~listed].view(torch.int32), old[~listed].view(torch.int32))                   # unlisted and miss rows
    keep = [c for c in range(R.ROW) if not 7 <= c <= 9]
    assert torch.equal(rows[listed][:, keep].view(torch.int32), old[listed][:, keep].view(torch.int32))
    ng = rows[listed][:, 4:7].cpu().numpy()
    sign = np.where((want[None] * ng).sum(1) < 0, np.float32(-1), np.float32(1))[:, None]
    assert np.array_equal(bits(rows[listed][:, 7:10]), bits((sign * want[None]).astype(np.float32)))
    assert (sign == 1).all()                                            # this camera looks at the plane from +z
    # the frames against the scene that has the normal per vertex
    mc, ss = frames(scene, atlas, True)
    scene.normals = dev(np.tile(n0, (int(scene.V.shape[0]), 1)), gpu)
    mc_v, ss_v = frames(scene, atlas, False)
    hit = mc_v[..., 3] > 0
    e_mc = rel(mc[hit][:, :3].cpu().numpy().astype(np.float64), mc_v[hit][:, :3].cpu().numpy().astype(np.float64))
    e_ss = rel(ss[hit][:, :3].cpu().numpy().astype(np.float64), ss_v[hit][:, :3].cpu().numpy().astype(np.float64))
    print(f"normal-mapped plane vs per-vertex normal ({int(hit.sum())} pixels): relight_linear {e_mc:.3e} (bound {TOL_LINEAR:.3e}), "
          f"split sum {e_ss:.3e} (bound {TOL_RESOLVE:.3e})")
    assert e_mc <= TOL_LINEAR and e_ss <= TOL_RESOLVE and torch.equal(mc[..., 3], mc_v[..., 3])
    flat_mc, _ = frames(plane_scene(gpu, n0)[0], atlas, False)
    assert not torch.equal(flat_mc, mc)                                 # and the map does change the frame
    # (c) zero texels: faces 0..7 keep (0,0,1)
    scene, atlas = plane_scene(gpu, n0, zero_faces=range(8))
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    before = gbuf.clone()
    X.texture_gbuffer(scene, face, gbuf, pix, atlas, normals=True)
    rows, old, fid = gbuf.reshape(-1, R.ROW)[pix.long()], before.reshape(-1, R.ROW)[pix.long()], face.reshape(-1)[pix.long()]
    kept = fid < 8
    assert 0 < int(kept.sum()) < int(pix.shape[0])
    assert torch.equal(rows[kept][:, 7:10].view(torch.int32), old[kept][:, 7:10].view(torch.int32))
    assert np.array_equal(bits(rows[~kept][:, 7:10]), bits(np.tile(want, (int((~kept).sum()), 1))))


# ---- 8. the gain on the device -----------------------------------------------------------------------------------------------------------
def gain(gpu, net, arrays, subdiv, name):
    from nu_nerf_amd import relight as R, texture as X
    V, F = ico(subdiv)
    atlas = X.bake_textures(net, V, F, size=256, normals='sdf')
    scene = R.Scene(V, F, None, device=gpu, texture=atlas)
    _, face, gbuf = _frame(gpu, scene, 64, 64)
    pix = R.hit_pixels(face)
    rows = gbuf.reshape(-1, R.ROW)
    x = rows[pix.long()][:, 1:4].cpu().numpy().astype(np.float64)
    truth = CO.sdf_jet64(arrays, x, device=gpu)['normal']
    ng = rows[pix.long()][:, 4:7].cpu().numpy().astype(np.float64)
    truth = np.where(((truth * ng).sum(1) < 0)[:, None], -truth, truth)                 # on the viewer's side, as the G-buffer keeps it
    angle = lambda n: np.degrees(np.arccos(np.clip((unit(n.astype(np.float64)) * truth).sum(1), -1, 1)))      # noqa: E731
    a_vertex = angle(rows[pix.long()][:, 7:10].cpu().numpy())
    X.texture_gbuffer(scene, face, gbuf, pix, scene.texture, normals=True)
    a_map = angle(rows[pix.long()][:, 7:10].cpu().numpy())
    ratio = a_vertex.max() / a_map.max()
    first = MEASURED_GAIN[name]
    print(f"shading normal vs the float64 network normal at the hit point ({name} network, {len(F)} faces, T = 256, {len(x)} pixels): "
          f"per vertex max {a_vertex.max():.4f} deg (mean {a_vertex.mean():.4f}), normal-mapped max {a_map.max():.5f} deg "
          f"(mean {a_map.mean():.5f}); ratio of maxima {ratio:.1f} x; bound on the mapped error {4 * first:.5f} deg")
    return float(a_vertex.max()), float(a_map.max()), float(ratio)


def test_gain_init_network(gpu):
    """80-face icosphere of radius 0.5, init network, T = 256, 64 x 64 frame.  Required: ratio of the maximum angular errors >= 10 x,
    and the normal-mapped error <= 4 x its first measurement.  Measured on an MI355X over 1535 hit pixels: per vertex 22.69 degrees
    (mean 13.42: the init network's level sets are far from the sphere the mesh is), normal-mapped 0.01742 (mean 0.00479), ratio
    1303 x; bound on the mapped error 0.0697 degrees."""
    net, arrays = stage1_net(gpu, init_only=True)
    a_vertex, a_map, ratio = gain(gpu, net, arrays, 1, 'init')
    assert a_map <= 4 * MEASURED_GAIN['init']
    assert ratio >= 10


def test_gain_parity_network(gpu, parity):
    """The same measurement on the parity network over the 320-face sphere: printed, the mapped error bounded the same way.  Measured
    on an MI355X over 1629 hit pixels: per vertex 32.61 degrees, normal-mapped 0.2233 (mean 0.0484; the randomised network's normal
    turns quickly, L = 16 texels a leg), ratio 146 x; bound 0.893 degrees."""
    net, arrays = parity[0], parity[1]
    a_vertex, a_map, ratio = gain(gpu, net, arrays, 2, 'parity')
    assert a_map <= 4 * MEASURED_GAIN['parity']
    assert a_map < a_vertex


# ---- 9. determinism ----------------------------------------------------------------------------------------------------------------------
def test_determinism(gpu, parity):
    from nu_nerf_amd import relight as R, texture as X
    net = parity[0]
    V, F = ico(2)
    a, b = (X.bake_textures(net, V, F, size=128, normals='sdf') for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in ('albedo', 'metallic', 'roughness', 'face', 'normal'))
    scene = R.Scene(V, F, None, device=gpu, texture=a)
    mc, ss = frames(scene, None, True)
    assert float(mc[..., 3].sum()) > 300 and not torch.equal(mc, frames(scene, None, False)[0])
    for kw in ({}, {'mc': dict(rows=7, chunk=24), 'ss': dict(rows=5)}, {'mc': dict(images=2, rows=64), 'ss': dict(images=2)}):
        mc2, ss2 = frames(scene, None, True, **kw)
        assert torch.equal(mc2.view(torch.int32), mc.view(torch.int32)) and torch.equal(ss2.view(torch.int32), ss.view(torch.int32)), kw
    # with transfer=: the baked per-vertex rows are used as they are, the map still moves the frame
    poses = R.camera_in_mesh_frame(R.relighting_poses(1, 20.0, 45.0, 2.0))
    pyramid, levels, diffuse = pyramid_inputs()
    tr = np.zeros((len(V), 16), np.float32)
    tr[:, 9] = 0.7
    tr[:, 10:13] = vertex_normals(V, F)
    sh = [R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, 64, 64, transfer=tr, normal_map=m) for m in (True, True, False)]
    assert torch.equal(sh[0], sh[1]) and not torch.equal(sh[0], sh[2]) and not torch.equal(sh[0], ss)
    # refusals on the device: a texture without normals
    plain = {k: v for k, v in a.items() if k != 'normal'}
    with pytest.raises(ValueError, match='normal_map'):
        R.relight_linear(scene, None, None, _env(), poses, 8, 8, 4, texture=plain, normal_map=True)
    with pytest.raises(ValueError, match='normal_map'):
        R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, 8, 8, texture=plain, normal_map=True)
    _, face, gbuf = _frame(gpu, scene, 8, 8)
    with pytest.raises(ValueError):
        X.texture_gbuffer(scene, face, gbuf, R.hit_pixels(face), X.pack_atlas(plain), normals=True)


# ---- 10. commands and the C entries' arguments ---------------------------------------------------------------------------------------------
def test_commands(gpu, tmp_path, monkeypatch, capsys, parity):
    import json
    import yaml
    from nu_nerf_amd import bake_textures as B, relight, texture as X
    from nu_nerf_amd.mask_render import _pillow
    from nu_nerf_amd.mesh import write_ply
    net = parity[0]
    V, F = ico(1)
    monkeypatch.chdir(tmp_path)
    os.makedirs('data/model/tiny')
    os.makedirs('data/meshes')
    torch.save({'step': 1234, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 'data/model/tiny/model.pth')
    write_ply('data/meshes/tiny-1234.ply', V, F)
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    out = B.main(['--cfg', 'tiny.yaml', '--size', '64', '--pad', '1', '--normals', 'sdf'])
    assert sorted(os.listdir(out)) == ['albedo.png', 'atlas.npz', 'normal.png', 'orm.png', 'tiny-1234.bin', 'tiny-1234.gltf', 'tiny-1234.mtl',
                                       'tiny-1234.obj']
    line = json.loads(capsys.readouterr().out.strip().split('\n')[-1])
    want = X.bake_textures(net, V, F, size=64, pad=1, normals='sdf')
    back = X.load_textures(out, len(F))
    assert np.array_equal(back['normal'], want['normal'].cpu().numpy()) and np.array_equal(back['albedo'], want['albedo'].cpu().numpy())
    image, backfacing = X.tangent_normal_image(back, V, F, count=True)
    assert line['normal_backfacing'] == backfacing and line['normals'] == 'sdf'
    assert np.asarray(_pillow().open(os.path.join(out, 'normal.png'))).tobytes() == image.tobytes()
    doc = json.load(open(os.path.join(out, 'tiny-1234.gltf')))
    assert doc['materials'][0]['normalTexture'] == {'index': 2, 'scale': 1.0} and 'TANGENT' in doc['meshes'][0]['primitives'][0]['attributes']
    assert 'normal' not in open(os.path.join(out, 'tiny-1234.mtl')).read()
    plain = B.main(['--cfg', 'tiny.yaml', '--size', '64', '--pad', '1', '--out', 'plain'])
    assert 'normal.png' not in os.listdir(plain) and 'normalTexture' not in open(os.path.join(plain, 'tiny-1234.gltf')).read()
    # relight --texture DIR --normal-map: one small frame, the function's bytes
    np.save('sky.npy', _env())
    base = ['--mesh', 'data/meshes/tiny-1234.ply', '--hdr', 'sky.npy', '--num', '1', '--width', '24', '--height', '24', '--cam_dist', '2.0']
    poses = relight.camera_in_mesh_frame(relight.relighting_poses(1, 0.0, 45.0, 2.0))
    got = np.asarray(_pillow().open(relight.frame_path(relight.main(base + ['--texture', out, '--normal-map', '--samples', '16', '--name', 'nm']), 0)))
    scene = relight.Scene(V, F, None, device=gpu, texture=back)
    ref = relight.relight(scene, None, None, _env(), poses, 24, 24, 16, normal_map=True).cpu().numpy()[0]
    assert np.array_equal(got, ref) and got[..., 3].max() == 255
    assert not np.array_equal(ref, relight.relight(scene, None, None, _env(), poses, 24, 24, 16).cpu().numpy()[0])
    for bad in (base + ['--material', out, '--normal-map', '--name', 'x'],                                  # no --texture
                base + ['--texture', plain, '--normal-map', '--name', 'x'],                                 # a directory without normals
                base + ['--texture', out, '--normal-map', '--name', 'x', '--inner', 'data/meshes/tiny-1234.ply', '--inner-material', out]):
        with pytest.raises(SystemExit):
            relight.main(bad)


def test_atlas_normal_entry_arguments(gpu):
    """Argument errors of the two new C entries: those of nu_atlas_sample / nu_atlas_gbuffer."""
    from nu_nerf_amd import _lib as L, relight as R
    lib = L.load()
    scene, atlas = plane_scene(gpu, (0.0, 0.0, 1.0), T=64)
    V, F = scene.V, scene.F
    nv, nf, T = int(V.shape[0]), int(F.shape[0]), 64
    null = L.ptr(None)
    fi, uv, out = torch.zeros(4, dtype=torch.int32, device=gpu), torch.zeros(4, 2, device=gpu), torch.full((4, 3), -7.0, device=gpu)

    def sample(a=None, size=T, n_faces=nf, pad=0, f=None, u=None, n=4, o=None):
        return lib.nu_atlas_sample_normal(L.ptr(atlas.tex) if a is None else a, size, n_faces, pad, L.ptr(fi) if f is None else f,
                                          L.ptr(uv) if u is None else u, n, L.ptr(out) if o is None else o, L.stream())
    assert sample(n=0, f=null, u=null, o=null) == 0 and bool((out == -7.0).all())
    for kw in (dict(a=null), dict(f=null), dict(u=null), dict(o=null), dict(n=-1), dict(size=16), dict(n_faces=0), dict(pad=6), dict(pad=-1)):
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_sample_normal failed with code -1"):
            sample(**kw)
    assert sample() == 0
    _, face, gbuf = _frame(gpu, scene, 8, 8)
    pix = R.hit_pixels(face)
    before = gbuf.clone()

    def gb(g=None, fa=None, p=None, n=None, v=None, n_verts=nv, f=None, n_faces=nf, a=None, size=T, pad=0):
        return lib.nu_atlas_gbuffer_normal(L.ptr(gbuf) if g is None else g, L.ptr(face) if fa is None else fa, L.ptr(pix) if p is None else p,
                                           int(pix.shape[0]) if n is None else n, L.ptr(V) if v is None else v, n_verts,
                                           L.ptr(F) if f is None else f, n_faces, L.ptr(atlas.tex) if a is None else a, size, pad, L.stream())
    assert gb(p=null, n=0) == 0
    for kw in (dict(g=null), dict(fa=null), dict(p=null), dict(n=-1), dict(v=null), dict(n_verts=0), dict(f=null), dict(n_faces=0), dict(a=null),
               dict(size=16), dict(pad=6)):
        with pytest.raises(L.NuNerfLibraryError, match="nu_atlas_gbuffer_normal failed with code -1"):
            gb(**kw)
    torch.cuda.synchronize()
    assert torch.equal(gbuf, before) and gb() == 0
