"""Split-sum relighting on the device: the prefilter kernel, the pyramid lookup and the resolve against the float64
oracle (tests/splitsum_oracle.py), the closed forms, independence / determinism bit for bit, the tap rule, arguments, what the pyramid
means against the exact learned light and against the Monte-Carlo path, and the two commands.

Bounds against float64 follow the project's custom: measured on the first GPU run, asserted at 4 x that, capped at 1e-4 relative to
max(|ref|, 1e-2).  Measured on an MI355X: see the constants below and the table of DESIGN.md 28."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import relight_oracle as RO
import splitsum_oracle as SO

pytestmark = pytest.mark.gpu

CAP = 1e-4
TOL_PREFILTER = 4 * 1.967e-5    # prefilter vs float64 over the shapes of test 1 (worst: M = 255)
TOL_FULL = 4 * 1.993e-6         # 256 x 512 source, 64 queries
TOL_CONST = 4 * 1.335e-6        # constant map, relative (cap 1e-5)
TOL_LOOKUP = min(4 * 2.673e-5, CAP)      # pyramid lookup: the cap holds
TOL_RESOLVE = 4 * 1.886e-6      # split-sum resolve
TOL_FURNACE = 4 * 1.444e-7      # white furnace of the resolve, absolute (cap 1e-5)
assert TOL_CONST <= 1e-5 and TOL_FURNACE <= 1e-5
assert max(TOL_PREFILTER, TOL_FULL, TOL_LOOKUP, TOL_RESOLVE) <= CAP

A_LIN = (0.3, -0.5, 0.4)
UNION = ['cosine', ('ggx', 0.2), ('ggx', 0.5), ('ggx', 1.0), ('vmf', 0.2), ('vmf', 0.5), ('vmf', 1.0)]
FIVE = ['cosine', ('ggx', 0.2), ('vmf', 0.5), ('ggx', 1.0), ('vmf', 1.0)]
ONES = ['cosine', ('ggx', 0.5), ('vmf', 0.2)]
# DESIGN.md 20, white-furnace table: (metallic, roughness) -> (bound, sigma of the S = 64 estimator)
FURNACE = {(0.0, 0.3): (0.00326, 0.00646), (0.0, 0.6): (0.00849, 0.00471), (0.0, 0.9): (0.01069, 0.00182),
           (1.0, 0.3): (0.01543, 0.05590), (1.0, 0.6): (0.04234, 0.06873), (1.0, 0.9): (0.08966, 0.02732)}


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-2)).max())


def unit_rows(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    d = g.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def sun_values(dirs, seed):
    """50 u^8 with u = (1 + z) / 2, tinted, and one entry at 5e4 (a sun)."""
    u = (1.0 + dirs[:, 2].astype(np.float64)) * 0.5
    rgb = np.zeros((len(dirs), 4), np.float32)
    rgb[:, :3] = (50.0 * u ** 8)[:, None] * np.asarray([1.0, 0.8, 0.6])
    rgb[(seed * 7919) % len(dirs), :3] = 5e4
    return rgb


@functools.lru_cache(maxsize=None)
def point_set(M):
    """(src_dir [M,4], src_rgb [M,4]): the 16 x 32 and 17 x 33 maps as source tables, otherwise a Fibonacci spiral with uneven weights."""
    from nu_nerf_amd.environment import source_table
    if M in (512, 561):
        h, w = (16, 32) if M == 512 else (17, 33)
        sd, _ = source_table(np.zeros((h, w, 3), np.float32))
    else:
        k = np.arange(M) + 0.5
        z, phi = 1.0 - 2.0 * k / M, np.pi * (1.0 + 5.0 ** 0.5) * k
        s = np.sqrt(1.0 - z * z)
        sd = np.stack([s * np.cos(phi), s * np.sin(phi), z, 1.0 + 0.5 * np.sin(k)], 1).astype(np.float32)
    return sd, sun_values(sd[:, :3], M)


def call(gpu, src, dirs, lobes):
    from nu_nerf_amd.environment import prefilter_dirs
    out = prefilter_dirs(src, dirs, lobes, device=gpu)
    assert out.shape == (len(lobes), len(dirs), 4) and bool((out[..., 3] == 1).all())
    return out[..., :3]


# ---- 1. the prefilter against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 255, 256, 257, 512, 561])
def test_prefilter_against_float64(gpu, M):
    from nu_nerf_amd import _lib
    sd, rgb = point_set(M)
    d = unit_rows(1000, 11 + M)
    if M == 1:                                                         # one point: only the hemisphere around it has weight
        d = np.where((d @ sd[0, :3])[:, None] < 0.1, -d, d)
        d = d[np.abs(d @ sd[0, :3]) >= 0.1]
    ref = SO.prefilter(sd, rgb, d, UNION)
    src = (dev(sd, gpu), dev(rgb, gpu))
    ws = _lib.load().nu_env_prefilter_workspace_bytes
    assert (ws(63, M, 5) > 0) == (M > 256) and ws(1000, 256, 5) == 0  # few queries and more than one tile: the split-source path
    worst = 0.0
    for N in (1, 63, 64, 65, len(d)):
        dn = dev(d[:N], gpu)
        for lobes in [FIVE] + [[x] for x in ONES]:
            got = call(gpu, src, dn, lobes).cpu().numpy().astype(np.float64)
            want = np.stack([ref[UNION.index(x), :N] for x in lobes])
            assert np.isfinite(got).all()
            worst = max(worst, rel(got, want))
    print(f"prefilter vs float64, M = {M}: max relative deviation {worst:.3e} (bound {TOL_PREFILTER:.3e})")
    assert worst <= TOL_PREFILTER


# ---- 2. full-size accuracy -----------------------------------------------------------------------------------------------------------
def test_full_size_accuracy(gpu):
    from nu_nerf_amd.environment import source_table
    sd, _ = source_table(np.zeros((256, 512, 3), np.float32))
    rgb = sun_values(sd[:, :3], 3)
    d = unit_rows(64, 5)
    lobes = [('ggx', 0.25), ('ggx', 1.0), 'cosine']
    got = call(gpu, (dev(sd, gpu), dev(rgb, gpu)), dev(d, gpu), lobes).cpu().numpy().astype(np.float64)
    e = rel(got, SO.prefilter(sd, rgb, d, lobes))
    print(f"prefilter vs float64, 256 x 512 source, 64 queries: max relative deviation {e:.3e} (bound {TOL_FULL:.3e})")
    assert e <= TOL_FULL


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------------------
def test_closed_forms(gpu):
    from nu_nerf_amd.environment import latlong_dirs
    env = SO.linear_map(64, 128, A_LIN, latlong_dirs).astype(np.float32)
    d = latlong_dirs(6, 12)
    rhos = (0.1, 0.25, 0.5, 1.0)
    got = call(gpu, env, dev(d, gpu), ['cosine'] + [('vmf', r) for r in rhos]).cpu().numpy().astype(np.float64)
    e_cos = float(np.abs(got[0] - SO.cosine_of_linear(A_LIN, d)[:, None]).max())
    e_vmf = [float(np.abs(got[1 + k] - SO.vmf_of_linear(A_LIN, d, r)[:, None]).max()) for k, r in enumerate(rhos)]
    print(f"closed forms: cosine {e_cos:.2e} (bound 2e-4), vMF {['%.2e' % e for e in e_vmf]} (bound 4e-4)")
    assert e_cos <= 2e-4 and max(e_vmf) <= 4e-4


# ---- 4. constant map -------------------------------------------------------------------------------------------------------------------
def test_constant_map(gpu):
    d = dev(unit_rows(300, 2), gpu)
    worst = 0.0
    for h, w, value in ((1, 1, 0.37), (5, 9, 3.25), (16, 32, 120.0), (64, 128, 1.0)):
        got = call(gpu, np.full((h, w, 3), value, np.float32), d, UNION)
        worst = max(worst, float((got - value).abs().max()) / value)
    print(f"constant map: max relative deviation {worst:.3e} (bound {TOL_CONST:.2e})")
    assert worst <= TOL_CONST


# ---- 5. independence and determinism, bit for bit ------------------------------------------------------------------------------------
def test_independence_and_determinism(gpu):
    from nu_nerf_amd import _lib
    from nu_nerf_amd.environment import latlong_dirs, prefilter, prefilter_dirs, source_table
    sd, rgb = point_set(561)
    src = (dev(sd, gpu), dev(rgb, gpu))
    d = unit_rows(32768, 9)
    ws = _lib.load().nu_env_prefilter_workspace_bytes
    assert ws(32768, 561, 5) == 0 and ws(1000, 561, 5) > 0           # the large call is unsplit, the small ones are split
    big = call(gpu, src, dev(d, gpu), FIVE)
    assert torch.equal(big, call(gpu, src, dev(d, gpu), FIVE))                                   # two runs
    for n in (1, 65, 1000):                                                                       # prefixes: N, whole against split
        assert torch.equal(call(gpu, src, dev(d[:n], gpu), FIVE), big[:, :n])
    perm = np.random.Generator(np.random.PCG64(1)).permutation(1000)                             # position and neighbours
    assert torch.equal(call(gpu, src, dev(d[perm], gpu), FIVE), big[:, dev(perm, gpu)])
    assert torch.equal(call(gpu, src, dev(d[700:701], gpu), FIVE), big[:, 700:701])
    for k, x in enumerate(FIVE):                                                                  # the other lobes of the call
        assert torch.equal(call(gpu, src, dev(d[:1000], gpu), [x])[0], big[k, :1000])
        assert torch.equal(call(gpu, src, dev(d, gpu), [x])[0], big[k])
    assert torch.equal(call(gpu, src, dev(d[:1000], gpu), FIVE[::-1]), big[:, :1000].flip(0))
    sixteen = call(gpu, src, dev(d[:300], gpu), FIVE + UNION + FIVE[:4])
    assert torch.equal(sixteen[:5], big[:, :300])
    # the map form is prefilter_dirs at the texel centres
    env = np.ascontiguousarray(rgb[:, :3].reshape(17, 33, 3))
    pyr, dif, info = prefilter(env, (0.5, 1.0), 6, 12, device=gpu)
    raw = prefilter_dirs(env, latlong_dirs(6, 12), [('ggx', 0.5), ('ggx', 1.0), 'cosine'], device=gpu)[..., :3].cpu().numpy()
    assert info['tapped'] == [] and np.array_equal(pyr.reshape(2, -1, 3), raw[:2]) and np.array_equal(dif.reshape(-1, 3), raw[2])
    assert np.array_equal(source_table(env)[0], sd)


# ---- 6. the tap rule ---------------------------------------------------------------------------------------------------------------------
def test_tapped_levels_are_the_bilinear_tap(gpu):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.environment import latlong_dirs, prefilter
    g = np.random.Generator(np.random.PCG64(8))
    env = (g.random((16, 32, 3)) * 4.0).astype(np.float32)
    pyr, dif, info = prefilter(env, (0.0, 0.05, 0.5, 1.0), 8, 16, device=gpu)         # GGX rho = 0.05: alpha = 2.5e-3, far below the pitch
    assert info['tapped'] == [0, 1] and pyr.shape == (4, 8, 16, 3) and dif.shape == (8, 16, 3)
    tap = R.env_lookup(dev(R.pack_env(env), gpu), dev(latlong_dirs(8, 16), gpu)).cpu().numpy().reshape(8, 16, 3)
    assert np.array_equal(pyr[0], tap) and np.array_equal(pyr[1], tap)
    assert not np.array_equal(pyr[2], tap) and np.abs(pyr[3] - pyr[3].mean((0, 1))).max() < np.abs(tap - tap.mean((0, 1))).max()
    same = prefilter(env, (0.0,), device=gpu)                                          # at the source's size the tap is the map
    assert same[2]['tapped'] == [0] and np.abs(same[0][0] - env).max() <= 1e-5 * env.max()
    v = prefilter(env, (0.0, 1.0), 4, 8, lobe='vmf', diffuse='vmf', device=gpu)        # the IDE's convention: the diffuse map is the rho = 1 level
    assert v[2]['tapped'] == [0] and np.array_equal(v[0][1], v[1])


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    from nu_nerf_amd import _lib
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.environment import prefilter_dirs
    sd_np, rgb_np = point_set(257)
    sd, rgb, d = dev(sd_np, gpu), dev(rgb_np, gpu), dev(unit_rows(40, 1), gpu)
    ref = prefilter_dirs((sd, rgb), d, FIVE)
    assert tuple(prefilter_dirs((sd, rgb), d[:0], FIVE).shape) == (5, 0, 4)                  # N = 0 works
    assert torch.equal(prefilter_dirs((sd_np, rgb_np), d.cpu().numpy(), FIVE, device=gpu), ref)      # arrays are taken to the device
    wide = torch.zeros(40, 8, device=gpu)
    for bad in (wide[:, :3], d.double(), d.half(), d[:, :2].contiguous(), d.reshape(-1), d.t().contiguous().t(), d.cpu()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            prefilter_dirs((sd, rgb), bad, FIVE)
    for bad in (sd.double(), sd[:, :3].contiguous(), sd.cpu(), sd.t().contiguous().t(), sd[:-1].contiguous()):
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            prefilter_dirs((bad, rgb), d, FIVE)
        with pytest.raises(NuNerfLibraryError, match=r"code -1"):
            prefilter_dirs((sd, bad), d, FIVE)
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        prefilter_dirs((sd, rgb), d, [])
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):
        prefilter_dirs((sd, rgb), d, ['cosine'] * 17)
    for bad in ([('phong', 0.5)], [('vmf', 0.0)], [('vmf', -1.0)]):
        with pytest.raises(ValueError):
            prefilter_dirs((sd, rgb), d, bad)
    # the C entry: every NU_ERR_ARG case launches nothing
    lib, S = _lib.load(), _lib.stream()
    out = torch.full((2, 40, 4), -7.0, device=gpu)
    need = lib.nu_env_prefilter_workspace_bytes(40, 257, 2)
    ws = torch.empty(max(need, 16) // 4, device=gpu)
    ints, flts = lambda *v: (ctypes.c_int * len(v))(*v), lambda *v: (ctypes.c_float * len(v))(*v)      # noqa: E731
    p = lambda t: t.data_ptr()                                                                          # noqa: E731
    good = [p(sd), p(rgb), 257, p(d), 40, ints(1, 2), flts(0.25, 2.0), 2, p(out), p(ws), need, S]

    def with_(**kw):
        names = ['sd', 'rgb', 'M', 'd', 'N', 'kind', 'param', 'L', 'out', 'ws', 'need', 'S']
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    for args in (with_(sd=None), with_(rgb=None), with_(d=None), with_(out=None), with_(kind=None), with_(param=None), with_(M=-1),
                 with_(N=-1), with_(L=0), with_(L=17), with_(kind=ints(1, 3)), with_(kind=ints(-1, 2)), with_(param=flts(0.0, 2.0)),
                 with_(param=flts(-0.5, 2.0)), with_(param=flts(0.25, 0.0)), with_(param=flts(0.25, -3.0)),
                 with_(param=flts(float('nan'), 2.0)), with_(param=flts(0.25, float('inf')))):
        with pytest.raises(NuNerfLibraryError, match=r"nu_env_prefilter failed with code -1"):
            lib.nu_env_prefilter(*args)
    if need:
        for args in (with_(ws=None), with_(need=need - 1)):
            with pytest.raises(NuNerfLibraryError, match=r"nu_env_prefilter failed with code -3"):
                lib.nu_env_prefilter(*args)
    assert lib.nu_env_prefilter(*with_(N=0)) == 0 and lib.nu_env_prefilter(*with_(M=0)) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                                   # nothing was launched
    assert lib.nu_env_prefilter(*with_(kind=ints(0, 2), param=flts(-1.0, 2.0))) == 0   # the cosine lobe reads no parameter
    torch.cuda.synchronize()
    assert torch.equal(out, prefilter_dirs((sd, rgb), d, ['cosine', ('vmf', 0.5)]))


# ---- 8. the pyramid lookup -------------------------------------------------------------------------------------------------------------
def test_pyramid_lookup(gpu):
    from nu_nerf_amd import _lib
    from nu_nerf_amd import relight as R
    g = np.random.Generator(np.random.PCG64(6))
    pyramid = (g.random((3, 8, 16, 3)) * 10.0 ** g.uniform(-1, 1, (3, 8, 16, 1))).astype(np.float32)
    levels = np.asarray([0.1, 0.45, 0.9], np.float32)
    packed, lv = R.pack_pyramid(pyramid, levels)
    pyr = dev(packed, gpu)
    d = unit_rows(1000, 7)
    d[:4] = [[0, 0, 1], [0, 0, -1], [-1, 1e-7, 0], [-1, -1e-7, 0]]
    rho = g.uniform(-0.2, 1.2, 1000).astype(np.float32)
    rho[:300] = np.repeat(levels, 100)                                  # exactly at each level
    rho[300:320], rho[320:340] = 0.0999, 0.9001                         # just below the first, just above the last
    dd, rr = dev(d, gpu), dev(rho, gpu)
    got = R.pyramid_lookup(pyr, lv, dd, rr)
    e = rel(got.cpu().numpy().astype(np.float64), SO.pyramid_lookup(pyramid, levels, d, rho))
    print(f"pyramid lookup vs float64 (1000 rows): max relative deviation {e:.3e} (bound {TOL_LOOKUP:.3e})")
    assert e <= TOL_LOOKUP
    taps = [R.env_lookup(pyr[k].contiguous(), dd) for k in range(3)]
    for k in range(3):                                                   # at a level: the bits of env_lookup on that level
        assert torch.equal(got[100 * k:100 * (k + 1)], taps[k][100 * k:100 * (k + 1)])
    below, above = rr < 0.1, rr > 0.9
    assert int(below.sum()) > 50 and int(above.sum()) > 50
    assert torch.equal(got[below], taps[0][below]) and torch.equal(got[above], taps[2][above])
    for k in range(3):                                                   # L = 1: that level's tap whatever rho
        assert torch.equal(R.pyramid_lookup(pyr[k:k + 1].contiguous(), lv[k:k + 1], dd, rr), taps[k])
    assert tuple(R.pyramid_lookup(pyr, lv, dd[:0], rr[:0]).shape) == (0, 3)
    with pytest.raises(_lib.NuNerfLibraryError, match=r"code -1"):
        R.pyramid_lookup(pyr, lv[:2], dd, rr)
    with pytest.raises(_lib.NuNerfLibraryError, match=r"code -1"):
        R.pyramid_lookup(pyr, lv, dd, rr[:-1].contiguous())
    with pytest.raises(_lib.NuNerfLibraryError, match=r"code -1"):
        R.pyramid_lookup(pyr, lv, dd.double(), rr)
    with pytest.raises(_lib.NuNerfLibraryError, match=r"nu_env_pyramid_lookup failed with code -1"):
        R.pyramid_lookup(pyr, np.asarray([0.1, 0.1, 0.9], np.float32), dd, rr)        # levels must ascend strictly


# ---- 9. the resolve ----------------------------------------------------------------------------------------------------------------------
def _material_scene(gpu):
    """320-face icosphere, per-vertex materials spanning metallic 0..1 and roughness 0..1; three cameras outside, one inside."""
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.lbvh import icosphere
    from test_relight_gpu import _look_at_inside, _orbit
    V, F = icosphere(2, 0.5)
    g = np.random.Generator(np.random.PCG64(12))
    mat = g.uniform(0.05, 0.95, (len(V), 5)).astype(np.float32)
    mat[:, 3], mat[:, 4] = g.permutation(np.linspace(0.0, 1.0, len(V))), g.permutation(np.linspace(0.0, 1.0, len(V)))
    poses = np.concatenate([_orbit(3, dist=2.0), _look_at_inside()[None]])
    return R.Scene(V, F, mat, device=gpu), poses


def test_resolve_against_float64(gpu):
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.mask_render import _cams
    from nu_nerf_amd.params import load_fg_lut
    scene, poses = _material_scene(gpu)
    h = w = 32
    g = np.random.Generator(np.random.PCG64(13))
    pyramid = (g.random((3, 8, 16, 3)) * 3.0).astype(np.float32)
    levels = np.asarray([0.0, 0.4, 1.0], np.float32)
    diffuse = g.random((4, 8, 3)).astype(np.float32)
    lut = load_fg_lut()[0].astype(np.float64)
    lin = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, images=4)
    face, gbuf = R.gbuffer(scene, _cams(R.intrinsics(h, w).astype(np.float32), poses.astype(np.float32), gpu), h, w)
    hit = (face.reshape(-1) != R.MISS).cpu().numpy()
    rows = gbuf.reshape(-1, R.ROW).cpu().numpy().astype(np.float64)[hit]
    flat = lin.reshape(-1, 4).cpu().numpy()
    assert hit.reshape(4, -1)[3].all() and 0 < hit.reshape(4, -1)[0].sum() < h * w           # the inside camera sees the mesh everywhere
    assert (flat[~hit] == 0).all() and (flat[hit, 3] == 1).all()                             # misses: four zeros; hits: alpha 1
    e = rel(flat[hit, :3].astype(np.float64), SO.resolve(rows, pyramid, levels, diffuse, lut))
    print(f"split-sum resolve vs float64 ({hit.sum()} pixels): max relative deviation {e:.3e} (bound {TOL_RESOLVE:.3e})")
    assert e <= TOL_RESOLVE
    # white furnace: ones in, (1 - m) a + F0 A + B out, against the table read in float64
    white = R.relight_splitsum_linear(scene, None, None, np.ones((2, 4, 8, 3), np.float32), [0.0, 1.0], np.ones((4, 8, 3), np.float32), poses, h, w,
                                      images=4).reshape(-1, 4).cpu().numpy()[hit, :3].astype(np.float64)
    n, a, m, rho, v = rows[:, 7:10], rows[:, 10:13], rows[:, 13:14], rows[:, 14], rows[:, 15:18]
    ab = RO.fg_lookup(lut, np.sum(n * v, 1), rho)
    dev_f = float(np.abs(white - ((1 - m) * a + (0.04 * (1 - m) + m * a) * ab[:, :1] + ab[:, 1:])).max())
    print(f"split-sum white furnace: max absolute deviation {dev_f:.3e} (bound {TOL_FURNACE:.2e})")
    assert dev_f <= TOL_FURNACE
    # chunk invariance
    for kw in (dict(rows=7), dict(rows=11, images=2), dict(images=1), dict(images=3), dict(rows=7, images=3)):
        assert torch.equal(lin, R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w, **kw)), kw
    img = R.relight_splitsum(scene, None, None, pyramid, levels, diffuse, poses, h, w)
    assert img.dtype == torch.uint8 and torch.equal(img, R.to_srgb8(lin))


# ---- 10. meaning: the learned light ------------------------------------------------------------------------------------------------------
def test_exported_pyramid_against_the_exact_learned_light(gpu):
    """The exported pyramid stands for the network: L(r, rho) and Ld(n) read from it against environment.bake_light at the same rows.
    What separates them is the grid (bilinear in direction, linear in roughness), so the finer pyramid must be closer."""
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.environment import bake_light, environment_map
    from test_environment_gpu import stage1_net
    net, _ = stage1_net(gpu, False)
    d = unit_rows(2000, 21)
    rho = np.random.Generator(np.random.PCG64(22)).uniform(0.0, 1.0, 2000).astype(np.float32)
    dd, rr = dev(d, gpu), dev(rho, gpu)
    exact = bake_light(net, dd, rr)['light']
    exact_d = bake_light(net, dd, 1.0)['light']
    figs = []
    for nl, h, w in ((3, 16, 32), (9, 64, 128)):
        levels = np.linspace(0.0, 1.0, nl).astype(np.float32)
        packed, lv = R.pack_pyramid(environment_map(net, h, w, levels), levels)
        pyr = dev(packed, gpu)
        spec = float(((R.pyramid_lookup(pyr, lv, dd, rr) - exact).abs() / exact.abs().clamp_min(1e-2)).max())
        diff = float(((R.env_lookup(pyr[-1].contiguous(), dd) - exact_d).abs() / exact_d.abs().clamp_min(1e-2)).max())
        figs.append((spec, diff))
        print(f"exported pyramid vs exact learned light, {nl} levels {h} x {w}: L(r, rho) max relative deviation {spec:.3e}, Ld(n) {diff:.3e}")
    assert figs[1][0] < figs[0][0] and figs[1][1] < figs[0][1]


# ---- 11. meaning: a foreign light --------------------------------------------------------------------------------------------------------
def test_split_sum_against_the_monte_carlo_path(gpu):
    """A convex 1 280-face icosphere under E = 1 + a.omega: the split-sum image against relight_linear at S = 1024, over the pixels with
    N.V >= 0.2.  The mean difference stays below the white-furnace bound of the material (what separates the estimator
    from the table) plus the Monte-Carlo sigma / sqrt(pixels) it lists."""
    from nu_nerf_amd import relight as R
    from nu_nerf_amd.environment import latlong_dirs, prefilter
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _cams
    from test_relight_gpu import _orbit
    env = SO.linear_map(64, 128, A_LIN, latlong_dirs).astype(np.float32)
    levels = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
    pyramid, diffuse, _ = prefilter(env, levels, 32, 64, device=gpu)
    V, F = icosphere(3, 0.5)
    scene = R.Scene(V, F, np.zeros((len(V), 5), np.float32), device=gpu)
    h = w = 96
    poses = _orbit(3, dist=2.0)[1:2]
    face, gbuf = R.gbuffer(scene, _cams(R.intrinsics(h, w).astype(np.float32), poses.astype(np.float32), gpu), h, w)
    g = gbuf.reshape(-1, R.ROW)
    sel = ((face.reshape(-1) != R.MISS) & ((g[:, 7:10] * g[:, 15:18]).sum(1) >= 0.2))
    npix = int(sel.sum())
    assert npix >= 1000
    for (metallic, roughness), (bound, sigma) in FURNACE.items():
        scene.materials[:] = torch.tensor([0.8, 0.8, 0.8, metallic, roughness], device=gpu)
        ss = R.relight_splitsum_linear(scene, None, None, pyramid, levels, diffuse, poses, h, w).reshape(-1, 4)[sel, :3]
        mc = R.relight_linear(scene, None, None, env, poses, h, w, 1024, seed=3).reshape(-1, 4)[sel, :3]
        mean, worst = float((ss - mc).mean(0).abs().max()), float((ss - mc).abs().max())
        limit = bound + sigma / npix ** 0.5
        print(f"split-sum vs Monte-Carlo S = 1024, metallic {metallic} roughness {roughness}, {npix} pixels: mean difference {mean:.5f} "
              f"(bound {limit:.5f}), max {worst:.5f}")
        assert mean <= limit, (metallic, roughness, mean, limit)


# ---- 12. the commands --------------------------------------------------------------------------------------------------------------------
def test_commands(gpu, tmp_path, monkeypatch, capsys):
    import yaml
    from nu_nerf_amd import extract_environment, prefilter_environment, relight
    from nu_nerf_amd.environment import prefilter
    from nu_nerf_amd.lbvh import icosphere
    from nu_nerf_amd.mask_render import _pillow
    from nu_nerf_amd.mesh import write_ply
    from test_environment_gpu import stage1_net
    from test_relight_gpu import _env, _orbit
    monkeypatch.chdir(tmp_path)
    env = _env(16, 32)
    np.save('sky.npy', env)
    # prefilter_environment writes its six files
    out = prefilter_environment.main(['--hdr', 'sky.npy', '--height', '8', '--width', '16', '--roughness', '0', '0.5', '1'])
    assert out == os.path.join('data', 'environment', 'sky-prefiltered')
    assert sorted(os.listdir(out)) == ['env.hdr', 'env.npy', 'env.png', 'env_diffuse.npy', 'env_pyramid.npy', 'roughness.npy']
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    pyr, dif, info = prefilter(env, (0.0, 0.5, 1.0), 8, 16, device=gpu)
    assert np.array_equal(np.load(os.path.join(out, 'env_pyramid.npy')), pyr) and np.array_equal(np.load(os.path.join(out, 'env_diffuse.npy')), dif)
    assert np.array_equal(np.load(os.path.join(out, 'env.npy')), pyr[0]) and np.array_equal(np.load(os.path.join(out, 'roughness.npy')), [0.0, 0.5, 1.0])
    assert line['shape'] == [3, 8, 16, 3] and line['tapped'] == info['tapped'] == [0] and line['source'] == [16, 32]
    assert line['paths']['diffuse'] == os.path.join(out, 'env_diffuse.npy') and _pillow().open(os.path.join(out, 'env.png')).size == (16, 8)
    assert relight.read_hdr(os.path.join(out, 'env.hdr')).shape == (8, 16, 3)
    # a mesh with baked materials
    V, F = icosphere(2, 0.5)
    V = np.asarray(V, np.float32)
    g = np.random.Generator(np.random.PCG64(2))
    mat = g.uniform(0.1, 0.9, (len(V), 5)).astype(np.float32)
    write_ply('ball.ply', V, F)
    os.makedirs('mat')
    np.save('mat/albedo.npy', mat[:, :3])
    np.save('mat/metallic.npy', mat[:, 3:4])
    np.save('mat/roughness.npy', mat[:, 4:5])
    base = ['--mesh', 'ball.ply', '--material', 'mat', '--num', '2', '--width', '24', '--height', '24', '--cam_dist', '2']
    poses = _orbit(2, az=0.0, dist=2.0)

    def frame(directory, k):
        return np.asarray(_pillow().open(relight.frame_path(directory, k))).copy()
    # --splitsum --hdr: the map is prefiltered at the default levels
    frames = relight.main(base + ['--splitsum', '--hdr', 'sky.npy', '--name', 'a'])
    assert '--samples, --seed and --chunk are not used' in capsys.readouterr().out
    p5, d5, _ = prefilter(env, device=gpu)
    want = relight.relight_splitsum(V, F, mat, p5, [0.0, 0.25, 0.5, 0.75, 1.0], d5, poses, 24, 24).cpu().numpy()
    assert np.array_equal(frame(frames, 0), want[0]) and np.array_equal(frame(frames, 1), want[1])
    assert want[..., 3].max() == 255 and want[..., :3][want[..., 3] == 255].max() > 60
    # --splitsum --pyramid on what prefilter_environment wrote (its own diffuse map) ...
    frames = relight.main(base + ['--splitsum', '--pyramid', out, '--name', 'b'])
    want = relight.relight_splitsum(V, F, mat, pyr, [0.0, 0.5, 1.0], dif, poses, 24, 24).cpu().numpy()
    assert np.array_equal(frame(frames, 1), want[1])
    # ... and on a directory written by extract_environment as it is: the diffuse map is the level of roughness 1
    net, _ = stage1_net(gpu, False)
    os.makedirs('data/model/tiny')
    torch.save({'step': 7, 'best_para': 0, 'network_state_dict': {k: v.cpu() for k, v in net.state_dict().items()}}, 'data/model/tiny/model.pth')
    with open('tiny.yaml', 'w') as fh:
        yaml.safe_dump({'name': 'tiny', 'network': 'shape'}, fh)
    learned = extract_environment.main(['--cfg', 'tiny.yaml', '--height', '8', '--width', '16', '--roughness', '0', '0.5', '1'])
    assert not os.path.exists(os.path.join(learned, 'env_diffuse.npy'))
    frames = relight.main(base + ['--splitsum', '--pyramid', learned, '--name', 'c'])
    lp = np.load(os.path.join(learned, 'env_pyramid.npy'))
    want = relight.relight_splitsum(V, F, mat, lp, [0.0, 0.5, 1.0], lp[2], poses, 24, 24).cpu().numpy()
    assert np.array_equal(frame(frames, 0), want[0]) and want[..., :3][want[..., 3] == 255].max() > 0
    # --splitsum with --inner raises
    with pytest.raises(SystemExit):
        relight.main(['--mesh', 'ball.ply', '--inner', 'ball.ply', '--inner-material', 'mat', '--splitsum', '--hdr', 'sky.npy', '--name', 'd'])
    # without --splitsum the command is the Monte-Carlo path, byte for byte what the library call gives
    frames = relight.main(base + ['--hdr', 'sky.npy', '--name', 'e', '--samples', '16'])
    want = relight.relight(V, F, mat, env, poses, 24, 24, 16, 0).cpu().numpy()
    assert np.array_equal(frame(frames, 0), want[0]) and np.array_equal(frame(frames, 1), want[1])
