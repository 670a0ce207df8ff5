"""Row-major-staged weight-gradient kernels (csrc/wgrad_rm.hip) through nu_gemm_tn and the engine's queue.

The library picks them by ALIGNMENT alone: 16-byte aligned operands take wgrad_rm256_kernel / wgrad_rm128_kernel, the same operands
copied to a buffer shifted by one float (same ld) take gemm_tn2_kernel / gemm_tn_kernel.  Both must give the same bits, C and db alike."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _buf(gpu, P, ld, seed):
    """(aligned, shifted): the same P x ld matrix at a 16-byte aligned address and one float past one; 128 floats of slack behind
    the last row so that a 64-column window offset stays inside the allocation."""
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    flat = torch.empty(P * ld + 128, device=gpu)
    flat[:P * ld].normal_(generator=g)
    flat[P * ld:] = float("nan")
    sh = torch.empty(P * ld + 132, device=gpu)
    sh[1:1 + P * ld + 128] = flat
    assert flat.data_ptr() % 16 == 0 and sh.data_ptr() % 16 == 0
    return flat, sh


def _tn(lib, L, gpu, a0, lda, b0, ldb, a1, b1, P, N1, N2, S, with_db):
    """a0 / b0 / a1 / b1: device addresses (ints; a1 = b1 = 0 for one pair)."""
    wsb = lib.nu_gemm_tn_workspace_bytes(N1, N2, S)
    ws = torch.empty(wsb // 4, device=gpu)
    C = torch.full((N1, N2), float("nan"), device=gpu)
    bo = torch.full((N1,), float("nan"), device=gpu)
    vp = ctypes.c_void_p
    rc = lib.nu_gemm_tn(vp(a0), lda, vp(b0), ldb, vp(a1) if a1 else None, lda if a1 else 0, vp(b1) if b1 else None, ldb if b1 else 0,
                        P, N1, N2, L.ptr(C), N2, L.ptr(bo) if with_db else None, S, L.ptr(ws), ctypes.c_longlong(wsb), L.stream())
    L.check(rc, "nu_gemm_tn")
    return C, (bo if with_db else None)


def _case(gpu, P, N1, N2, S, lda, ldb, offs):
    """Every variant of one shape: pairs 1 and 2, db present and absent, each window offset; aligned against shifted operands
    (bitwise), against float64 (test_tn_weight_grad's tolerances), and twice for determinism."""
    from nu_nerf_amd import _lib as L
    lib = L.load()
    bufs = [_buf(gpu, P, ld, 1000 * k + P) for k, ld in enumerate((lda, ldb, lda, ldb))]
    tol = 3e-5 * P ** 0.5
    for oa, ob in offs:
        assert oa + N1 <= lda and ob + N2 <= ldb and oa % 4 == 0 and ob % 4 == 0
        win = [torch.as_strided(bufs[k][0], (P, n), (ld, 1), o).double() for k, (ld, n, o) in
               enumerate(((lda, N1, oa), (ldb, N2, ob), (lda, N1, oa), (ldb, N2, ob)))]
        ref1 = win[0].t() @ win[1]
        ref2 = ref1 + win[2].t() @ win[3]
        bref = win[0].sum(0)
        for pairs in (1, 2):
            for with_db in (True, False):
                def addrs(which, shift):
                    o = (oa, ob, oa, ob)
                    return [bufs[k][which].data_ptr() + 4 * (o[k] + shift) if (k < 2 or pairs == 2) else 0 for k in range(4)]
                al, sh = addrs(0, 0), addrs(1, 1)
                assert all(a % 16 == 0 for a in al) and all(a % 16 == 4 for a in sh if a)
                C, bo = _tn(lib, L, gpu, al[0], lda, al[1], ldb, al[2], al[3], P, N1, N2, S, with_db)
                C2, bo2 = _tn(lib, L, gpu, al[0], lda, al[1], ldb, al[2], al[3], P, N1, N2, S, with_db)
                Cs, bos = _tn(lib, L, gpu, sh[0], lda, sh[1], ldb, sh[2], sh[3], P, N1, N2, S, with_db)
                what = (P, N1, N2, S, oa, ob, pairs, with_db)
                assert torch.equal(C, C2), ("not deterministic", what)
                assert torch.equal(C, Cs), ("aligned and shifted operands differ", what, float((C - Cs).abs().max()))
                torch.testing.assert_close(C.double(), ref2 if pairs == 2 else ref1, rtol=2e-5, atol=tol)
                if with_db:
                    assert torch.equal(bo, bo2) and torch.equal(bo, bos), ("db", what, float((bo - bos).abs().max()))
                    torch.testing.assert_close(bo.double(), bref, rtol=2e-5, atol=tol)


@pytest.mark.parametrize("P", [6400, 6500, 12800, 300, 60001])
@pytest.mark.parametrize("N1,N2", [(256, 256), (512, 256)])
def test_256_tile_aligned_equals_shifted(gpu, N1, N2, P):
    """S = 200: 6400 rows = one full chunk per split, 6500 a ragged second chunk, 12800 two chunks, 300 most splits empty.
    Dense operands, then column windows of ld = 352 at offsets 0 and 64 (N1 = 512 does not fit a 352-wide row: A stays dense)."""
    _case(gpu, P, N1, N2, 200, N1, N2, [(0, 0)])
    lda = 352 if N1 == 256 else N1
    _case(gpu, P, N1, N2, 200, lda, 352, [(0, 0), (64 if N1 == 256 else 0, 64), (0, 64)])


@pytest.mark.parametrize("P,N1,N2,S", [(1, 1, 1, 1), (1000, 257, 256, 7), (5000, 256, 39, 16), (333, 3, 256, 4), (4000, 1024, 288, 8),
                                      (3000, 128, 288, 5), (2000, 217, 256, 3)])
def test_128_tile_shapes_aligned_equals_shifted(gpu, P, N1, N2, S):
    """The shapes the 256-tile rule rejects: wgrad_rm128_kernel (aligned) against gemm_tn_kernel (shifted), ragged N1 / N2 included."""
    _case(gpu, P, N1, N2, S, (N1 + 3) // 4 * 4 + 4, (N2 + 3) // 4 * 4, [(0, 0)])


def _plan(items, edge, target, rows_min):
    """nu_wgrad_flush's split of one tile class: items = [(P, N1, N2, groups)] -> [S]."""
    cd = lambda a, b: (a + b - 1) // b
    tiles = [cd(n1, edge) * cd(n2, edge) * g for _, n1, n2, g in items]
    rows = max(cd(sum(p * t for (p, _, _, _), t in zip(items, tiles)), target), rows_min)
    rows = cd(rows, 32) * 32
    while sum(cd(p, rows) * t for (p, _, _, _), t in zip(items, tiles)) > target:
        rows += 32
    return [cd(p, rows) for p, _, _, _ in items]


def test_queue_of_four_items_equals_single_launches(gpu):
    """Two 256 x 256 items on 50 000 rows (one with two pairs), one 1024 x 288 and one with groups = 4, queued in the engine's
    wgrad_batch(): the bits of the single launches with the queue's splits, and of the same queue on shifted operands."""
    from nu_nerf_amd import _lib as L
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params
    lib = L.load()
    cfg = {'is_nerf': True, 'n_samples': 16, 'n_importance': 16, 'n_bg_samples': 8, 'mlp_dtype': 'fp32'}
    net = NeROShapeRenderer(cfg, training=False)
    net.load_param_dict(init_stage1_params(6033))
    eng = net.to(gpu).engine()
    P, P1, G = 50000, 20000, 4
    a = [_buf(gpu, P, 256, 10 + k) for k in range(4)]            # item 0: a[0], a[1]; item 1: two pairs a[0..3]
    c = [_buf(gpu, P1, 1024, 20), _buf(gpu, P1, 288, 21)]        # item 2
    d = [_buf(gpu, G * P * 256, 1, 30), _buf(gpu, G * P * 256, 1, 31)]       # item 3: four groups, stride P * 256
    items2 = [(P, 256, 256, 1), (P, 256, 256, 1), (P, 256, 256, G)]
    S2 = _plan(items2, 256, 256, 256)
    assert sum(s * t for s, t in zip(S2, (1, 1, G))) >= 192       # the queue's 256-tile class fills the chip: it stays one
    S1 = _plan([(P1, 1024, 288, 1)], 128, 1024, 256)

    def queue(which, shift):
        ad = lambda t: t[which].data_ptr() + 4 * shift
        dW = [torch.full(s, float("nan"), device=gpu) for s in ((256, 256), (256, 256), (1024, 288), (G, 256, 256))]
        db = [torch.full(s, float("nan"), device=gpu) for s in ((256,), (256,), (1024,), (G, 256))]
        with eng.wgrad_batch():
            eng.wgrad(ad(a[0]), 256, ad(a[1]), 256, P, 256, 256, dW[0].data_ptr(), 256, db[0].data_ptr())
            eng.wgrad(ad(a[0]), 256, ad(a[1]), 256, P, 256, 256, dW[1].data_ptr(), 256, db[1].data_ptr(), A1=ad(a[2]), lda1=256,
                      B1=ad(a[3]), ldb1=256)
            eng.wgrad(ad(c[0]), 1024, ad(c[1]), 288, P1, 1024, 288, dW[2].data_ptr(), 288, db[2].data_ptr())
            eng.wgrad(ad(d[0]), 256, ad(d[1]), 256, P, 256, 256, dW[3].data_ptr(), 256, db[3].data_ptr(), groups=G, sA0=P * 256,
                      sB0=P * 256, sW=256 * 256, sDb=256)
        eng.flush_reductions()
        torch.cuda.synchronize()
        return dW, db

    dW, db = queue(0, 0)
    dWs, dbs = queue(1, 1)
    for k in range(4):
        assert torch.equal(dW[k], dWs[k]) and torch.equal(db[k], dbs[k]), k
    ad = lambda t: t[0].data_ptr()
    C, bo = _tn(lib, L, gpu, ad(a[0]), 256, ad(a[1]), 256, 0, 0, P, 256, 256, S2[0], True)
    assert torch.equal(C, dW[0]) and torch.equal(bo, db[0])
    C, bo = _tn(lib, L, gpu, ad(a[0]), 256, ad(a[1]), 256, ad(a[2]), ad(a[3]), P, 256, 256, S2[1], True)
    assert torch.equal(C, dW[1]) and torch.equal(bo, db[1])
    C, bo = _tn(lib, L, gpu, ad(c[0]), 1024, ad(c[1]), 288, 0, 0, P1, 1024, 288, S1[0], True)
    assert torch.equal(C, dW[2]) and torch.equal(bo, db[2])
    for z in range(G):
        C, bo = _tn(lib, L, gpu, ad(d[0]) + 4 * z * P * 256, 256, ad(d[1]) + 4 * z * P * 256, 256, 0, 0, P, 256, 256, S2[2], True)
        assert torch.equal(C, dW[3][z]) and torch.equal(bo, db[3][z]), z
    ref = torch.as_strided(a[0][0], (P, 256), (256, 1)).double().t() @ torch.as_strided(a[1][0], (P, 256), (256, 1)).double()
    torch.testing.assert_close(dW[0].double(), ref, rtol=2e-5, atol=3e-5 * P ** 0.5)
