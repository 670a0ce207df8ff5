"""A numpy model of the operand mapping of csrc/wgrad_rm.hip: the 256 x 256 tile (8 waves, wave tile 64 x 128) and the 128 x 128
tile (4 waves, wave tile 64 x 64).

v_mfma_f32_32x32x2_f32: lane l supplies A[i = l & 31][k = l >> 5] and B[j = l & 31][k = l >> 5]; accumulator register r of lane l
is C[i = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][j = l & 31] (the layout the present slab store of gemm_tn.hip relies on)."""
import numpy as np

TBK = 32


def quad_clamp(n0, lane, N, ld):
    """Quad index the loader fetches (wgrad_rm.hip ld_begin)."""
    return min(n0 // 4 + lane, min((N - 1) // 4, ld // 4 - 1))


def load_stage(X, ld, N, n0, p_begin, p_end, kt, touched, T=256):
    """One operand's [32][T] stage of chunk kt, as the waves fetch and hand it over.  X: flat operand (P * ld floats).
    T = 256: wave w, load e = point 4 w + e, lane = quad.  T = 128: point 8 w + 4 (lane >> 5) + e, quad lane & 31."""
    st = np.full((TBK, T), np.nan)
    for w in range(T // 32):
        for e in range(4):
            for lane in range(64):
                if T == 256:
                    row, quad = 4 * w + e, lane
                else:
                    row, quad = 8 * w + 4 * (lane >> 5) + e, lane & 31
                p = p_begin + kt * TBK + row
                pr = min(p, p_end - 1)
                byte = pr * ld * 4 + quad_clamp(n0, quad, N, ld) * 16
                touched.append((byte, byte + 16))
                assert np.isnan(st[row, 4 * quad]).all()                  # every stage element is written once
                st[row, 4 * quad: 4 * quad + 4] = X[byte // 4: byte // 4 + 4] if p < p_end else 0.0
    assert not np.isnan(st).any()
    return st


def model_tile(A, lda, B, ldb, P, N1, N2, n1_0, n2_0, T=256):
    """The tile's T x T outputs through stage reads, MFMA steps and the slab store; plus the sequence of point pairs."""
    NJ = T // 64                                          # B tiles of a wave (its columns: 32 NJ); waves as (T / 64) x 2
    lanes = np.arange(64)
    li, lh = lanes & 31, lanes >> 5
    slab = np.zeros((T, T))
    writes = np.zeros((T, T), dtype=int)
    touched, pairs = [], []
    ntile = (P + TBK - 1) // TBK
    nw = T // 32
    acc = np.zeros((nw, 2, NJ, 64, 16))                   # [wave][i][j][lane][r]
    r = np.arange(16)
    rrow = (r & 3) + 8 * (r >> 2)
    for kt in range(ntile):
        sA = load_stage(A, lda, N1, n1_0, 0, P, kt, touched, T)
        sB = load_stage(B, ldb, N2, n2_0, 0, P, kt, touched, T)
        for s in range(16):
            row = 8 * (s >> 2) + (s & 3) + 4 * lh         # per lane
            pairs.append((kt * TBK + row[0], kt * TBK + row[32]))
            for w in range(nw):
                wr, wc = w >> 1, w & 1
                fa = np.stack([sA[row, 64 * wr + 2 * li + i] for i in range(2)])                  # one ds_read_b64: [i][lane]
                fb = np.stack([sB[row, 32 * NJ * wc + NJ * li + j] for j in range(NJ)])           # one ds_read_b128 / b64: [j][lane]
                for i in range(2):
                    for j in range(NJ):
                        # C[i'][j'] += sum_k A[i'][k] B[j'][k], operand of (i', k) in lane i' + 32 k
                        Am = fa[i].reshape(2, 32)         # [k][i']
                        Bm = fb[j].reshape(2, 32)
                        C = Am[0][:, None] * Bm[0][None, :] + Am[1][:, None] * Bm[1][None, :]
                        acc[w, i, j] += C[rrow[None, :] + 4 * lh[:, None], li[:, None]]
    for w in range(nw):
        wr, wc = w >> 1, w & 1
        for i in range(2):
            for rr in range(16):
                for l in range(64):
                    row = 64 * wr + 2 * ((rr & 3) + 8 * (rr >> 2) + 4 * (l >> 5)) + i
                    col = 32 * NJ * wc + NJ * (l & 31)
                    slab[row, col: col + NJ] = acc[w, i, :, l, rr]
                    writes[row, col: col + NJ] += 1
    return slab, writes, pairs, touched


def present_pairs(P):
    """gemm_tn2_kernel: in k-group kk, step e, lanes 0-31 hold k = 8 kk + e of the chunk and lanes 32-63 k = 8 kk + 4 + e."""
    return [(kt * TBK + 8 * kk + e, kt * TBK + 8 * kk + 4 + e) for kt in range((P + TBK - 1) // TBK) for kk in range(4) for e in range(4)]


def test_256_tile_reproduces_the_product_every_output_once_in_the_present_order():
    rng = np.random.default_rng(0)
    P, N1, N2, lda, ldb = 70, 512, 256, 516, 260          # ragged third chunk, ld > N, second row tile of A
    A = rng.integers(-4, 5, size=P * lda).astype(np.float64)
    B = rng.integers(-4, 5, size=P * ldb).astype(np.float64)
    slab, writes, pairs, touched = model_tile(A, lda, B, ldb, P, N1, N2, 256, 0)
    ref = A.reshape(P, lda)[:, 256:512].T @ B.reshape(P, ldb)[:, :256]
    assert np.array_equal(slab, ref)
    assert (writes == 1).all()
    assert pairs == present_pairs(P)
    assert min(b for b, _ in touched) >= 0


def test_128_tile_reproduces_the_product_every_output_once_in_the_present_order():
    """A ragged tile: N1 = 217 (second row tile holds 89 real columns of A), N2 = 39; the real outputs are compared."""
    rng = np.random.default_rng(1)
    P, N1, N2, lda, ldb = 45, 217, 39, 220, 40
    A = rng.integers(-4, 5, size=P * lda).astype(np.float64)
    B = rng.integers(-4, 5, size=P * ldb).astype(np.float64)
    slab, writes, pairs, touched = model_tile(A, lda, B, ldb, P, N1, N2, 128, 0, T=128)
    ref = A.reshape(P, lda)[:, 128:217].T @ B.reshape(P, ldb)[:, :39]
    assert np.array_equal(slab[:89, :39], ref)
    assert (writes == 1).all()
    assert pairs == present_pairs(P)
    assert max(e for _, e in touched) <= P * max(lda, ldb) * 4


def test_load_addresses_stay_inside_the_operand():
    """Ragged P, N not a multiple of 4, ld > N, every tile origin: a lane's 16 bytes lie in [0, (P - 1) ld 4 + ld 4)."""
    for T in (256, 128):
        for P, N, ld in ((1, 256, 256), (33, 256, 352), (70, 217, 220), (5, 39, 40), (64, 257, 264), (31, 3, 4), (100, 512, 516), (9, 1, 8)):
            X = np.zeros(P * ld)
            for n0 in range(0, (N + T - 1) // T * T, T):
                for p_begin, p_end in ((0, P), (P // 2, P)):
                    touched = []
                    for kt in range((p_end - p_begin + TBK - 1) // TBK):
                        load_stage(X, ld, N, n0, p_begin, p_end, kt, touched, T)
                    assert touched
                    assert min(b for b, _ in touched) >= 0 and max(e for _, e in touched) <= (P - 1) * ld * 4 + ld * 4, (T, P, N, ld, n0)
                    # ... and never past the last real column's quad
                    assert max(b % (ld * 4) for b, _ in touched) <= (N - 1) // 4 * 16
