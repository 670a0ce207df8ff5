// wgrad_rm.hip -- exact-fp32 weight-gradient (TN) GEMM on 256 x 256 tiles with ROW-MAJOR operand stages (gfx950).
//
// Same contract, slab layout, split rule and -- element by element -- the same fmaf chains as gemm_tn2_kernel (gemm_tn.hip);
// what differs is the way the operands travel.  gemm_tn2_kernel transposes them on the way into LDS ([column][k]), which costs
// 32 four-byte loads per thread and 32-deep chunk, each with its own row clamp.  No transpose is needed to feed
// v_mfma_f32_32x32x2_f32 from a [point][column] image:
//
//   stage      [32 points][256 columns] per operand, no padding: 2 stages x 2 operands x 32 KB = 128 KB
//   loads      wave w fetches points 4 w .. 4 w + 3 of the chunk, lane l the quad of columns 4 l .. 4 l + 3: four 16-byte loads per
//              operand and chunk, wave-uniform row address, one ds_write_b128 each; the ragged tail is zeroed by whole rows
//   fragments  lane (li = lane & 31, lh = lane >> 5) supplies A[i = li][k = lh].  One ds_read_b64 at [point][64 wr + 2 li] is the
//              same-k operand of TWO 32-column tiles, one ds_read_b128 at [point][128 wc + 4 li] of FOUR: the tiles of a wave
//              are column-INTERLEAVED (A tile i owns columns 2 i' + i, B tile j columns 4 j' + j).  Per MFMA step (8 MFMAs over
//              the 64 x 128 wave tile) that is one b64 and one b128 read, each lane group on 256 contiguous bytes: no conflict.
//   order      step e of k-group kk consumes point kk 8 + e (lanes 0-31) and kk 8 + 4 + e (lanes 32-63), chunks in sequence,
//              pair 0 before pair 1: the pairs and the order of gemm_tn2_kernel, so every dW element keeps its bits
//   slab       for accumulator register r and A tile i a lane holds four consecutive n2: 32 sixteen-byte stores
//   bias sums  gemm_tn2_kernel's thread (column c, half kg) adds, per chunk, rs_i = (r0 + r1) + (r2 + r3) of its four 4-point
//              pieces i = 0..3 in sequence.  Piece i of half kg is what wave 4 kg + i fetched: the waves leave their rs in a
//              double-buffered [8][256] LDS array and the same owner adds them in the same order after the chunk's barrier.
//
// The operands must be 16-byte aligned (nu_wgrad_rm_ok); everything else keeps gemm_tn2_kernel.
#include <type_traits>

#include "gemm_epi.h"
#include "wgrad_rm.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// (an opaque scalar add: beside MFMAs the packed fp32 VALU forms the vectoriser would pick for these sums are expensive)
static __device__ __forceinline__ float rm_add(float a, float b) {
    float r;
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

static __device__ __forceinline__ void rm256_body(const NuGemmTN& g, const int bx, const int split, const int grp) {
    constexpr int T = 256;                           // tile edge
    __shared__ __attribute__((aligned(16))) float smem[2][2][TBK * T];        // [stage][A | B][point][column]
    __shared__ __attribute__((aligned(16))) float rsb[2][8][T];               // [chunk parity][piece = fetching wave][column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;           // wave tile: rows (N1) 64 wr .. +64, columns (N2) 128 wc .. +128
    const int t2 = g.N2 / T;
    const int n1t = bx / t2, n2t = bx - n1t * t2;
    const int n1_0 = n1t * T, n2_0 = n2t * T;
    const int N1p = g.N1, N2p = g.N2;                // multiples of 256: the slab extents of nu_wgrad_workspace_bytes

    int rows_per = (g.P + g.S - 1) / g.S;
    rows_per = ((rows_per + TBK - 1) / TBK) * TBK;
    const int p_begin = split * rows_per;
    int p_end = p_begin + rows_per;
    p_end = p_end < g.P ? p_end : g.P;
    const int ntile = p_end > p_begin ? (p_end - p_begin + TBK - 1) / TBK : 0;
    const int npair = g.A1 ? 2 : 1;
    const int total = ntile * npair;

    const int c = tid & (T - 1);    // bias sums: the column this thread owns ...
    const int kg = tid / T;         // ... and its half of the chunk (pieces 4 kg .. 4 kg + 3)
    const bool do_bias = (g.bias_slab != nullptr) && (n2t == 0);

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float bs = 0.f;

    if (total > 0) {
        f32x4 ra[4], rb[4];             // the chunk in registers: points 4 wid + e, this lane's quad
        int pend_pr0 = 0;               // ... its first point (wave-uniform) and whether it belongs to pair 0
        bool pend_pair0 = true;
        // loader state of the chunk being fetched (all wave-uniform but the quad offsets)
        const char* __restrict__ ldA = nullptr;
        const char* __restrict__ ldB = nullptr;
        unsigned ld_lda4 = 0, ld_ldb4 = 0, ld_qa = 0, ld_qb = 0;
        int ld_pr0 = 0;
        bool ld_pair0 = true;
        auto ld_begin = [&](int t) {
            const int pair = t >= ntile ? 1 : 0;
            const int kt = t - pair * ntile;
            ldA = (const char*)(pair ? g.A1 + (long long)grp * g.sA1 : g.A0 + (long long)grp * g.sA0);
            ldB = (const char*)(pair ? g.B1 + (long long)grp * g.sB1 : g.B0 + (long long)grp * g.sB0);
            const int lda = pair ? g.lda1 : g.lda0, ldb = pair ? g.ldb1 : g.ldb0;
            // quads past the operand (never with N a multiple of 256 inside its row; kept as the one guard against a bad ld) are
            // clamped to the last quad that holds a real column: a 16-byte load never leaves the row
            int qa = n1_0 / 4 + lane, qb = n2_0 / 4 + lane;
            const int qam = (g.N1 - 1) / 4 < lda / 4 - 1 ? (g.N1 - 1) / 4 : lda / 4 - 1;
            const int qbm = (g.N2 - 1) / 4 < ldb / 4 - 1 ? (g.N2 - 1) / 4 : ldb / 4 - 1;
            qa = qa < qam ? qa : qam;
            qb = qb < qbm ? qb : qbm;
            ld_qa = (unsigned)qa * 16u; ld_qb = (unsigned)qb * 16u;
            ld_lda4 = (unsigned)lda * 4u; ld_ldb4 = (unsigned)ldb * 4u;
            ld_pr0 = p_begin + kt * TBK + 4 * wid;
            ld_pair0 = pair == 0;
        };
        // one 16-byte load: point 4 wid + e of the chunk (the ragged tail re-reads the split's last row, zeroed at the hand-over);
        // operands are below 4 GiB, so the row's byte offset fits 32 bits
        auto ld_row = [&](bool isA, int e) {
            int pr = ld_pr0 + e;
            pr = pr < p_end ? pr : p_end - 1;
            if (isA) ra[e] = *reinterpret_cast<const f32x4*>(ldA + (size_t)((unsigned)pr * ld_lda4) + ld_qa);
            else rb[e] = *reinterpret_cast<const f32x4*>(ldB + (size_t)((unsigned)pr * ld_ldb4) + ld_qb);
        };
        auto ld_done = [&]() { pend_pr0 = ld_pr0; pend_pair0 = ld_pair0; };
        // hand-over of the chunk in registers: zero the rows past the split's end, bias pieces, 16-byte writes
        auto st_zero = [&](bool isA) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = pend_pr0 + e < p_end;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (isA) ra[e][q] = ok ? ra[e][q] : 0.f;
                    else rb[e][q] = ok ? rb[e][q] : 0.f;
                }
            }
        };
        auto st_rs = [&](int par) {
            f32x4 rs;
#pragma unroll
            for (int q = 0; q < 4; ++q) rs[q] = rm_add(rm_add(ra[0][q], ra[1][q]), rm_add(ra[2][q], ra[3][q]));
            *reinterpret_cast<f32x4*>(&rsb[par][wid][4 * lane]) = rs;
        };
        auto st_write = [&](bool isA, int st, int e) {
            if (isA) *reinterpret_cast<f32x4*>(&smem[st][0][(4 * wid + e) * T + 4 * lane]) = ra[e];
            else *reinterpret_cast<f32x4*>(&smem[st][1][(4 * wid + e) * T + 4 * lane]) = rb[e];
        };
        // the owner's turn: pieces 4 kg .. 4 kg + 3 of the chunk of parity `par`, in sequence (a select, not a branch)
        auto bias_add = [&](int par, bool on) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = rsb[par][4 * kg + i][c];
                bs += on ? v : 0.f;
            }
        };

        // two LDS stages: chunk t+1 waits in registers (fetched during chunk t-1), goes to the other stage under the first MFMAs of
        // chunk t, and the registers are re-issued for chunk t+2 at once: one barrier per chunk
        ld_begin(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ld_row(true, e); ld_row(false, e); }
        ld_done();
        st_zero(true); st_zero(false);
        st_rs(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { st_write(true, 0, e); st_write(false, 0, e); }
        ld_begin(total > 1 ? 1 : 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ld_row(true, e); ld_row(false, e); }
        ld_done();
        __syncthreads();
        bias_add(0, do_bias);

        const int li = lane & 31, lh = lane >> 5;
        const int a_off = 4 * lh * T + wr * 64 + 2 * li;
        const int b_off = 4 * lh * T + wc * 128 + 4 * li;
        struct FragT { f32x2 a; f32x4 b; };
        FragT F0, F1;
        F0.a = *reinterpret_cast<const f32x2*>(&smem[0][0][a_off]);
        F0.b = *reinterpret_cast<const f32x4*>(&smem[0][1][b_off]);
        int cur = 0;
        bool bias_on = false;
        // Fragments are double-buffered in registers and every memory instruction of a chunk sits alone between two MFMAs (see
        // gemm_tn2_kernel).  A chunk is 16 slots of 8 MFMAs (slot s = 4 kk + e reads points 8 kk + e and 8 kk + 4 + e); every slot
        // issues the two fragment reads of the next one in its first two gaps.  The other gaps:
        //   slots 0-3    chunk t+1, registers -> the other stage (zero the rows past the end, bias pieces, eight 16-byte writes), and
        //                every register quad re-issued for chunk t+2 as soon as it is written: one memory instruction per gap, all
        //                eight loads in flight twelve slots before the next chunk's hand-over needs them
        //   behind slot 14 the barrier; slot 15 reads the first fragments of chunk t+1 and the bias owner adds that chunk's pieces
#define RM_PIN __builtin_amdgcn_sched_barrier(0);
#define RM_M(F, i, j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a[i], F.b[j], acc[i][j], 0, 0, 0); RM_PIN
#define RM_SLOT(F, ...) RM_SLOT_(F, __VA_ARGS__)
#define RM_SLOT_(F, X0, X1, X2, X3, X4, X5, X6)                                                   \
    RM_M(F, 0, 0) X0; RM_PIN RM_M(F, 0, 1) X1; RM_PIN RM_M(F, 0, 2) X2; RM_PIN RM_M(F, 0, 3) X3; RM_PIN     \
    RM_M(F, 1, 0) X4; RM_PIN RM_M(F, 1, 1) X5; RM_PIN RM_M(F, 1, 2) X6; RM_PIN RM_M(F, 1, 3)
#define RM_RDA(F, ST, s) F.a = *reinterpret_cast<const f32x2*>(&smem[ST][0][a_off + (((s) >> 2) * 8 + ((s) & 3)) * T])
#define RM_RDB(F, ST, s) F.b = *reinterpret_cast<const f32x4*>(&smem[ST][1][b_off + (((s) >> 2) * 8 + ((s) & 3)) * T])
#define RM_RD(F, ST, s) RM_RDA(F, ST, s), RM_RDB(F, ST, s)
        // No instruction of the loop body is conditional (a branch around a load makes the compiler wait for every load in flight at
        // the join).  Past the end of the split the loader re-reads the last chunk (valid addresses, data never used) and the
        // hand-over writes a stage nobody reads again; only the bias sum must not see those chunks (a select).
        for (int t = 0; t < total; ++t) {
            bias_on = do_bias && pend_pair0 && t + 1 < total;
            RM_SLOT(F0, RM_RD(F1, cur, 1), st_zero(true), st_rs(cur ^ 1), ld_begin(t + 2 < total ? t + 2 : total - 1), st_write(true, cur ^ 1, 0), st_write(true, cur ^ 1, 1))
            RM_SLOT(F1, RM_RD(F0, cur, 2), st_write(true, cur ^ 1, 2), st_write(true, cur ^ 1, 3), ld_row(true, 0), ld_row(true, 1), st_zero(false))
            RM_SLOT(F0, RM_RD(F1, cur, 3), ld_row(true, 2), ld_row(true, 3), st_write(false, cur ^ 1, 0), st_write(false, cur ^ 1, 1), st_write(false, cur ^ 1, 2))
            RM_SLOT(F1, RM_RD(F0, cur, 4), st_write(false, cur ^ 1, 3), ld_row(false, 0), ld_row(false, 1), ld_row(false, 2), ld_row(false, 3))
            RM_SLOT(F0, RM_RD(F1, cur, 5), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F1, RM_RD(F0, cur, 6), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F0, RM_RD(F1, cur, 7), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F1, RM_RD(F0, cur, 8), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F0, RM_RD(F1, cur, 9), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F1, RM_RD(F0, cur, 10), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F0, RM_RD(F1, cur, 11), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F1, RM_RD(F0, cur, 12), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F0, RM_RD(F1, cur, 13), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F1, RM_RD(F0, cur, 14), (void)0, (void)0, (void)0, (void)0, (void)0)
            RM_SLOT(F0, RM_RD(F1, cur, 15), (void)0, (void)0, (void)0, (void)0, (void)0)
            __syncthreads();            // the other stage is complete; every wave holds its last fragments of this one
            RM_SLOT(F1, RM_RD(F0, cur ^ 1, 0), bias_add(cur ^ 1, bias_on), (void)0, (void)0, (void)0, (void)0)   // (after the last chunk: stale bytes, never used)
            ld_done();
            cur ^= 1;
        }
#undef RM_PIN
#undef RM_M
#undef RM_SLOT
#undef RM_SLOT_
#undef RM_RDA
#undef RM_RDB
#undef RM_RD
    }

    // accumulator register r of tile (i, j): row 2 ((r & 3) + 8 (r >> 2) + 4 lh) + i of the wave's 64, column 4 li + j of its 128
    const int li = lane & 31, lh = lane >> 5;
    float* __restrict__ slab = g.slab + (long long)grp * g.sSlab + (long long)split * N1p * N2p;
    const int col = n2_0 + wc * 128 + 4 * li;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = n1_0 + wr * 64 + 2 * ((r & 3) + 8 * (r >> 2) + 4 * lh) + i;
            f32x4 v;
            v[0] = acc[i][0][r]; v[1] = acc[i][1][r]; v[2] = acc[i][2][r]; v[3] = acc[i][3][r];
            *reinterpret_cast<f32x4*>(&slab[(long long)row * N2p + col]) = v;
        }
    if (do_bias) {
        __syncthreads();
        float* red = &smem[0][0][0];
        red[kg * T + c] = bs;
        __syncthreads();
        if (tid < T) g.bias_slab[(long long)grp * g.sBiasSlab + (long long)split * N1p + n1_0 + tid] = red[tid] + red[T + tid];
    }
}

__global__ __launch_bounds__(512, 2) void wgrad_rm256_kernel(NuGemmTN g) { rm256_body(g, blockIdx.x, blockIdx.y, blockIdx.z); }
__global__ __launch_bounds__(512, 2) void wgrad_rm256b_kernel(NuGemmTNBatch b) {
    int bx, split;
    const int pi = tn_batch_decode(b, 256, bx, split);
    rm256_body(b.p[pi], bx, split, 0);
}

// ------------------------------------------------------------------------------------------------
// The same mapping on a 128 x 128 tile (256 threads, 4 waves as 2 x 2, wave tile 64 x 64 = 2 x 2 MFMA tiles) for the shapes the
// 256-tile rule rejects (1024 x 288, 256 x 352, 257 x 256, ...).  Two ds_read_b64 per MFMA step of 4; stages 2 x 2 x 16 KB.
// A wave load covers TWO rows (32 quads each): lane half h = lane >> 5 fetches points 8 w + 4 h + e, so that the four rows of
// bias piece 2 w + h (gemm_tn_kernel's thread (c, kg) owns pieces 4 kg .. 4 kg + 3) meet in one lane.  The tiles of a wave are
// column-interleaved, so the padding of a ragged N1 / N2 is skipped by whole waves (64 columns), not by 32 x 32 blocks: a wave
// with no real output keeps loading, handing over and meeting the barriers, and issues no MFMA.
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ void rm128_body(const NuGemmTN& g, const int bx, const int split, const int grp) {
    constexpr int T = 128;
    __shared__ __attribute__((aligned(16))) float smem[2][2][TBK * T];        // [stage][A | B][point][column]
    __shared__ __attribute__((aligned(16))) float rsb[2][8][T];               // [chunk parity][piece][column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int t2 = (g.N2 + T - 1) / T;
    const int n1t = bx / t2, n2t = bx - n1t * t2;
    const int n1_0 = n1t * T, n2_0 = n2t * T;
    const int N1p = ((g.N1 + 127) / 128) * 128, N2p = t2 * 128;

    int rows_per = (g.P + g.S - 1) / g.S;
    rows_per = ((rows_per + TBK - 1) / TBK) * TBK;
    const int p_begin = split * rows_per;
    int p_end = p_begin + rows_per;
    p_end = p_end < g.P ? p_end : g.P;
    const int ntile = p_end > p_begin ? (p_end - p_begin + TBK - 1) / TBK : 0;
    const int npair = g.A1 ? 2 : 1;
    const int total = ntile * npair;

    const int c = tid & (T - 1);    // bias sums: the column this thread owns and its half of the chunk
    const int kg = tid / T;
    const bool do_bias = (g.bias_slab != nullptr) && (n2t == 0);
    const bool live = (n1_0 + wr * 64 < g.N1) && (n2_0 + wc * 64 < g.N2);      // wave-uniform

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float bs = 0.f;
    const int li = lane & 31, lh = lane >> 5;

    if (total > 0) {
        f32x4 ra[4], rb[4];             // the chunk in registers: points 8 wid + 4 lh + e, quad li
        int pend_pr = 0;                // ... this lane's first point, and whether the chunk belongs to pair 0
        bool pend_pair0 = true;
        const char* __restrict__ ldA = nullptr;
        const char* __restrict__ ldB = nullptr;
        unsigned ld_lda4 = 0, ld_ldb4 = 0, ld_qa = 0, ld_qb = 0;
        int ld_pr = 0;
        bool ld_pair0 = true;
        auto ld_begin = [&](int t) {
            const int pair = t >= ntile ? 1 : 0;
            const int kt = t - pair * ntile;
            ldA = (const char*)(pair ? g.A1 + (long long)grp * g.sA1 : g.A0 + (long long)grp * g.sA0);
            ldB = (const char*)(pair ? g.B1 + (long long)grp * g.sB1 : g.B0 + (long long)grp * g.sB0);
            const int lda = pair ? g.lda1 : g.lda0, ldb = pair ? g.ldb1 : g.ldb0;
            // quads past the operand are clamped to the last quad that holds a real column: a 16-byte load never leaves the row, and
            // what it brings only reaches slab entries the reduction never reads
            int qa = n1_0 / 4 + li, qb = n2_0 / 4 + li;
            const int qam = (g.N1 - 1) / 4 < lda / 4 - 1 ? (g.N1 - 1) / 4 : lda / 4 - 1;
            const int qbm = (g.N2 - 1) / 4 < ldb / 4 - 1 ? (g.N2 - 1) / 4 : ldb / 4 - 1;
            qa = qa < qam ? qa : qam;
            qb = qb < qbm ? qb : qbm;
            ld_qa = (unsigned)qa * 16u; ld_qb = (unsigned)qb * 16u;
            ld_lda4 = (unsigned)lda * 4u; ld_ldb4 = (unsigned)ldb * 4u;
            ld_pr = p_begin + kt * TBK + 8 * wid + 4 * lh;
            ld_pair0 = pair == 0;
        };
        auto ld_row = [&](bool isA, int e) {
            int pr = ld_pr + e;
            pr = pr < p_end ? pr : p_end - 1;
            if (isA) ra[e] = *reinterpret_cast<const f32x4*>(ldA + (size_t)((unsigned)pr * ld_lda4 + ld_qa));
            else rb[e] = *reinterpret_cast<const f32x4*>(ldB + (size_t)((unsigned)pr * ld_ldb4 + ld_qb));
        };
        auto ld_done = [&]() { pend_pr = ld_pr; pend_pair0 = ld_pair0; };
        auto st_zero = [&](bool isA) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = pend_pr + e < p_end;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (isA) ra[e][q] = ok ? ra[e][q] : 0.f;
                    else rb[e][q] = ok ? rb[e][q] : 0.f;
                }
            }
        };
        auto st_rs = [&](int par) {
            f32x4 rs;
#pragma unroll
            for (int q = 0; q < 4; ++q) rs[q] = rm_add(rm_add(ra[0][q], ra[1][q]), rm_add(ra[2][q], ra[3][q]));
            *reinterpret_cast<f32x4*>(&rsb[par][2 * wid + lh][4 * li]) = rs;
        };
        auto st_write = [&](bool isA, int st, int e) {
            if (isA) *reinterpret_cast<f32x4*>(&smem[st][0][(8 * wid + 4 * lh + e) * T + 4 * li]) = ra[e];
            else *reinterpret_cast<f32x4*>(&smem[st][1][(8 * wid + 4 * lh + e) * T + 4 * li]) = rb[e];
        };
        auto bias_add = [&](int par, bool on) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = rsb[par][4 * kg + i][c];
                bs += on ? v : 0.f;
            }
        };

        ld_begin(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ld_row(true, e); ld_row(false, e); }
        ld_done();
        st_zero(true); st_zero(false);
        st_rs(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { st_write(true, 0, e); st_write(false, 0, e); }
        ld_begin(total > 1 ? 1 : 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ld_row(true, e); ld_row(false, e); }
        ld_done();
        __syncthreads();
        bias_add(0, do_bias);

        const int a_off = 4 * lh * T + wr * 64 + 2 * li;
        const int b_off = 4 * lh * T + wc * 64 + 2 * li;
        struct FragT { f32x2 a; f32x2 b; };
        FragT F0, F1;
        F0.a = *reinterpret_cast<const f32x2*>(&smem[0][0][a_off]);
        F0.b = *reinterpret_cast<const f32x2*>(&smem[0][1][b_off]);
        F1 = F0;
        int cur = 0;
        bool bias_on = false;
        // A chunk is 16 slots of 4 MFMAs; a slot issues the two fragment reads of the next one behind its first two MFMAs and has two
        // more gaps: slots 0-9 carry the hand-over of chunk t+1 and the re-issue of its registers for chunk t+2 (A first, then B), the
        // barrier sits behind slot 14, slot 15 reads the first fragments of chunk t+1 and adds its bias pieces.  LIVE = false is the
        // same sequence without fragments and MFMAs (a wave whose 64 x 64 outputs are all padding).
#define RM_PIN __builtin_amdgcn_sched_barrier(0);
#define RM_M(F, i, j) if constexpr (LIVE) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a[i], F.b[j], acc[i][j], 0, 0, 0); RM_PIN
#define RM_SLOT(F, ...) RM_SLOT_(F, __VA_ARGS__)      /* (one more level: RM_RD expands to two arguments first) */
#define RM_SLOT_(F, R0, R1, X2, X3) RM_M(F, 0, 0) if constexpr (LIVE) { R0; } RM_PIN RM_M(F, 0, 1) if constexpr (LIVE) { R1; } RM_PIN RM_M(F, 1, 0) X2; RM_PIN RM_M(F, 1, 1) X3; RM_PIN
#define RM_RDA(F, ST, s) F.a = *reinterpret_cast<const f32x2*>(&smem[ST][0][a_off + (((s) >> 2) * 8 + ((s) & 3)) * T])
#define RM_RDB(F, ST, s) F.b = *reinterpret_cast<const f32x2*>(&smem[ST][1][b_off + (((s) >> 2) * 8 + ((s) & 3)) * T])
#define RM_RD(F, ST, s) RM_RDA(F, ST, s), RM_RDB(F, ST, s)
        auto chunks = [&](auto live_c) {
            constexpr bool LIVE = decltype(live_c)::value;
            for (int t = 0; t < total; ++t) {
                bias_on = do_bias && pend_pair0 && t + 1 < total;
                RM_SLOT(F0, RM_RD(F1, cur, 1), st_zero(true), st_rs(cur ^ 1))
                RM_SLOT(F1, RM_RD(F0, cur, 2), ld_begin(t + 2 < total ? t + 2 : total - 1), st_write(true, cur ^ 1, 0))
                RM_SLOT(F0, RM_RD(F1, cur, 3), st_write(true, cur ^ 1, 1), st_write(true, cur ^ 1, 2))
                RM_SLOT(F1, RM_RD(F0, cur, 4), st_write(true, cur ^ 1, 3), ld_row(true, 0))
                RM_SLOT(F0, RM_RD(F1, cur, 5), ld_row(true, 1), ld_row(true, 2))
                RM_SLOT(F1, RM_RD(F0, cur, 6), ld_row(true, 3), st_zero(false))
                RM_SLOT(F0, RM_RD(F1, cur, 7), st_write(false, cur ^ 1, 0), st_write(false, cur ^ 1, 1))
                RM_SLOT(F1, RM_RD(F0, cur, 8), st_write(false, cur ^ 1, 2), st_write(false, cur ^ 1, 3))
                RM_SLOT(F0, RM_RD(F1, cur, 9), ld_row(false, 0), ld_row(false, 1))
                RM_SLOT(F1, RM_RD(F0, cur, 10), ld_row(false, 2), ld_row(false, 3))
                RM_SLOT(F0, RM_RD(F1, cur, 11), (void)0, (void)0)
                RM_SLOT(F1, RM_RD(F0, cur, 12), (void)0, (void)0)
                RM_SLOT(F0, RM_RD(F1, cur, 13), (void)0, (void)0)
                RM_SLOT(F1, RM_RD(F0, cur, 14), (void)0, (void)0)
                RM_SLOT(F0, RM_RD(F1, cur, 15), (void)0, (void)0)
                __syncthreads();            // the other stage is complete; every wave holds its last fragments of this one
                RM_SLOT(F1, RM_RD(F0, cur ^ 1, 0), bias_add(cur ^ 1, bias_on), (void)0)
                ld_done();
                cur ^= 1;
            }
        };
        if (live) chunks(std::true_type{});
        else chunks(std::false_type{});
#undef RM_PIN
#undef RM_M
#undef RM_SLOT
#undef RM_SLOT_
#undef RM_RDA
#undef RM_RDB
#undef RM_RD
    }

    // accumulator register r of tile (i, j): row 2 ((r & 3) + 8 (r >> 2) + 4 lh) + i of the wave's 64, column 2 li + j of its 64
    if (live) {
        float* __restrict__ slab = g.slab + (long long)grp * g.sSlab + (long long)split * N1p * N2p;
        const int col = n2_0 + wc * 64 + 2 * li;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = n1_0 + wr * 64 + 2 * ((r & 3) + 8 * (r >> 2) + 4 * lh) + i;
                f32x2 v;
                v[0] = acc[i][0][r]; v[1] = acc[i][1][r];
                *reinterpret_cast<f32x2*>(&slab[(long long)row * N2p + col]) = v;
            }
    }
    if (do_bias) {
        __syncthreads();
        float* red = &smem[0][0][0];
        red[kg * T + c] = bs;
        __syncthreads();
        if (tid < T) g.bias_slab[(long long)grp * g.sBiasSlab + (long long)split * N1p + n1_0 + tid] = red[tid] + red[T + tid];
    }
}

__global__ __launch_bounds__(256, 2) void wgrad_rm128_kernel(NuGemmTN g) { rm128_body(g, blockIdx.x, blockIdx.y, blockIdx.z); }
__global__ __launch_bounds__(256, 2) void wgrad_rm128b_kernel(NuGemmTNBatch b) {
    int bx, split;
    const int pi = tn_batch_decode(b, 128, bx, split);
    rm128_body(b.p[pi], bx, split, 0);
}

bool nu_wgrad_rm_ok(const NuGemmTN& g) {
    if ((g.bf16 & 3) != 0 || (g.bf16 & ~3) != 0) return false;
    const int groups = g.groups > 0 ? g.groups : 1;
    auto ok = [&](const float* p, int ld, long long s, int n) {
        if (p == nullptr) return true;
        if ((((uintptr_t)p) & 15) != 0 || (ld & 3) != 0 || ld < n) return false;
        if (groups > 1 && (s & 3) != 0) return false;
        return (long long)g.P * ld * 4 < (1LL << 32);
    };
    if (g.A1 != nullptr && g.B1 == nullptr) return false;
    return ok(g.A0, g.lda0, g.sA0, g.N1) && ok(g.B0, g.ldb0, g.sB0, g.N2) && ok(g.A1, g.lda1, g.sA1, g.N1) && ok(g.B1, g.ldb1, g.sB1, g.N2);
}

int nu_wgrad_rm256_launch(const NuGemmTN& g, hipStream_t stream) {
    if ((g.N1 % 256) != 0 || (g.N2 % 256) != 0 || !nu_wgrad_rm_ok(g)) return NU_ERR_ARG;
    dim3 grid((g.N1 / 256) * (g.N2 / 256), g.S, g.groups > 0 ? g.groups : 1);
    hipLaunchKernelGGL(wgrad_rm256_kernel, grid, dim3(512), 0, stream, g);
    return nu_launch_status();
}

int nu_wgrad_rm256_launch_batch(const NuGemmTNBatch& b, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL(wgrad_rm256b_kernel, dim3(blocks), dim3(512), 0, stream, b);
    return nu_launch_status();
}

int nu_wgrad_rm128_launch(const NuGemmTN& g, hipStream_t stream) {
    if (!nu_wgrad_rm_ok(g)) return NU_ERR_ARG;
    dim3 grid(nu_cdiv(g.N1, 128) * nu_cdiv(g.N2, 128), g.S, g.groups > 0 ? g.groups : 1);
    hipLaunchKernelGGL(wgrad_rm128_kernel, grid, dim3(256), 0, stream, g);
    return nu_launch_status();
}

int nu_wgrad_rm128_launch_batch(const NuGemmTNBatch& b, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL(wgrad_rm128b_kernel, dim3(blocks), dim3(256), 0, stream, b);
    return nu_launch_status();
}
