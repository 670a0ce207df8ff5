// background.hip -- the learned NeRF++ background of a set of rays as ONE no-gradient kernel: (o, d, z nodes, t_stop) -> the outer
// (|x| > 1) samples through outer_nerf -> density / colour activation -> the front-to-back composite with every inner alpha zero.
//
// Reference: color_bkgr of render_core (network/renderer_zerothick.py:757, :777-779) over compute_density_alpha (:687-693) and NeRF
// (network/field.py:265-289).  The training step computes it through the layered path -- nu_partition_* (point records, one host read
// of P_in), nu_nerf_embed + ten NT GEMMs + two skinny heads + nu_nerf_act_fwd (about 11 KB of workspace per outer row), then
// nu_composite_fwd -- which a frame's tens of millions of outer rows cannot go through without chunking and host reads.  The arithmetic
// per ray and sample is stated at nu_background_fwd in include/nu_nerf.h; every row carries the bits of the layered path (same point
// arithmetic as partition_write_kernel, same embedding as nerf_embed_kernel, same MFMA and k order per accumulator as nu_gemm_nt, the
// head reductions of skinny_fwd_kernel<1, 256> and <3, 128>, the expressions of nerf_act_fwd_kernel).
//
// Design: the pipeline of csrc/fused_mlp.h (activation tile in LDS as the A operand of every layer, weights streamed through two LDS
// stages behind ONE cursor that crosses all ten layer boundaries), 32 rows per workgroup (TMN = 1).  A workgroup takes one ray at a
// time (statically assigned, grid-stride over persistent workgroups, no atomics) in tiles of 32 consecutive samples.  ONE activation
// tile of row stride 356 floats (= 4 mod 32: no ds_read_b128 bank conflict, as in fused_mlp.h) holds in turn
//   columns 0 .. 255   the hidden activations (and the output of feature_linear),
//   columns 256 .. 351 the 96 input columns E4 -- written once per tile, read in place by layer 0 (K = 96, A fragments at column 256)
//                      and by layer 5 as the skip input U5 = [h (256) | E4 (96)] (K = 352); the epilogues in between write below 256,
//   columns 256 .. 287 afterwards the 32 view columns: the view layer reads [feat (256) | view (32)] (K = 288).
// The view embedding is the ray's (the view direction is -du for all its samples) and waits in a 32-float LDS record.  Per tile: one
// wave per row forms the sample point, its live flag and its input row; a tile with no live row skips its network behind a uniform
// branch (on a pixel that hits the surface two of three tiles go this way) but still contributes the factors fl(1 + 1e-7) of its
// samples to the transmittance.  Rows that are not live get zero input columns (finite everywhere in the network) and alpha = 0.
// Heads: one wave per row (sigma, 256 wide), two rows per wave (rgb, 128 wide).  Composite: in sample order, one sample after the
// other -- every thread runs the same 32 steps on the tile's record, so nothing is reduced across lanes and a ray's result depends on
// nothing but the ray.
//
// What is this file's own and not the header's, and why:
//   * BgStream / bg_layer restate FmStream / fm_layer<1>.  The view layer has N = 128 and its packed table has 128 rows; FmStream loads
//     256 rows per chunk and would read 147 KB past the table.  BgStream keeps a second row offset: the upper four of a thread's eight
//     row loads step back by 128 rows on a 128-row layer (branch-free, an offset of 0 on the 256-row layers), so stage rows 128 .. 255
//     receive a copy of rows 0 .. 127 -- finite weights whose products waves 2 and 3 discard (9 of the 79 chunks do half-useful work).
//     fm_layer takes an FmStream by type, so the loop is restated with it; with the loop in this file the A fragments are declared
//     16-byte aligned (every offset is a multiple of four floats) although the tile offset is a per-layer value.
//   * the rgb head is 128 wide, fm_row_dot is 256 wide.
// The header itself is untouched: the sibling kernels' code does not move.
//
// LDS: 32 x 356 x 4 + 16 = 45 584 (tile) + 1 024 (sample record) + 128 (view) + 73 728 (weight stages) = 120 464 B of the CU's
// 163 840: one workgroup per CU.  A 64-row tile does NOT fit: 64 rows at stride 356 are 91 136 B and with the 73 728 B of weight
// stages 164 864 B; a 260-stride tile (66 576 B) with a separate 64 x 100 E4 region (25 600 B) and the stages comes to 165 904 B.
#include "fused_mlp.h"

#define BG_ALD 356                 // activation row stride (floats): 352 columns + 4
#define BG_E4 256                  // first input column of the tile
#define BG_NL 10                   // streamed layers: pts_linears 0..7, feature_linear, views_linears.0
#define BG_RD 8                    // sample record per row: dist, live, sig, rgb x 3 (raw heads), unused x 2
#define BG_TM 32

struct BgNet {                     // kernel-argument block
    const float* Wp[BG_NL]; const float* bias[BG_NL];
    int Kp[BG_NL], half[BG_NL];    // half: the layer has 128 output rows (the view layer)
    const float *Wsig, *bsig, *Wrgb, *brgb;
    const float *O, *D, *z, *t_stop;
    int o_ld, d_ld, S, R;
    float *color, *trans, *enc, *raw, *act;
};

// The argument block again, behind a pointer the optimiser cannot see through (as in surface_shade.hip): fields read through it are
// loaded from the kernel-argument segment where they are used instead of being held in SGPRs across the main loop.
typedef const __attribute__((address_space(4))) BgNet* BgArgs;
#define BG_ARGS(q) BgArgs q = (BgArgs)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(q))      /* `net` is the first argument */

// FmStream of fused_mlp.h with the upper row loads of a 128-row layer folded back onto its lower rows (see the file header)
struct BgStream {
    int ld_l, ld_kt;
    const float* bp;               // this thread's slot of row r0 of the chunk at the cursor
    long long bstep, bhi;          // 32 rows further; added to row loads 4 .. 7: 0, or -128 rows on a 128-row layer
    f32x4 rb4[8];
    int cur;

    __device__ __forceinline__ void set_cursor(const BgNet& net, const FmThread& T) {
        bp = net.Wp[ld_l] + (long long)T.r0 * net.Kp[ld_l] + 4 * T.c4 + ld_kt * 32;
        bstep = 32LL * net.Kp[ld_l];
        bhi = -128LL * net.half[ld_l] * net.Kp[ld_l];
    }
    __device__ __forceinline__ void advance(const BgNet& net, const FmThread& T) {
        const bool wrap = ld_kt + 1 == net.Kp[ld_l] / 32, last = ld_l == BG_NL - 1;
        ld_kt = wrap ? (last ? ld_kt : 0) : ld_kt + 1;
        ld_l += wrap && !last;
        set_cursor(net, T);
    }
    __device__ __forceinline__ const float* row(int i) const { return bp + i * bstep + (i >= 4 ? bhi : 0LL); }
    __device__ __forceinline__ void load() {
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(row(i));
    }
    __device__ __forceinline__ void prologue(const BgNet& net, float* bst, const FmThread& T) {
        ld_l = 0; ld_kt = 0;
        set_cursor(net, T);
        load();
        advance(net, T);
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(&bst[T.w_off + 32 * i * FM_BLD]) = rb4[i];
        load();
        advance(net, T);
        __syncthreads();
        cur = 0;
    }
};

struct BgFrag { f32x4 a0, b0, b1; };

// fm_layer<1> of fused_mlp.h over a BgStream: the same schedule, one memory instruction per MFMA gap
static __device__ __forceinline__ void bg_layer(f32x16 (&acc)[2], BgStream& S, const BgNet& net, int nk, const float* tile, int a0_off,
                                                float* bst, BgFrag& F0, const FmThread& T) {
    BgFrag F1;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    F0.a0 = *reinterpret_cast<const f32x4*>(&tile[a0_off]);
#define BG_PIN __builtin_amdgcn_sched_barrier(0);
#define BG_M(F, e, j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a0[e], F.b##j[e], acc[j], 0, 0, 0); BG_PIN
#define BG_RA(F, k0, kk) F.a0 = *reinterpret_cast<const f32x4*>(&tile[a0_off + (k0) + (kk) * 8]); BG_PIN
#define BG_RB(F, St, kk, m) F.m = *reinterpret_cast<const f32x4*>(&(St)[T.m##_off + (kk) * 8]); BG_PIN
#define BG_W(i) *reinterpret_cast<f32x4*>(&so[T.w_off + 32 * (i) * FM_BLD]) = S.rb4[i]; BG_PIN
#define BG_L(i) S.rb4[i] = *reinterpret_cast<const f32x4*>(S.row(i)); BG_PIN
    const float* sc = &bst[S.cur * FM_BSTAGE];
    for (int kt = 0; kt < nk; ++kt) {
        float* so = &bst[(S.cur ^ 1) * FM_BSTAGE];
        const int k0 = kt * 32;
        // k-group 0: fragment reads of k-group 1
        BG_M(F0, 0, 0) BG_M(F0, 0, 1) BG_RA(F1, k0, 1)
        BG_M(F0, 1, 0) BG_M(F0, 1, 1)
        BG_M(F0, 2, 0) BG_M(F0, 2, 1) BG_RB(F1, sc, 1, b0)
        BG_M(F0, 3, 0) BG_M(F0, 3, 1) BG_RB(F1, sc, 1, b1)
        // k-group 1: the next weight chunk registers -> other stage; fragment reads of k-group 2
        BG_M(F1, 0, 0) BG_W(0) BG_M(F1, 0, 1) BG_RA(F0, k0, 2) BG_W(1)
        BG_M(F1, 1, 0) BG_W(2) BG_M(F1, 1, 1) BG_W(3)
        BG_M(F1, 2, 0) BG_W(4) BG_M(F1, 2, 1) BG_RB(F0, sc, 2, b0) BG_W(5)
        BG_M(F1, 3, 0) BG_W(6) BG_M(F1, 3, 1) BG_RB(F0, sc, 2, b1) BG_W(7)
        // k-group 2: the chunk after that global -> registers; fragment reads of k-group 3
        BG_M(F0, 0, 0) BG_L(0) BG_M(F0, 0, 1) BG_RA(F1, k0, 3) BG_L(1)
        BG_M(F0, 1, 0) BG_L(2) BG_M(F0, 1, 1) BG_L(3)
        BG_M(F0, 2, 0) BG_L(4) BG_M(F0, 2, 1) BG_RB(F1, sc, 3, b0) BG_L(5)
        BG_M(F0, 3, 0) BG_L(6) BG_M(F0, 3, 1) BG_RB(F1, sc, 3, b1) BG_L(7)
        S.advance(net, T);
        __syncthreads();        // the other stage is complete; every wave holds its last fragments of this chunk
        // k-group 3: first fragments of the next chunk (weights: the other stage, also across a layer boundary).  The A read is
        // unconditional and after a layer's last chunk returns bytes nobody uses, from the FM_APAD floats behind the tile at most
        BG_M(F1, 0, 0) BG_M(F1, 0, 1) BG_RA(F0, k0 + 32, 0)
        BG_M(F1, 1, 0) BG_M(F1, 1, 1)
        BG_M(F1, 2, 0) BG_M(F1, 2, 1) BG_RB(F0, so, 0, b0)
        BG_M(F1, 3, 0) BG_M(F1, 3, 1) BG_RB(F0, so, 0, b1)
        S.cur ^= 1;
        sc = so;
    }
#undef BG_M
#undef BG_RA
#undef BG_RB
#undef BG_W
#undef BG_L
#undef BG_PIN
}

// |x| of partition_write_kernel (nu_norm3 of csrc/render.hip)
static __device__ inline float bg_norm3(const float* x) {
#pragma clang fp contract(off)
    return sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
}
// nu_sample_point of csrc/render.hip (contraction off: the inner / outer decision rounds like eager ops), also returning the mid-point
static __device__ inline void bg_sample_point(const float* __restrict__ zrow, int S, int j, const float* o, const float* d, float* x,
                                              float& dist, float& mid) {
#pragma clang fp contract(off)
    const float z0 = zrow[j];
    if (j + 1 < S) dist = zrow[j + 1] - z0;
    else dist = S >= 2 ? zrow[S - 1] - zrow[S - 2] : 0.f;
    mid = z0 + dist * 0.5f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = d[c] * mid;
        x[c] = o[c] + m;
    }
}
// a . a as the gfx950 code of partition_write_kernel and nerf_embed_kernel forms it: a2 a2 + fma(a1, a1, a0 a0), not fused at the top
// (contraction is the compiler's choice per kernel; the encoded rows carry those kernels' bits only if these sums round as there)
static __device__ inline float bg_dot3(const float* a) {
#pragma clang fp contract(off)
    return a[2] * a[2] + __builtin_fmaf(a[1], a[1], a[0] * a[0]);
}
static __device__ inline float bg_softplus1(float x) { return x > 20.f ? x : log1pf(expf(x)); }
// nu_embed_col(x, D, col) of ide.h with the coordinate picked by selects (an array indexed by the lane would live in private memory)
template <int D>
static __device__ inline float bg_embed_col(const float (&x)[4], int col) {
    const int q = col < D ? 0 : col - D;
    const int k = q / (2 * D);
    const int r = q - k * 2 * D;
    const int c = col < D ? col : (r >= D ? r - D : r);
    const float xc = c == 0 ? x[0] : (c == 1 ? x[1] : (c == 2 ? x[2] : x[3]));
    if (col < D) return xc;
    const float a = xc * (float)(1 << k);
    return r >= D ? cosf(a) : sinf(a);
}

__global__ __launch_bounds__(256, 1) void background_fwd_kernel(BgNet net) {
    __shared__ __attribute__((aligned(16))) float tl[BG_TM * BG_ALD + FM_APAD];
    __shared__ __attribute__((aligned(16))) float rec[BG_TM * BG_RD];
    __shared__ __attribute__((aligned(16))) float vw[32];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int S = net.S, R = net.R;
    BgStream St;
    BgFrag F0;

    for (int ray = blockIdx.x; ray < R; ray += gridDim.x) {
        // ---- the ray: origin, direction, unit direction (partition_write_kernel), view embedding (nerf_embed_kernel) ----
        BG_ARGS(qr);
        const float* op = qr->O + (long long)ray * qr->o_ld;
        const float* dp = qr->D + (long long)ray * qr->d_ld;
        const float o[3] = {op[0], op[1], op[2]}, d[3] = {dp[0], dp[1], dp[2]};
        const float dn = fmaxf(sqrtf(bg_dot3(d)), 1e-12f);
        const float vd[4] = {-(d[0] / dn), -(d[1] / dn), -(d[2] / dn), 0.f};
        if (tid < 32) vw[tid] = tid < 27 ? bg_embed_col<3>(vd, tid) : 0.f;
        const float* zrow = qr->z + (long long)ray * S;
        const bool has_stop = qr->t_stop != nullptr;
        const float ts = has_stop ? qr->t_stop[ray] : 0.f;
        float Tr = 1.0f, col[3] = {0.f, 0.f, 0.f};              // the composite so far: every thread carries the same values

        for (int j0 = 0; j0 < S; j0 += BG_TM) {
            // ---- sample points, live flags and input rows: one wave per row, every lane the point's arithmetic ----
            for (int r = wc; r < BG_TM; r += 4) {
                const int j = j0 + r;
                float x[3] = {0.f, 0.f, 0.f}, dist = 0.f, mid = 0.f;
                bool live = false;
                if (j < S) {
                    bg_sample_point(zrow, S, j, o, d, x, dist, mid);
                    live = !(bg_norm3(x) <= 1.0f) && (!has_stop || mid < ts);
                }
                float* row = &tl[r * BG_ALD + BG_E4];
                if (live) {
                    const float nn = sqrtf(bg_dot3(x));
                    const float xe[4] = {x[0] / nn, x[1] / nn, x[2] / nn, 1.0f / nn};
                    for (int c = lane; c < 96; c += 64) row[c] = c < 84 ? bg_embed_col<4>(xe, c) : 0.f;
                } else {
                    for (int c = lane; c < 96; c += 64) row[c] = 0.f;
                }
                if (lane < BG_RD) rec[r * BG_RD + lane] = lane == 0 ? dist : (lane == 1 && live ? 1.0f : 0.f);
            }
            __syncthreads();
            const bool any_live = __ballot(rec[li * BG_RD + 1] != 0.f) != 0ull;     // every wave reads all 32 flags: uniform
            BG_ARGS(q);
            if (q->enc != nullptr) {            // test output: the rows as the network reads them (zeros where not live)
                for (int idx = tid; idx < BG_TM * 128; idx += 256) {
                    const int r = idx >> 7, c = idx & 127;
                    if (j0 + r >= S) break;
                    const bool lv = rec[r * BG_RD + 1] != 0.f;
                    q->enc[((long long)ray * S + j0 + r) * 128 + c] = c < 96 ? tl[r * BG_ALD + BG_E4 + c] : (lv ? vw[c - 96] : 0.f);
                }
            }
            if (any_live) {
                St.prologue(net, bst, T);
                F0.b0 = *reinterpret_cast<const f32x4*>(&bst[T.b0_off]);
                F0.b1 = *reinterpret_cast<const f32x4*>(&bst[T.b1_off]);
                for (int l = 0; l < BG_NL; ++l) {
                    const int a0_off = li * BG_ALD + 4 * lh + (l == 0 ? BG_E4 : 0);
                    f32x16 acc[2];
                    bg_layer(acc, St, net, net.Kp[l] / 32, tl, a0_off, bst, F0, T);
                    // ---- epilogue: bias (+ ReLU, all but feature_linear) back over the tile's columns below 256 (every read of the
                    // tile retired at the last barrier); the view layer has 128 columns: waves 2 and 3 hold nothing of it ----
                    if (l < BG_NL - 1 || wc < 2) {
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn) {
                            const int cl = wc * 64 + tn * 32 + li;
                            const float bv = net.bias[l][cl];
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int rw = (r & 3) + 8 * (r >> 2) + 4 * lh;
                                const float v = acc[tn][r] + bv;
                                tl[rw * BG_ALD + cl] = l == 8 ? v : fmaxf(v, 0.0f);
                            }
                        }
                    }
                    if (l == 8) {               // the view layer's input [feat | view]: the skip columns were last read by layer 5
                        for (int idx = tid; idx < BG_TM * 32; idx += 256) tl[(idx >> 5) * BG_ALD + BG_E4 + (idx & 31)] = vw[idx & 31];
                    }
                    __syncthreads();
                    if (l == 7) {
                        // sigma head on the last hidden layer: one wave per row, the arithmetic of skinny_fwd_kernel<1, 256>.  The next
                        // writer of the tile is feature_linear's epilogue, behind the barriers of its main loop
                        BG_ARGS(qh);
                        const f32x4 w = *reinterpret_cast<const f32x4*>(qh->Wsig + 4 * lane);
                        const float b = qh->bsig[0];
                        for (int r = wc; r < BG_TM; r += 4) {
                            const float a = fm_row_dot(&tl[r * BG_ALD], w, lane);
                            if (lane == 0) rec[r * BG_RD + 2] = a + b;
                        }
                    }
                }
                {
                    // rgb head on the view layer's output: two rows per wave, 32 lanes each -- skinny_fwd_kernel<3, 128>
#pragma clang fp contract(off)
                    BG_ARGS(qh);
                    const int sub = lane >> 5, ln = lane & 31;
                    for (int jh = 0; jh < 3; ++jh) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(qh->Wrgb + jh * 128 + 4 * ln);
                        const float b = qh->brgb[jh];
                        for (int r = 2 * wc + sub; r < BG_TM; r += 8) {
                            const f32x4 h = *reinterpret_cast<const f32x4*>(&tl[r * BG_ALD + 4 * ln]);
                            float a = 0.f;
                            a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
                            for (int of = 16; of > 0; of >>= 1) a += __shfl_xor(a, of);
                            if (ln == 0) rec[r * BG_RD + 3 + jh] = a + b;
                        }
                    }
                }
                __syncthreads();
            }
            // ---- activation (nerf_act_fwd_kernel's expressions): one thread per row; alpha and colour replace the raw heads ----
            if (tid < BG_TM) {
                float* h = &rec[tid * BG_RD];
                const bool lv = h[1] != 0.f;
                const float sg = lv ? h[2] : 0.f, r0 = lv ? h[3] : 0.f, r1 = lv ? h[4] : 0.f, r2 = lv ? h[5] : 0.f;
                float al = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
                if (lv) {
                    al = 1.0f - expf(-bg_softplus1(sg) * h[0]);
                    c0 = nu_linear_to_srgb(expf(fminf(r0, 5.0f)));
                    c1 = nu_linear_to_srgb(expf(fminf(r1, 5.0f)));
                    c2 = nu_linear_to_srgb(expf(fminf(r2, 5.0f)));
                }
                h[2] = al; h[3] = c0; h[4] = c1; h[5] = c2;
                if (j0 + tid < S) {
                    const long long p = (long long)ray * S + j0 + tid;
                    if (q->raw != nullptr) { const f32x4 v = {sg, r0, r1, r2}; *reinterpret_cast<f32x4*>(q->raw + p * 4) = v; }
                    if (q->act != nullptr) { const f32x4 v = {al, c0, c1, c2}; *reinterpret_cast<f32x4*>(q->act + p * 4) = v; }
                }
            }
            __syncthreads();
            {
                // ---- composite, front to back, one sample after the other: colour += (alpha T) c;  T *= fl(1 - alpha + 1e-7) ----
#pragma clang fp contract(off)
                const int n = S - j0 < BG_TM ? S - j0 : BG_TM;
                for (int r = 0; r < n; ++r) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&rec[r * BG_RD + 2]);
                    const float w = q[0] * Tr;
                    col[0] = col[0] + w * q[1]; col[1] = col[1] + w * q[2]; col[2] = col[2] + w * q[3];
                    Tr = Tr * (1.0f - q[0] + 1e-7f);
                }
            }
            __syncthreads();            // the tile's LDS is free for the next tile
        }
        if (tid == 0) {
            BG_ARGS(qo);
            float* const cp = qo->color;
            if (cp != nullptr) { cp[ray * 3LL] = col[0]; cp[ray * 3LL + 1] = col[1]; cp[ray * 3LL + 2] = col[2]; }
            if (qo->trans != nullptr) qo->trans[ray] = Tr;
        }
    }
}

// The learned background of R rays; the contract is stated at nu_background_fwd in include/nu_nerf.h.
extern "C" int nu_background_fwd(const NuNerfNet* net, const float* O, int o_ld, const float* D, int d_ld, const float* z, int S,
                                 const float* t_stop, int R, float* color, float* trans, float* enc_dbg, float* raw_dbg, float* act_dbg,
                                 hipStream_t stream) {
    if (!net || !O || !D || !z || R < 0 || S < 1 || o_ld < 3 || d_ld < 3) return NU_ERR_ARG;
    BgNet n = {};
    for (int l = 0; l < BG_NL; ++l) {
        const NuLin& L = l < 8 ? net->pts[l] : (l == 8 ? net->feat : net->view);
        const int Kp = l == 0 ? 96 : (l == 5 ? 352 : (l == 9 ? 288 : 256));
        const int K = l == 0 ? 84 : (l == 5 ? 340 : (l == 9 ? 283 : 256));
        if (!L.Wp || !L.bias || L.N != (l == 9 ? 128 : 256) || L.Kp != Kp || L.K != K) return NU_ERR_ARG;
        n.Wp[l] = L.Wp; n.bias[l] = L.bias; n.Kp[l] = Kp; n.half[l] = l == 9 ? 1 : 0;
    }
    if (!net->alpha.Wp || !net->alpha.bias || net->alpha.N != 1 || net->alpha.Kp != 256) return NU_ERR_ARG;
    if (!net->rgb.Wp || !net->rgb.bias || net->rgb.N != 3 || net->rgb.Kp != 128) return NU_ERR_ARG;
    if (R == 0) return NU_OK;
    n.Wsig = net->alpha.Wp; n.bsig = net->alpha.bias; n.Wrgb = net->rgb.Wp; n.brgb = net->rgb.bias;
    n.O = O; n.D = D; n.z = z; n.t_stop = t_stop;
    n.o_ld = o_ld; n.d_ld = d_ld; n.S = S; n.R = R;
    n.color = color; n.trans = trans; n.enc = enc_dbg; n.raw = raw_dbg; n.act = act_dbg;
    hipLaunchKernelGGL(background_fwd_kernel, dim3(R < 256 ? R : 256), dim3(256), 0, stream, n);
    return nu_launch_status();
}
