// sdf_grad.hip -- the SDF network's FIRST-order jet as ONE no-gradient kernel: x -> f, grad f [3] and the unit normal grad f / |grad f| of
// the level set through x.  The bulk tool of the normal-map bake: millions of texel points that need first order only.
//
// Design: the pipeline of sdf_jet_fwd_kernel (csrc/sdf_jet.hip) restated with four rows per point instead of ten -- value,
// d/dx, d/dy, d/dz.  A linear layer acts on all four alike, so the hot loop is the [rows, K] x W^T product on exact-fp32 MFMA: the
// activation tile (64 x 260) is the A operand of every layer, the fp32 packed weights (the skip's 1 / sqrt 2 folded in) stream through
// two 256 x 36 LDS stages behind one cursor that crosses layer boundaries.  The bias goes to the value row only.
// Row order: tile row 4 p + j is component j of tile point p = 0..15.  In the accumulators of v_mfma_f32_32x32x2f32 a lane of half
// h = lane / 32 holds, per 32-row block b, the 16 rows (r & 3) + 8 (r >> 2) + 4 h, so registers 4 g .. 4 g + 3 of a block are the four
// rows of ONE point, 8 b + 2 g + h: the softplus epilogue, which mixes the four rows of a point per column, runs in registers with static
// indices -- no pass over LDS, no barrier, no scratch, and no idle row.  A tile is 16 points on all 64 rows (the jet: 6 on 60).
//   a = sp(z), a_i = s z_i,  s = sigmoid(100 z)
// The embedding jet (value, 2^k cos / -2^k sin on the point's own axis) is kept in LDS and re-inserted in all four rows at the skip.
// Head: the sdf row of lin8 on all rows, one wave per row with the arithmetic of skinny_fwd_kernel<1, 256>; then one thread per point
// forms the normal.
// Every row runs the MFMA k order, the epilogue expressions and the head of sdf_jet_fwd_kernel, and a row's result does not depend on
// which tile row carries it: sdf carries the bits of nu_sdf_fused_fwd, grad and normal the bits of nu_sdf_jet_fwd.
// LDS: 66 576 (activations) + 10 240 (embedding jet) + 73 728 (weight stages) + 256 (head results) = 150 800 B: one workgroup per CU.
#include "gemm.h"

#define SG_ALD 260                 // activation row stride (floats)
#define SG_ELD 40                  // embedding row stride
#define SG_BLD 36                  // weight-stage row stride
#define SG_BSTAGE (256 * SG_BLD)
#define SG_PTS 16                  // points per 64-row tile

// jet component j (0: value, 1..3: d/dx, d/dy, d/dz) of column col of get_embedder(6, 3) at x: sj_embed_jet (sdf_jet.hip) for j <= 3
static __device__ inline float sg_embed_jet(const float* x, int col, int j) {
    if (col >= 39) return 0.f;
    if (col < 3) return j == 0 ? x[col] : (j == 1 + col ? 1.f : 0.f);
    const int q = col - 3;
    const int k = q / 6;
    const int r = q - k * 6;
    const int c = r >= 3 ? r - 3 : r;
    const float fk = (float)(1 << k);
    const float a = x[c] * fk;
    if (j == 0) return r >= 3 ? cosf(a) : sinf(a);
    if (j == 1 + c) return r >= 3 ? -fk * sinf(a) : fk * cosf(a);
    return 0.f;
}

struct SgNet {                     // what the kernel needs of NuSdfNet (kernel-argument block)
    const float* Wp[8]; const float* bias[8];
    const float* w8; const float* b8;
    int Kp[8], N[8];
};
struct SgOut { float *sdf, *grad, *normal; };

__global__ __launch_bounds__(256, 1) void sdf_grad_fwd_kernel(SgNet net, const float* __restrict__ X, int x_ld, int P, SgOut out) {
    constexpr int TM = 64;
    __shared__ __attribute__((aligned(16))) float act[TM * SG_ALD + 4];     // (+ 4: a layer's last chunk prefetches the fragment slot behind the last row; never used)
    __shared__ __attribute__((aligned(16))) float emb[TM * SG_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * SG_BSTAGE];
    __shared__ float res[TM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wc = tid >> 6;                                  // this wave's 64 output columns
    const int li = lane & 31, lh = lane >> 5;
    const int c4 = tid & 7, r0 = tid >> 3;                    // weight loader: rows r0 + 32 i (i < 8), 16-byte slot c4
    const int a0_off = li * SG_ALD + 4 * lh, a1_off = a0_off + 32 * SG_ALD;
    const int b0_off = (wc * 64 + li) * SG_BLD + 4 * lh, b1_off = b0_off + 32 * SG_BLD;
    const int w_off = r0 * SG_BLD + 4 * c4;
    const int ntiles = (P + SG_PTS - 1) / SG_PTS;

    // ---- weight loader: a cursor over the chunks of all eight layers, in order (past the end it stays on the last chunk) ----
    int ld_l = 0, ld_kt = 0;
    const float* bp = nullptr;                                // this thread's slot of row r0 of the chunk at the cursor
    long long bstep = 0;                                      // 32 rows further
    f32x4 rb4[8];
    auto set_cursor = [&]() {
        bp = net.Wp[ld_l] + (long long)r0 * net.Kp[ld_l] + 4 * c4 + ld_kt * 32;
        bstep = 32LL * net.Kp[ld_l];
    };
    auto advance = [&]() {
        if (++ld_kt == net.Kp[ld_l] / 32) {
            if (ld_l == 7) { --ld_kt; return; }
            ld_kt = 0;
            ++ld_l;
        }
        set_cursor();
    };
    struct Frag { f32x4 a0, a1, b0, b1; };

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long p0 = (long long)tile * SG_PTS;
        // ---- embedding jet of the tile's points: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input.  Points
        //      past the end repeat point P - 1 (read only; nothing of them is stored) ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int row = idx >> 6, c = idx & 63;
            long long p = p0 + (row >> 2);
            p = p < P ? p : P - 1;
            float x[3] = {X[p * x_ld], X[p * x_ld + 1], X[p * x_ld + 2]};
            const float v = sg_embed_jet(x, c, row & 3);
            act[row * SG_ALD + c] = v;
            if (c < SG_ELD) emb[row * SG_ELD + c] = v;
        }
        // ---- weight pipeline prologue: chunk 0 -> stage 0, chunk 1 -> registers ----
        ld_l = 0; ld_kt = 0;
        set_cursor();
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(&bst[w_off + 32 * i * SG_BLD]) = rb4[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
        __syncthreads();
        int cur = 0;
        Frag F0, F1;
        F0.b0 = *reinterpret_cast<const f32x4*>(&bst[b0_off]);
        F0.b1 = *reinterpret_cast<const f32x4*>(&bst[b1_off]);

        for (int l = 0; l < 8; ++l) {
            const int nk = net.Kp[l] / 32;
            f32x16 acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
            // first A fragments of the layer (the activation tile was rewritten by the previous layer's epilogue)
            F0.a0 = *reinterpret_cast<const f32x4*>(&act[a0_off]);
            F0.a1 = *reinterpret_cast<const f32x4*>(&act[a1_off]);
#define SG_PIN __builtin_amdgcn_sched_barrier(0);
#define SG_M(F, e, i, j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a##i[e], F.b##j[e], acc[i][j], 0, 0, 0); SG_PIN
#define SG_RA0(F, k0, kk) F.a0 = *reinterpret_cast<const f32x4*>(&act[a0_off + (k0) + (kk) * 8]); SG_PIN
#define SG_RA1(F, k0, kk) F.a1 = *reinterpret_cast<const f32x4*>(&act[a1_off + (k0) + (kk) * 8]); SG_PIN
#define SG_RB(F, S, kk, m) F.m = *reinterpret_cast<const f32x4*>(&(S)[m##_off + (kk) * 8]); SG_PIN
#define SG_W(i) *reinterpret_cast<f32x4*>(&so[w_off + 32 * (i) * SG_BLD]) = rb4[i]; SG_PIN
#define SG_L(i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + (i) * bstep); SG_PIN
            const float* sc = &bst[cur * SG_BSTAGE];
            for (int kt = 0; kt < nk; ++kt) {
                float* so = &bst[(cur ^ 1) * SG_BSTAGE];
                const int k0 = kt * 32;
                // k-group 0: fragment reads of k-group 1
                SG_M(F0, 0, 0, 0) SG_M(F0, 0, 0, 1) SG_RA0(F1, k0, 1) SG_M(F0, 0, 1, 0) SG_M(F0, 0, 1, 1)
                SG_M(F0, 1, 0, 0) SG_M(F0, 1, 0, 1) SG_RA1(F1, k0, 1) SG_M(F0, 1, 1, 0) SG_M(F0, 1, 1, 1)
                SG_M(F0, 2, 0, 0) SG_M(F0, 2, 0, 1) SG_RB(F1, sc, 1, b0) SG_M(F0, 2, 1, 0) SG_M(F0, 2, 1, 1)
                SG_M(F0, 3, 0, 0) SG_M(F0, 3, 0, 1) SG_RB(F1, sc, 1, b1) SG_M(F0, 3, 1, 0) SG_M(F0, 3, 1, 1)
                // k-group 1: the next weight chunk registers -> other stage; fragment reads of k-group 2
                SG_M(F1, 0, 0, 0) SG_W(0) SG_M(F1, 0, 0, 1) SG_RA0(F0, k0, 2) SG_M(F1, 0, 1, 0) SG_W(1) SG_M(F1, 0, 1, 1)
                SG_M(F1, 1, 0, 0) SG_W(2) SG_M(F1, 1, 0, 1) SG_RA1(F0, k0, 2) SG_M(F1, 1, 1, 0) SG_W(3) SG_M(F1, 1, 1, 1)
                SG_M(F1, 2, 0, 0) SG_W(4) SG_M(F1, 2, 0, 1) SG_RB(F0, sc, 2, b0) SG_M(F1, 2, 1, 0) SG_W(5) SG_M(F1, 2, 1, 1)
                SG_M(F1, 3, 0, 0) SG_W(6) SG_M(F1, 3, 0, 1) SG_RB(F0, sc, 2, b1) SG_M(F1, 3, 1, 0) SG_W(7) SG_M(F1, 3, 1, 1)
                // k-group 2: the chunk after that global -> registers; fragment reads of k-group 3
                SG_M(F0, 0, 0, 0) SG_L(0) SG_M(F0, 0, 0, 1) SG_RA0(F1, k0, 3) SG_M(F0, 0, 1, 0) SG_L(1) SG_M(F0, 0, 1, 1)
                SG_M(F0, 1, 0, 0) SG_L(2) SG_M(F0, 1, 0, 1) SG_RA1(F1, k0, 3) SG_M(F0, 1, 1, 0) SG_L(3) SG_M(F0, 1, 1, 1)
                SG_M(F0, 2, 0, 0) SG_L(4) SG_M(F0, 2, 0, 1) SG_RB(F1, sc, 3, b0) SG_M(F0, 2, 1, 0) SG_L(5) SG_M(F0, 2, 1, 1)
                SG_M(F0, 3, 0, 0) SG_L(6) SG_M(F0, 3, 0, 1) SG_RB(F1, sc, 3, b1) SG_M(F0, 3, 1, 0) SG_L(7) SG_M(F0, 3, 1, 1)
                advance();
                __syncthreads();        // the other stage is complete; every wave holds its last fragments of this chunk
                // k-group 3: first fragments of the next chunk (weights: the other stage, also across a layer boundary).  The activation
                // reads are unconditional and after a layer's last chunk return bytes nobody uses (the next layer re-reads them)
                SG_M(F1, 0, 0, 0) SG_M(F1, 0, 0, 1) SG_RA0(F0, k0 + 32, 0) SG_M(F1, 0, 1, 0) SG_M(F1, 0, 1, 1)
                SG_M(F1, 1, 0, 0) SG_M(F1, 1, 0, 1) SG_RA1(F0, k0 + 32, 0) SG_M(F1, 1, 1, 0) SG_M(F1, 1, 1, 1)
                SG_M(F1, 2, 0, 0) SG_M(F1, 2, 0, 1) SG_RB(F0, so, 0, b0) SG_M(F1, 2, 1, 0) SG_M(F1, 2, 1, 1)
                SG_M(F1, 3, 0, 0) SG_M(F1, 3, 0, 1) SG_RB(F0, so, 0, b1) SG_M(F1, 3, 1, 0) SG_M(F1, 3, 1, 1)
                cur ^= 1;
                sc = so;
            }
#undef SG_M
#undef SG_RA0
#undef SG_RA1
#undef SG_RB
#undef SG_W
#undef SG_L
#undef SG_PIN
            // ---- epilogue: the softplus jet of each of this lane's eight points, back over the activation tile (all reads of it
            //      retired at the last barrier).  Component j of point 8 b + 2 g + h lives in acc[b][tn][4 g + j], tile row
            //      32 b + 8 g + 4 h + j: static after unrolling ----
            const int N = net.N[l];
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                // columns [N, 256) (layer 3: the slots of the skip embedding) are not this layer's
                if (col >= N) continue;
                const float bv = net.bias[l][col];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float z = acc[b][tn][4 * g] + bv;
                        const float t = __builtin_amdgcn_exp2f(-144.26950408889634f * fabsf(z));      // exp(-|100 z|)
                        const float d = 1.0f / (1.0f + t);
                        const float s = z >= 0.f ? d : t * d;                                         // sigmoid(100 z)
                        float* const o = &act[(32 * b + 8 * g + 4 * lh) * SG_ALD + col];
                        o[0] = nu_softplus100_fast(z);
                        o[SG_ALD] = s * acc[b][tn][4 * g + 1];
                        o[2 * SG_ALD] = s * acc[b][tn][4 * g + 2];
                        o[3 * SG_ALD] = s * acc[b][tn][4 * g + 3];
                    }
                }
            }
            if (l == 3) {               // layer 4's input: [h4 (217) | embedding (39)], all four rows of a point
                for (int idx = tid; idx < TM * 39; idx += 256) {
                    const int r = idx / 39, c = idx - r * 39;
                    act[r * SG_ALD + 217 + c] = emb[r * SG_ELD + c];
                }
            }
            __syncthreads();
        }
        // ---- head: the sdf row of the output layer on every row, one wave per row, the arithmetic of skinny_fwd_kernel<1, 256> ----
        {
#pragma clang fp contract(off)
            const f32x4 w = *reinterpret_cast<const f32x4*>(net.w8 + 4 * lane);
            for (int r = wc; r < TM; r += 4) {
                const f32x4 h = *reinterpret_cast<const f32x4*>(&act[r * SG_ALD + 4 * lane]);
                float a = 0.f;
                a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                if (lane == 0) res[r] = a;
            }
        }
        __syncthreads();
        // ---- per point: f, g -> normal (the expressions of sdf_jet_fwd_kernel) ----
        if (tid < SG_PTS && p0 + tid < P) {
            const long long p = p0 + tid;
            const float f = res[4 * tid] + net.b8[0];          // the bias belongs to the value row only
            const float gx = res[4 * tid + 1], gy = res[4 * tid + 2], gz = res[4 * tid + 3];
            const float g2 = gx * gx + gy * gy + gz * gz;
            float nx = 0.f, ny = 0.f, nz = 0.f;
            if (g2 >= 1e-12f) {
                const float gn = sqrtf(g2);
                const float ig = 1.0f / gn;
                nx = gx * ig; ny = gy * ig; nz = gz * ig;
            }
            if (out.sdf) out.sdf[p] = f;
            if (out.grad) { out.grad[3 * p] = gx; out.grad[3 * p + 1] = gy; out.grad[3 * p + 2] = gz; }
            if (out.normal) { out.normal[3 * p] = nx; out.normal[3 * p + 1] = ny; out.normal[3 * p + 2] = nz; }
        }
        __syncthreads();            // the tile's LDS is free for the next tile
    }
}

// f [P], grad f [P,3] and the unit normal grad f / |grad f| [P,3] (0 where |grad f|^2 < 1e-12) for X [P, x_ld] (first three floats of a
// row = x).  Exact fp32 on the fp32 packed tables, nothing kept, no workspace.  Every output pointer may be NULL.
extern "C" int nu_sdf_grad_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, float* grad, float* normal,
                               hipStream_t stream) {
    if (!net || !X || P < 0 || x_ld < 3) return NU_ERR_ARG;
    if (P == 0) return NU_OK;
    SgNet n;
    for (int l = 0; l < 8; ++l) {
        const NuLin& L = net->lin[l];
        const int Kexp = l == 0 ? 64 : 256;
        if (L.Kp != Kexp || L.N > 256 || L.N < 1 || !L.Wp || !L.bias) return NU_ERR_ARG;     // SDFNetwork(dims 39 -> 8 x 256 -> 257, skip at 4)
        n.Wp[l] = L.Wp; n.bias[l] = L.bias; n.Kp[l] = L.Kp; n.N[l] = L.N;
    }
    if (net->lin[3].N != 217 || net->lin[8].Kp != 256 || !net->lin[8].Wp || !net->lin[8].bias) return NU_ERR_ARG;
    n.w8 = net->lin[8].Wp; n.b8 = net->lin[8].bias;
    const SgOut out = {sdf, grad, normal};
    const int ntiles = nu_cdiv(P, SG_PTS);
    hipLaunchKernelGGL(sdf_grad_fwd_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, X, x_ld, P, out);
    return nu_launch_status();
}
