// sdf_grad.hip -- the SDF network's FIRST-order jet as ONE no-gradient kernel: x -> f, grad f [3] and the unit normal grad f / |grad f| of
// the level set through x.  The bulk tool of the normal-map bake: millions of texel points that need first order only.
//
// Design: sdf_jet_fwd_kernel (csrc/sdf_jet.hip) with four rows per point instead of ten -- value, d/dx, d/dy, d/dz.  A linear
// layer acts on all four alike, so the hot loop is the [rows, K] x W^T product of csrc/fused_mlp.h on a 64-row tile.  The bias goes to the
// value row only.
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
#include "fused_mlp.h"

#define SG_PTS 16                  // points per 64-row tile

struct SgNet {                     // what the kernel needs of NuSdfNet (kernel-argument block)
    const float* Wp[8]; const float* bias[8];
    const float* w8; const float* b8;
    int Kp[8], N[8];
};
struct SgOut { float *sdf, *grad, *normal; };

__global__ __launch_bounds__(256, 1) void sdf_grad_fwd_kernel(SgNet net, const float* __restrict__ X, int x_ld, int P, SgOut out) {
    constexpr int TM = 64;
    __shared__ __attribute__((aligned(16))) float act[TM * FM_ALD + FM_APAD];
    __shared__ __attribute__((aligned(16))) float emb[TM * FM_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];
    __shared__ float res[TM];

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int a0_off = li * FM_ALD + 4 * lh, a1_off = a0_off + 32 * FM_ALD;
    const int ntiles = (P + SG_PTS - 1) / SG_PTS;
    FmStream S;
    FmFrag F0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long p0 = (long long)tile * SG_PTS;
        // ---- embedding jet of the tile's points: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input.  Points
        //      past the end repeat point P - 1 (read only; nothing of them is stored) ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int row = idx >> 6, c = idx & 63;
            long long p = p0 + (row >> 2);
            p = p < P ? p : P - 1;
            float x[3] = {X[p * x_ld], X[p * x_ld + 1], X[p * x_ld + 2]};
            const float v = fm_embed_jet<1>(x, c, row & 3);
            act[row * FM_ALD + c] = v;
            if (c < FM_ELD) emb[row * FM_ELD + c] = v;
        }
        S.prologue(net, 8, bst, T);
        S.first_b(F0, bst, T);

        for (int l = 0; l < 8; ++l) {
            const FmAcc<2> A = fm_layer<2>(S, net, 8, net.Kp[l] / 32, act, a0_off, a1_off, bst, F0, T);
            const f32x16 (&acc)[2][2] = A.v;
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
                        float* const o = &act[(32 * b + 8 * g + 4 * lh) * FM_ALD + col];
                        o[0] = nu_softplus100_fast(z);
                        o[FM_ALD] = s * acc[b][tn][4 * g + 1];
                        o[2 * FM_ALD] = s * acc[b][tn][4 * g + 2];
                        o[3 * FM_ALD] = s * acc[b][tn][4 * g + 3];
                    }
                }
            }
            if (l == 3) fm_skip_reinsert(act, emb, TM);     // all four rows of a point
            __syncthreads();
        }
        // ---- head: the sdf row of the output layer on every row, one wave per row, the arithmetic of skinny_fwd_kernel<1, 256> ----
        {
            const f32x4 w = *reinterpret_cast<const f32x4*>(net.w8 + 4 * lane);
            for (int r = wc; r < TM; r += 4) {
                const float a = fm_row_dot(&act[r * FM_ALD], w, lane);
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
