// sdf_jet.hip -- the SDF network's second-order jet as ONE no-gradient kernel: x -> f, grad f [3], Hessian f [6] (xx, yy, zz, xy, xz,
// yz) -> mean and Gaussian curvature of the level set through x and its unit normal.
//
//   g = grad f, H = Hessian f;  mean = (|g|^2 tr H - g^T H g) / (2 |g|^3);  gauss = g^T adj(H) g / |g|^4;  n = g / |g|
// (f = |x| - r: mean = 1 / r, gauss = 1 / r^2.)  Nothing else in the library evaluates H: the reverse sweep gives g, the training
// backward Hessian-vector terms only.
//
// Design: forward-mode propagation of the jet through the pipeline of csrc/fused_mlp.h on a 64-row tile.  A point carries ten rows --
// value, d/dx, d/dy, d/dz, d2/dxx, yy, zz, xy, xz, yz -- and a linear layer acts on all ten alike, so the hot loop is the existing
// [rows, K] x W^T product.  The bias goes to the value row only.
// Row order: in the accumulators of v_mfma_f32_32x32x2f32 a lane of half h = lane / 32 holds, per 32-row block, the 16 rows
// (r & 3) + 8 (r >> 2) + 4 h.  Over the tile's two blocks that is 32 rows per lane = the 3 x 10 rows of three points (+ 2 idle), so
// point q of half h is given exactly the rows of that lane's accumulator slots 10 q .. 10 q + 9 (slot s = 16 block + r): the
// softplus epilogue, which mixes the ten rows of a point per column, runs in registers with static indices -- no pass over LDS, no
// barrier, no scratch.  A tile is 6 points on 60 of 64 rows.
//   a = sp(z), a_i = s z_i, a_ij = 100 s (1 - s) z_i z_j + s z_ij,  s = sigmoid(100 z)
// The embedding jet (value, 2^k cos / -2^k sin on the point's own axis, -4^k sin / -4^k cos on (c, c)) is kept in LDS and re-inserted
// in all ten rows at the skip.  Head: the sdf row of lin8 on all rows, one wave per row with the arithmetic of skinny_fwd_kernel<1,
// 256>; then one thread per point forms the curvatures.
// The value row runs the MFMA k order, the softplus and the head of nu_sdf_fused_fwd: the sdf output carries its bits.
// LDS: 66 576 (activations) + 10 240 (embedding jet) + 73 728 (weight stages) + 256 (head results) = 150 800 B: one workgroup per CU.
#include "fused_mlp.h"

#define SJ_PTS 6                   // points per 64-row tile

// tile row of jet component j (0..9) of tile point pt (0..5): slot s = 10 q + j of the lanes of half h (pt = 3 h + q)
static __device__ inline int sj_row(int pt, int j) {
    const int h = pt >= 3 ? 1 : 0;
    const int s = (pt - 3 * h) * 10 + j;
    const int r = s & 15;
    return (s >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
}

struct SjNet {                     // what the kernel needs of NuSdfNet (kernel-argument block)
    const float* Wp[8]; const float* bias[8];
    const float* w8; const float* b8;
    int Kp[8], N[8];
};
struct SjOut { float *sdf, *grad, *hess, *mean, *gauss, *normal; };

__global__ __launch_bounds__(256, 1) void sdf_jet_fwd_kernel(SjNet net, const float* __restrict__ X, int x_ld, int P, SjOut out) {
    constexpr int TM = 64;
    __shared__ __attribute__((aligned(16))) float act[TM * FM_ALD + FM_APAD];
    __shared__ __attribute__((aligned(16))) float emb[TM * FM_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];
    __shared__ float res[TM];

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int a0_off = li * FM_ALD + 4 * lh, a1_off = a0_off + 32 * FM_ALD;
    const int ntiles = (P + SJ_PTS - 1) / SJ_PTS;

    FmStream S;
    FmFrag F0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int p0 = tile * SJ_PTS;
        // ---- embedding jet of the tile's points: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input; the
        //      two idle rows of each half (slots 30, 31) are zero and stay zero ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int row = idx >> 6, c = idx & 63;
            const int rr = row & 31;
            const int h = (rr >> 2) & 1;
            const int s = (row >> 5) * 16 + (rr & 3) + 4 * (rr >> 3);
            float v = 0.f;
            if (s < 30) {
                const int q = s / 10, j = s - 10 * q;
                long long p = p0 + 3 * h + q;
                p = p < P ? p : P - 1;
                float x[3] = {X[p * x_ld], X[p * x_ld + 1], X[p * x_ld + 2]};
                v = fm_embed_jet<2>(x, c, j);
            }
            act[row * FM_ALD + c] = v;
            if (c < FM_ELD) emb[row * FM_ELD + c] = v;
        }
        S.prologue(net, 8, bst, T);
        S.first_b(F0, bst, T);

        for (int l = 0; l < 8; ++l) {
            const FmAcc<2> A = fm_layer<2>(S, net, 8, net.Kp[l] / 32, act, a0_off, a1_off, bst, F0, T);
            const f32x16 (&acc)[2][2] = A.v;
            // ---- epilogue: the softplus jet of each of this lane's three points, back over the activation tile (all reads of it
            //      retired at the last barrier).  Slot s = 10 q + j lives in acc[s >> 4][tn][s & 15]: static after unrolling ----
            const int N = net.N[l];
#define SJ_A(j) acc[(q * 10 + (j)) >> 4][tn][(q * 10 + (j)) & 15]
#define SJ_ROW(j) ((((q * 10 + (j)) >> 4) * 32 + ((q * 10 + (j)) & 3) + 8 * (((q * 10 + (j)) & 15) >> 2) + 4 * lh) * FM_ALD)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                // columns [N, 256) (layer 3: the slots of the skip embedding) are not this layer's
                if (col >= N) continue;
                const float bv = net.bias[l][col];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float z = SJ_A(0) + bv;
                    const float t = __builtin_amdgcn_exp2f(-144.26950408889634f * fabsf(z));      // exp(-|100 z|)
                    const float d = 1.0f / (1.0f + t);
                    const float s = z >= 0.f ? d : t * d;                                         // sigmoid(100 z)
                    const float c2 = 100.0f * (t * d * d);                                        // 100 s (1 - s)
                    const float z1 = SJ_A(1), z2 = SJ_A(2), z3 = SJ_A(3);
                    float* const o = &act[col];
                    o[SJ_ROW(0)] = nu_softplus100_fast(z);
                    o[SJ_ROW(1)] = s * z1;
                    o[SJ_ROW(2)] = s * z2;
                    o[SJ_ROW(3)] = s * z3;
                    o[SJ_ROW(4)] = c2 * (z1 * z1) + s * SJ_A(4);
                    o[SJ_ROW(5)] = c2 * (z2 * z2) + s * SJ_A(5);
                    o[SJ_ROW(6)] = c2 * (z3 * z3) + s * SJ_A(6);
                    o[SJ_ROW(7)] = c2 * (z1 * z2) + s * SJ_A(7);
                    o[SJ_ROW(8)] = c2 * (z1 * z3) + s * SJ_A(8);
                    o[SJ_ROW(9)] = c2 * (z2 * z3) + s * SJ_A(9);
                }
            }
#undef SJ_A
#undef SJ_ROW
            if (l == 3) fm_skip_reinsert(act, emb, TM);     // all ten rows of a point
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
        // ---- per point: f, g, H -> curvatures and normal ----
        if (tid < SJ_PTS && p0 + tid < P) {
            const long long p = p0 + tid;
            float v[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) v[j] = res[sj_row(tid, j)];
            const float f = v[0] + net.b8[0];                  // the bias belongs to the value row only
            const float gx = v[1], gy = v[2], gz = v[3];
            const float hxx = v[4], hyy = v[5], hzz = v[6], hxy = v[7], hxz = v[8], hyz = v[9];
            const float g2 = gx * gx + gy * gy + gz * gz;
            float km = 0.f, kg = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
            if (g2 >= 1e-12f) {
                const float gn = sqrtf(g2);
                const float gHg = gx * (hxx * gx + hxy * gy + hxz * gz) + gy * (hxy * gx + hyy * gy + hyz * gz)
                                  + gz * (hxz * gx + hyz * gy + hzz * gz);
                km = (g2 * (hxx + hyy + hzz) - gHg) / (2.0f * g2 * gn);
                // adj(H), symmetric
                const float axx = hyy * hzz - hyz * hyz, ayy = hxx * hzz - hxz * hxz, azz = hxx * hyy - hxy * hxy;
                const float axy = hxz * hyz - hxy * hzz, axz = hxy * hyz - hxz * hyy, ayz = hxy * hxz - hyz * hxx;
                const float gAg = gx * (axx * gx + axy * gy + axz * gz) + gy * (axy * gx + ayy * gy + ayz * gz)
                                  + gz * (axz * gx + ayz * gy + azz * gz);
                kg = gAg / (g2 * g2);
                const float ig = 1.0f / gn;
                nx = gx * ig; ny = gy * ig; nz = gz * ig;
            }
            if (out.sdf) out.sdf[p] = f;
            if (out.grad) { out.grad[3 * p] = gx; out.grad[3 * p + 1] = gy; out.grad[3 * p + 2] = gz; }
            if (out.hess) {
                float* const o = out.hess + 6 * p;
                o[0] = hxx; o[1] = hyy; o[2] = hzz; o[3] = hxy; o[4] = hxz; o[5] = hyz;
            }
            if (out.mean) out.mean[p] = km;
            if (out.gauss) out.gauss[p] = kg;
            if (out.normal) { out.normal[3 * p] = nx; out.normal[3 * p + 1] = ny; out.normal[3 * p + 2] = nz; }
        }
        __syncthreads();            // the tile's LDS is free for the next tile
    }
}

// f [P], grad f [P,3], Hessian f [P,6] (xx, yy, zz, xy, xz, yz), mean and Gaussian curvature [P] of the level set through each point
// and its unit normal [P,3], for X [P, x_ld] (first three floats of a row = x).  Exact fp32 on the fp32 packed tables, nothing kept, no
// workspace.  Every output pointer may be NULL.
extern "C" int nu_sdf_jet_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, float* grad, float* hess, float* mean,
                              float* gauss, float* normal, hipStream_t stream) {
    if (!net || !X || P < 0 || x_ld < 3) return NU_ERR_ARG;
    if (P == 0) return NU_OK;
    SjNet n;
    for (int l = 0; l < 8; ++l) {
        const NuLin& L = net->lin[l];
        const int Kexp = l == 0 ? 64 : 256;
        if (L.Kp != Kexp || L.N > 256 || L.N < 1 || !L.Wp || !L.bias) return NU_ERR_ARG;     // SDFNetwork(dims 39 -> 8 x 256 -> 257, skip at 4)
        n.Wp[l] = L.Wp; n.bias[l] = L.bias; n.Kp[l] = L.Kp; n.N[l] = L.N;
    }
    if (net->lin[3].N != 217 || net->lin[8].Kp != 256 || !net->lin[8].Wp || !net->lin[8].bias) return NU_ERR_ARG;
    n.w8 = net->lin[8].Wp; n.b8 = net->lin[8].bias;
    const SjOut out = {sdf, grad, hess, mean, gauss, normal};
    const int ntiles = nu_cdiv(P, SJ_PTS);
    hipLaunchKernelGGL(sdf_jet_fwd_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, X, x_ld, P, out);
    return nu_launch_status();
}
