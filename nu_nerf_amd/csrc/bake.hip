// bake.hip -- per-vertex material baking as ONE no-gradient kernel: x -> embedding -> the SDF network (eight softplus layers, sdf head
// and the 256 feature columns) -> the material predictors on [feature | x] -> sigmoid -> metallic, roughness, albedo (, transmission).
//
// Replaces, for predict_materials (network/renderer_zerothick.py:846-864, network/renderer.py:885; relight hand-off
// blender_backend/relight_backend.py:26-28):
//   feature = sdf_network(x)[:, 1:]                       network/field.py:133-153
//   color_network.predict_materials(x, feature)           network/field.py:779-783 (make_predictor :386-393)
// which the layered path (nu_sdf_mlp_fwd(..., want_feat = 1) + the materials part of nu_shading_stack_fwd) runs with three [P,1024]
// hidden buffers, YX [P,288], the SDF activations and the ReLU sign masks of a backward nobody runs here.
//
// Design: the pipeline of csrc/fused_mlp.h (32-row tiles) run over a longer layer list than the SDF forward's.  This file's own: a second tile
// yx (32 x 292) = [sdf | feature (256) | x (3) | 0 (28)], the YX row of the layered path (K = 259 padded to 288).  The feature layer
// (rows 1..256 of the SDF output layer, bias, no activation) writes it, and it stays in LDS as the A operand of every predictor's
// first layer.  Per predictor: 288 -> 256 ReLU (from yx) -> 256 ReLU -> 256 ReLU (over the activation tile) -> head: one wave per
// row with the arithmetic of skinny_fwd_kernel (16 bytes per lane, xor-shuffle reduction) -> sigmoid -> global.
// LDS: 33 296 (act) + 37 392 (yx) + 5 120 (embedding) + 73 728 (weight stages) = 149 536 B of the CU's 163 840: one workgroup per CU.
// Arithmetic: exact fp32 MFMA in the k order of the layered path, the same epilogue functions, the same head reduction (the layered
// head reduces a block-diagonal 1024-wide row; the three foreign blocks add exact zeros), so sdf, feature, hidden layers and raw heads
// carry the layered path's bits.
#include "fused_mlp.h"

#define BK_YLD 292                 // yx row stride (= 4 mod 32, as every A tile of csrc/fused_mlp.h)
#define BK_ACT 0                   // offsets into the tile array
#define BK_YX (32 * FM_ALD + FM_APAD)
#define BK_TILE (BK_YX + 32 * BK_YLD + FM_APAD)
#define BK_MAXL 21                 // 8 SDF layers + feature + 4 predictors x 3

enum { BK_SOFTPLUS = 0, BK_FEATURE = 1, BK_RELU = 2 };

struct BkNet {                     // kernel-argument block: the layer list in stream order
    const float* Wp[BK_MAXL]; const float* bias[BK_MAXL];
    int Kp[BK_MAXL], N[BK_MAXL];
    int kind[BK_MAXL];             // BK_SOFTPLUS / BK_FEATURE / BK_RELU
    int from_yx[BK_MAXL];          // A operand: the yx tile (a predictor's first layer) instead of the activation tile
    int head[BK_MAXL];             // predictor whose head follows this layer, or -1
    int nl;
    const float* w8; const float* b8;           // sdf head
    const float* Ws6; const float* b6;          // block-diagonal material heads [6, 1024], [6]
    float* out[4];                              // metallic [P], roughness [P], albedo [P,3], transmission [P]
    float* sdf; float* feat;                    // [P], [P,256]; nullable
    int raw;
};

__global__ __launch_bounds__(256, 1) void material_bake_fwd_kernel(BkNet net, const float* __restrict__ X, int x_ld, int P) {
    constexpr int TM = 32;
    __shared__ __attribute__((aligned(16))) float tl[BK_TILE];
    __shared__ __attribute__((aligned(16))) float emb[TM * FM_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int ntiles = (P + TM - 1) / TM;
    const int nl = net.nl;
    float* const act = &tl[BK_ACT];
    float* const yx = &tl[BK_YX];

    FmStream S;
    FmFrag F0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * TM;
        // ---- embedding of the tile's points: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            int p = row0 + r;
            p = p < P ? p : P - 1;
            float x[3] = {X[(long long)p * x_ld], X[(long long)p * x_ld + 1], X[(long long)p * x_ld + 2]};
            const float v = c < 39 ? fm_embed_col(x, c) : 0.f;
            act[r * FM_ALD + c] = v;
            if (c < FM_ELD) emb[r * FM_ELD + c] = v;
            // the tail of the yx row: x at columns 257..259 (nu_sdf_embed), zeros up to 288
            if (c >= 1 && c < 32) yx[r * BK_YLD + 256 + c] = c < 4 ? x[c - 1] : 0.f;
        }
        S.prologue(net, nl, bst, T);
        S.first_b(F0, bst, T);

        for (int l = 0; l < nl; ++l) {
            const int nk = net.Kp[l] / 32;
            const int a0_off = net.from_yx[l] ? BK_YX + li * BK_YLD + 4 * lh : BK_ACT + li * FM_ALD + 4 * lh;
            const FmAcc<1> A = fm_layer<1>(S, net, nl, nk, tl, a0_off, 0, bst, F0, T);
            const f32x16 (&acc)[2] = A.v[0];
            // ---- epilogue (every read of the A tile retired at the last barrier) ----
            const int N = net.N[l];
            const int kind = net.kind[l];
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                const float bv = col < N ? net.bias[l][col] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const float v = acc[tn][r] + bv;
                    if (kind == BK_SOFTPLUS) {
                        // columns [N, 256) (layer 3: the slots of the skip embedding) are not this layer's
                        if (col < N) act[row * FM_ALD + col] = nu_softplus100_fast(v);
                    } else if (kind == BK_RELU) {
                        act[row * FM_ALD + col] = fmaxf(v, 0.0f);
                    } else {            // feature columns: plain, into the yx tile behind the sdf slot
                        yx[row * BK_YLD + 1 + col] = v;
                        if (net.feat != nullptr && row0 + row < P) net.feat[(long long)(row0 + row) * 256 + col] = v;
                    }
                }
            }
            if (l == 3) fm_skip_reinsert(act, emb, TM);
            if (kind == BK_FEATURE) {
                // sdf head on the last hidden layer (still in the activation tile): one wave per row, the arithmetic of
                // skinny_fwd_kernel<1, 256> -> yx column 0 (and global)
#pragma clang fp contract(off)
                const f32x4 w = *reinterpret_cast<const f32x4*>(net.w8 + 4 * lane);
                const float b = net.b8[0];
                for (int r = wc; r < TM; r += 4) {
                    const float a = fm_row_dot(&act[r * FM_ALD], w, lane);
                    if (lane == 0) {
                        yx[r * BK_YLD] = a + b;
                        if (net.sdf != nullptr && row0 + r < P) net.sdf[row0 + r] = a + b;
                    }
                }
            }
            __syncthreads();
            const int pr = net.head[l];
            if (pr >= 0) {
                // head of predictor pr on its last hidden layer: rows hr .. hr + no of the block-diagonal table, columns 256 pr ..;
                // the arithmetic of skinny_fwd_kernel<6, 1024> on the one block that is not zero.  The next writer of the activation
                // tile is an epilogue behind the barriers of a whole layer.
#pragma clang fp contract(off)
                const int hr = pr < 3 ? pr : 5, no = pr == 2 ? 3 : 1;
                float* const out = net.out[pr];
                for (int j = 0; j < no; ++j) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(net.Ws6 + (long long)(hr + j) * 1024 + pr * 256 + 4 * lane);
                    const float b = net.b6[hr + j];
                    for (int r = wc; r < TM; r += 4) {
                        const float a = fm_row_dot(&act[r * FM_ALD], w, lane);
                        if (lane == 0 && row0 + r < P) {
                            const float v = a + b;
                            out[(long long)(row0 + r) * no + j] = net.raw ? v : 1.0f / (1.0f + expf(-v));
                        }
                    }
                }
            }
        }
        __syncthreads();            // the tile's LDS is free for the next tile
    }
}

extern "C" int nu_bake_net_size(void) { return (int)sizeof(NuBakeNet); }

// metallic [P], roughness [P], albedo [P,3] (, transmission [P], sdf [P]) of the points X [P, x_ld] (first three floats of a row = x):
// sigmoid of the material predictors on [SDF feature | x], exact fp32, nothing else written.  Every output pointer may be NULL: a
// predictor whose output is not asked for is not evaluated.
extern "C" int nu_material_bake_fwd(const NuBakeNet* net, const float* X, int x_ld, int P, float* metallic, float* roughness, float* albedo,
                                    float* transmission, float* sdf, hipStream_t stream) {
    if (P <= 0) return NU_OK;
    if (!net || !X || x_ld < 3) return NU_ERR_ARG;
    if (net->n_pred < 3 || net->n_pred > 4 || (transmission && net->n_pred < 4)) return NU_ERR_ARG;
    if (!net->WpM0 || !net->bM0 || !net->WpM[1] || !net->WpM[2] || !net->bM[1] || !net->bM[2] || !net->Ws6 || !net->b6) return NU_ERR_ARG;
    BkNet n = {};
    int nl = 0;
    auto push = [&](const float* W, const float* b, int Kp, int N, int kind, int from_yx) {
        n.Wp[nl] = W; n.bias[nl] = b; n.Kp[nl] = Kp; n.N[nl] = N; n.kind[nl] = kind; n.from_yx[nl] = from_yx;
        n.head[nl] = -1;
        ++nl;
    };
    for (int l = 0; l < 8; ++l) {
        const NuLin& L = net->sdf.lin[l];
        const int Kexp = l == 0 ? 64 : 256;
        if (L.Kp != Kexp || L.N > 256 || L.N < 1 || !L.Wp || !L.bias) return NU_ERR_ARG;     // SDFNetwork(dims 39 -> 8 x 256 -> 257, skip at 4)
        push(L.Wp, L.bias, L.Kp, L.N, BK_SOFTPLUS, 0);
    }
    const NuLin& L8 = net->sdf.lin[8];
    if (net->sdf.lin[3].N != 217 || L8.Kp != 256 || L8.N != 257 || !L8.Wp || !L8.bias) return NU_ERR_ARG;
    n.w8 = L8.Wp; n.b8 = L8.bias;
    push(L8.Wp + 256, L8.bias + 1, 256, 256, BK_FEATURE, 0);       // rows 1..256 of the output layer
    float* const outs[4] = {metallic, roughness, albedo, transmission};
    for (int p = 0; p < net->n_pred; ++p) {
        if (!outs[p]) continue;
        push(net->WpM0 + (long long)p * 256 * 288, net->bM0 + p * 256, 288, 256, BK_RELU, 1);
        push(net->WpM[1] + (long long)p * 65536, net->bM[1] + p * 256, 256, 256, BK_RELU, 0);
        push(net->WpM[2] + (long long)p * 65536, net->bM[2] + p * 256, 256, 256, BK_RELU, 0);
        n.head[nl - 1] = p;
        n.out[p] = outs[p];
    }
    n.nl = nl;
    n.Ws6 = net->Ws6; n.b6 = net->b6;
    n.sdf = sdf; n.feat = net->feat; n.raw = net->raw;
    const int ntiles = nu_cdiv(P, 32);
    hipLaunchKernelGGL(material_bake_fwd_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, X, x_ld, P);
    return nu_launch_status();
}
