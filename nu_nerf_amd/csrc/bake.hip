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
// Design: the pipeline of sdf_fused_fwd_kernel<1> (csrc/fused_sdf.hip) run over a longer layer list.  A workgroup owns 32 points for
// ALL layers; the activation tile (32 x 260) is the A operand and the epilogue's target of every 256-wide layer; the weights stream
// through two 256 x 36 LDS stages in 32-deep chunks behind ONE cursor that crosses every layer boundary.  New here: a second tile
// yx (32 x 292) = [sdf | feature (256) | x (3) | 0 (28)], the YX row of the layered path (K = 259 padded to 288).  The feature layer
// (rows 1..256 of the SDF output layer, bias, no activation) writes it, and it stays in LDS as the A operand of every predictor's
// first layer.  Per predictor: 288 -> 256 ReLU (from yx) -> 256 ReLU -> 256 ReLU (over the activation tile) -> head: one wave per
// row with the arithmetic of skinny_fwd_kernel (16 bytes per lane, xor-shuffle reduction) -> sigmoid -> global.
// LDS: 33 296 (act) + 37 392 (yx) + 5 120 (embedding) + 73 728 (weight stages) = 149 536 B of the CU's 163 840: one workgroup per CU.
// Arithmetic: exact fp32 MFMA in the k order of the layered path, the same epilogue functions, the same head reduction (the layered
// head reduces a block-diagonal 1024-wide row; the three foreign blocks add exact zeros), so sdf, feature, hidden layers and raw heads
// carry the layered path's bits.
#include "gemm.h"

#define BK_ALD 260                 // activation row stride (floats)
#define BK_YLD 292                 // yx row stride (292 mod 32 = 4, as 260: ds_read_b128 fragment reads hit every 16-byte slot once per 16 rows)
#define BK_ELD 40                  // embedding row stride
#define BK_BLD 36                  // weight-stage row stride
#define BK_BSTAGE (256 * BK_BLD)
#define BK_ACT 0                   // offsets into the tile array
#define BK_YX (32 * BK_ALD + 4)    // (+ 4: a layer's last chunk prefetches the fragment slot behind the last row; never used)
#define BK_TILE (BK_YX + 32 * BK_YLD + 4)
#define BK_MAXL 21                 // 8 SDF layers + feature + 4 predictors x 3

enum { BK_SOFTPLUS = 0, BK_FEATURE = 1, BK_RELU = 2 };

static __device__ inline float bk_embed_col(const float* x, int col) {      // get_embedder(6, 3) column (fused_sdf.hip: fs_embed_col)
    if (col < 3) return x[col];
    const int q = col - 3;
    const int k = q / 6;
    const int r = q - k * 6;
    const int c = r >= 3 ? r - 3 : r;
    const float a = x[c] * (float)(1 << k);
    return r >= 3 ? cosf(a) : sinf(a);
}

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
    __shared__ __attribute__((aligned(16))) float emb[TM * BK_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * BK_BSTAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wc = tid >> 6;                                  // this wave's 64 output columns
    const int li = lane & 31, lh = lane >> 5;
    const int c4 = tid & 7, r0 = tid >> 3;                    // weight loader: rows r0 + 32 i (i < 8), 16-byte slot c4
    const int b0_off = (wc * 64 + li) * BK_BLD + 4 * lh, b1_off = b0_off + 32 * BK_BLD;
    const int w_off = r0 * BK_BLD + 4 * c4;
    const int ntiles = (P + TM - 1) / TM;
    const int nl = net.nl;
    float* const act = &tl[BK_ACT];
    float* const yx = &tl[BK_YX];

    // ---- weight loader: a cursor over the chunks of all layers, in order (past the end it stays on the last chunk) ----
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
            if (ld_l == nl - 1) { --ld_kt; return; }
            ld_kt = 0;
            ++ld_l;
        }
        set_cursor();
    };
    struct Frag { f32x4 a0, b0, b1; };

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * TM;
        // ---- embedding of the tile's points: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            int p = row0 + r;
            p = p < P ? p : P - 1;
            float x[3] = {X[(long long)p * x_ld], X[(long long)p * x_ld + 1], X[(long long)p * x_ld + 2]};
            const float v = c < 39 ? bk_embed_col(x, c) : 0.f;
            act[r * BK_ALD + c] = v;
            if (c < BK_ELD) emb[r * BK_ELD + c] = v;
            // the tail of the yx row: x at columns 257..259 (nu_sdf_embed), zeros up to 288
            if (c >= 1 && c < 32) yx[r * BK_YLD + 256 + c] = c < 4 ? x[c - 1] : 0.f;
        }
        // ---- weight pipeline prologue: chunk 0 -> stage 0, chunk 1 -> registers ----
        ld_l = 0; ld_kt = 0;
        set_cursor();
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(&bst[w_off + 32 * i * BK_BLD]) = rb4[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
        __syncthreads();
        int cur = 0;
        Frag F0, F1;
        F0.b0 = *reinterpret_cast<const f32x4*>(&bst[b0_off]);
        F0.b1 = *reinterpret_cast<const f32x4*>(&bst[b1_off]);

        for (int l = 0; l < nl; ++l) {
            const int nk = net.Kp[l] / 32;
            const int a0_off = net.from_yx[l] ? BK_YX + li * BK_YLD + 4 * lh : BK_ACT + li * BK_ALD + 4 * lh;
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
            // first A fragment of the layer (its tile was rewritten by an earlier layer's epilogue)
            F0.a0 = *reinterpret_cast<const f32x4*>(&tl[a0_off]);
#define BK_PIN __builtin_amdgcn_sched_barrier(0);
#define BK_M(F, e, j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a0[e], F.b##j[e], acc[j], 0, 0, 0); BK_PIN
#define BK_RA(F, k0, kk) F.a0 = *reinterpret_cast<const f32x4*>(&tl[a0_off + (k0) + (kk) * 8]); BK_PIN
#define BK_RB(F, S, kk, m) F.m = *reinterpret_cast<const f32x4*>(&(S)[m##_off + (kk) * 8]); BK_PIN
#define BK_W(i) *reinterpret_cast<f32x4*>(&so[w_off + 32 * (i) * BK_BLD]) = rb4[i]; BK_PIN
#define BK_L(i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + (i) * bstep); BK_PIN
            const float* sc = &bst[cur * BK_BSTAGE];
            for (int kt = 0; kt < nk; ++kt) {
                float* so = &bst[(cur ^ 1) * BK_BSTAGE];
                const int k0 = kt * 32;
                // k-group 0: fragment reads of k-group 1
                BK_M(F0, 0, 0) BK_M(F0, 0, 1) BK_RA(F1, k0, 1)
                BK_M(F0, 1, 0) BK_M(F0, 1, 1)
                BK_M(F0, 2, 0) BK_M(F0, 2, 1) BK_RB(F1, sc, 1, b0)
                BK_M(F0, 3, 0) BK_M(F0, 3, 1) BK_RB(F1, sc, 1, b1)
                // k-group 1: the next weight chunk registers -> other stage; fragment reads of k-group 2
                BK_M(F1, 0, 0) BK_W(0) BK_M(F1, 0, 1) BK_RA(F0, k0, 2) BK_W(1)
                BK_M(F1, 1, 0) BK_W(2) BK_M(F1, 1, 1) BK_W(3)
                BK_M(F1, 2, 0) BK_W(4) BK_M(F1, 2, 1) BK_RB(F0, sc, 2, b0) BK_W(5)
                BK_M(F1, 3, 0) BK_W(6) BK_M(F1, 3, 1) BK_RB(F0, sc, 2, b1) BK_W(7)
                // k-group 2: the chunk after that global -> registers; fragment reads of k-group 3
                BK_M(F0, 0, 0) BK_L(0) BK_M(F0, 0, 1) BK_RA(F1, k0, 3) BK_L(1)
                BK_M(F0, 1, 0) BK_L(2) BK_M(F0, 1, 1) BK_L(3)
                BK_M(F0, 2, 0) BK_L(4) BK_M(F0, 2, 1) BK_RB(F1, sc, 3, b0) BK_L(5)
                BK_M(F0, 3, 0) BK_L(6) BK_M(F0, 3, 1) BK_RB(F1, sc, 3, b1) BK_L(7)
                advance();
                __syncthreads();        // the other stage is complete; every wave holds its last fragments of this chunk
                // k-group 3: first fragments of the next chunk (weights: the other stage, also across a layer boundary).  The A read is
                // unconditional and after a layer's last chunk returns bytes nobody uses (the next layer re-reads its first fragment)
                BK_M(F1, 0, 0) BK_M(F1, 0, 1) BK_RA(F0, k0 + 32, 0)
                BK_M(F1, 1, 0) BK_M(F1, 1, 1)
                BK_M(F1, 2, 0) BK_M(F1, 2, 1) BK_RB(F0, so, 0, b0)
                BK_M(F1, 3, 0) BK_M(F1, 3, 1) BK_RB(F0, so, 0, b1)
                cur ^= 1;
                sc = so;
            }
#undef BK_M
#undef BK_RA
#undef BK_RB
#undef BK_W
#undef BK_L
#undef BK_PIN
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
                        if (col < N) act[row * BK_ALD + col] = nu_softplus100_fast(v);
                    } else if (kind == BK_RELU) {
                        act[row * BK_ALD + col] = fmaxf(v, 0.0f);
                    } else {            // feature columns: plain, into the yx tile behind the sdf slot
                        yx[row * BK_YLD + 1 + col] = v;
                        if (net.feat != nullptr && row0 + row < P) net.feat[(long long)(row0 + row) * 256 + col] = v;
                    }
                }
            }
            if (l == 3) {               // layer 4's input: [h4 (217) | embedding (39)]
                for (int idx = tid; idx < TM * 39; idx += 256) {
                    const int r = idx / 39, c = idx - r * 39;
                    act[r * BK_ALD + 217 + c] = emb[r * BK_ELD + c];
                }
            }
            if (kind == BK_FEATURE) {
                // sdf head on the last hidden layer (still in the activation tile): one wave per row, the arithmetic of
                // skinny_fwd_kernel<1, 256> -> yx column 0 (and global)
#pragma clang fp contract(off)
                const f32x4 w = *reinterpret_cast<const f32x4*>(net.w8 + 4 * lane);
                const float b = net.b8[0];
                for (int r = wc; r < TM; r += 4) {
                    const f32x4 h = *reinterpret_cast<const f32x4*>(&act[r * BK_ALD + 4 * lane]);
                    float a = 0.f;
                    a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
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
                        const f32x4 h = *reinterpret_cast<const f32x4*>(&act[r * BK_ALD + 4 * lane]);
                        float a = 0.f;
                        a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
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
