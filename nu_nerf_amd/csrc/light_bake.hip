// light_bake.hip -- the illumination a trained model learned, for a caller's directions, as ONE no-gradient kernel:
// (d, rho, x) -> encodings -> outer_light (, inner_light, inner_weight) -> exp / clamp -> radiance.
//
// Reference: AppShadingNetwork.predict_specular_lights with reflective = d and no human light (network/field.py:636-667, :1399-1430;
// the networks :594-604; offset_points_to_sphere + get_sphere_intersection :447-464):
//   direct   = exp(min(outer_light([IDE(d, rho) | IDE(sph(x, d), rho) if sphere_direction]), exp_max))
//   indirect = exp(min(inner_light([pos_enc(x) | IDE(d, rho)]), exp_max))                                  (probe)
//   occ      = clamp(0.5 inner_weight([pos_enc(x) | dir_enc(d)]) + 0.5, 0, 1)                              (probe)
//   light    = indirect occ + direct (1 - occ)                                                             (probe; else light = direct)
// Inside the training step these networks run as rows of nu_shading_stack_fwd and as the per-ray mirror query nu_spec_encode; the
// layered composition for free directions (nu_spec_encode / nu_ide + three NT GEMMs + nu_skinny_fwd per predictor) writes the encoded
// rows, three [rows, 256] hidden buffers and the ReLU sign masks of a backward nobody runs here.
//
// Design: the pipeline of csrc/fused_mlp.h (32-row tiles) over three input tiles.  A workgroup owns 32 rows for ALL layers of ALL predictors.  The
// three input tiles are built in LDS first, one wave per row, lanes below 36 evaluating the IDE terms with the helpers of the encoding
// kernels (ide.h): ol (32 x 164) = the nu_spec_encode / OLin row, il (32 x 132) = the ILin row, iw (32 x 100) = the IWin row of
// nu_(s2_)shade_encode_fwd.  Per predictor: Kp -> 256 ReLU (from its input tile) -> 256 ReLU -> 256 ReLU (over the activation tile,
// 32 x 260) as exact fp32 MFMA in the k order of gemm_nt2, the weights streamed through two 256 x 36 LDS stages in 32-deep chunks
// behind ONE cursor that crosses every layer boundary; head: one wave per row with the arithmetic of skinny_fwd_kernel<NO, 256>.
// Raw heads wait in a 32 x 8 LDS record until the last predictor is through; one thread per (row, channel) then activates, blends
// and writes.  Nothing else goes to HBM.
// LDS: 33 296 (act) + 21 008 (ol) + 16 912 (il) + 12 816 (iw) + 1 024 (heads) + 73 728 (weight stages) = 158 784 B of the CU's
// 163 840: one workgroup per CU.  Row strides 260 / 164 / 132 / 100 (and 36 of the weight stages) are odd multiples of 4 floats: a
// ds_read_b128 is served in groups of 16 lanes over 64 banks, the 16 rows of a group have 16 different residues mod 16, and an odd
// stride / 4 maps them onto the 16 different 16-byte slots of the 256-byte bank row -- no conflict, as with 260 / 292 in bake.hip.
#include "fused_mlp.h"

#define LB_OLD 164                 // outer_light input row stride (Kp = 96 or 160)
#define LB_ILD 132                 // inner_light input row stride (Kp = 128)
#define LB_WLD 100                 // inner_weight input row stride (Kp = 96)
#define LB_ACT 0                   // offsets into the tile array
#define LB_OL (32 * FM_ALD + FM_APAD)
#define LB_IL (LB_OL + 32 * LB_OLD + FM_APAD)
#define LB_IW (LB_IL + 32 * LB_ILD + FM_APAD)
#define LB_TILE (LB_IW + 32 * LB_WLD + FM_APAD)
#define LB_MAXL 9                  // 3 predictors x 3 hidden layers
#define LB_HD 8                    // raw-head record per row: direct (3), indirect (3), occlusion (1), unused (1)

struct LbNet {                     // kernel-argument block: the layer list in stream order
    const float* Wp[LB_MAXL]; const float* bias[LB_MAXL];
    int Kp[LB_MAXL];
    int a_off[LB_MAXL], a_ld[LB_MAXL];          // A operand of the layer: offset and row stride in the tile array
    int head[LB_MAXL];                          // predictor whose head follows this layer (0 outer_light, 1 inner_light, 2 inner_weight), or -1
    int nl;
    const float* Wh[3]; const float* bh[3];     // heads [3,256], [3,256], [1,256] and their biases
    float exp_max;
    int sphere, ld_ol, pe, probe;               // pe = 3 + 6 pos_freq columns of pos_enc
    const float* dirs; const float* kinv; const float* x;
    int x_stride;                               // floats between the points of two rows; 0: one point for all rows
    float *light, *direct, *indirect, *occ;     // [N,3], [N,3], [N,3], [N]; nullable
    float *enc, *raw;                           // test outputs: encoded rows [N, ld_ol (+ 224)], raw heads [N, 8]; nullable
};

__global__ __launch_bounds__(256, 1) void light_bake_fwd_kernel(LbNet net, int N) {
    constexpr int TM = 32;
    __shared__ __attribute__((aligned(16))) float tl[LB_TILE];
    __shared__ __attribute__((aligned(16))) float hd[TM * LB_HD];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int ntiles = (N + TM - 1) / TM;
    const int nl = net.nl;
    const int ld_ol = net.ld_ol, pe = net.pe;
    const int ld_enc = net.probe ? ld_ol + 224 : ld_ol;
    float* const act = &tl[LB_ACT];

    FmStream S;
    FmFrag F0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * TM;
        // ---- input tiles: one wave per row.  ol = the nu_spec_encode row at this row's roughness; il / iw = the ILin / IWin rows of
        // nu_s2_shade_encode_fwd with r = d ----
        {
            const NuIdeLane IL = nu_ide_lane(lane);
            for (int r = wc; r < TM; r += 4) {
                int p = row0 + r;
                p = p < N ? p : N - 1;
                const float d[3] = {net.dirs[p * 3LL], net.dirs[p * 3LL + 1], net.dirs[p * 3LL + 2]};
                float x[3] = {0.f, 0.f, 0.f};
                if (net.x != nullptr) {
                    const float* xp = net.x + (long long)p * net.x_stride;
                    x[0] = xp[0]; x[1] = xp[1]; x[2] = xp[2];
                }
                const NuIdeDir td = nu_ide_dir(IL, d[0], d[1], d[2]);
                const float att = nu_ide_att(IL, net.kinv[p]);
                float* ol = &tl[LB_OL + r * LB_OLD];
                if (net.sphere) {
                    const NuSph s = nu_sph_point_n2(x, d, nu_sph_norm2(x));      // (ide.h: the encoding kernels' rounding of |x|^2)
                    nu_ide_store(ol, lane, IL, td, att, 72);
                    nu_ide_store(ol + 72, lane, IL, nu_ide_dir(IL, s.s[0], s.s[1], s.s[2]), att, ld_ol - 72);
                } else {
                    nu_ide_store(ol, lane, IL, td, att, ld_ol);
                }
                if (net.probe) {
                    const float e = lane < pe ? nu_embed_col(x, 3, lane) : 0.f;
                    float* il = &tl[LB_IL + r * LB_ILD];
                    float* iw = &tl[LB_IW + r * LB_WLD];
                    if (lane < pe) { il[lane] = e; iw[lane] = e; }
                    nu_ide_store(il + pe, lane, IL, td, att, 128 - pe);
                    if (lane < 39) iw[pe + lane] = nu_embed_col(d, 3, lane);
                    for (int c = pe + 39 + lane; c < 96; c += 64) iw[c] = 0.f;
                }
            }
        }
        S.prologue(net, nl, bst, T);
        if (net.enc != nullptr) {           // test output: the rows as the predictors read them
            for (int idx = tid; idx < TM * ld_enc; idx += 256) {
                const int r = idx / ld_enc, c = idx - r * ld_enc;
                if (row0 + r >= N) break;
                const float v = c < ld_ol ? tl[LB_OL + r * LB_OLD + c]
                              : c < ld_ol + 128 ? tl[LB_IL + r * LB_ILD + c - ld_ol] : tl[LB_IW + r * LB_WLD + c - ld_ol - 128];
                net.enc[(long long)(row0 + r) * ld_enc + c] = v;
            }
        }
        S.first_b(F0, bst, T);

        for (int l = 0; l < nl; ++l) {
            const int nk = net.Kp[l] / 32;
            const int a0_off = net.a_off[l] + li * net.a_ld[l] + 4 * lh;
            const FmAcc<1> A = fm_layer<1>(S, net, nl, nk, tl, a0_off, 0, bst, F0, T);
            const f32x16 (&acc)[2] = A.v[0];
            // ---- epilogue: bias + ReLU into the activation tile (every read of the A tile retired at the last barrier) ----
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                const float bv = net.bias[l][col];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                    act[row * FM_ALD + col] = fmaxf(acc[tn][r] + bv, 0.0f);
                }
            }
            __syncthreads();
            const int pr = net.head[l];
            if (pr >= 0) {
                // head of predictor pr on its last hidden layer: one wave per row, the arithmetic of skinny_fwd_kernel<NO, 256> -> the
                // row's head record.  The next writer of the activation tile is an epilogue behind the barriers of a whole layer.
#pragma clang fp contract(off)
                const int no = pr == 2 ? 1 : 3;
                for (int j = 0; j < no; ++j) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(net.Wh[pr] + j * 256 + 4 * lane);
                    const float b = net.bh[pr][j];
                    for (int r = wc; r < TM; r += 4) {
                        const float a = fm_row_dot(&act[r * FM_ALD], w, lane);
                        if (lane == 0) hd[r * LB_HD + 3 * pr + j] = a + b;
                    }
                }
            }
        }
        __syncthreads();            // every head record of the tile is written
        // ---- activation and blend: one thread per (row, channel) ----
        if (tid < TM * 3) {
#pragma clang fp contract(off)
            const int r = tid / 3, c = tid - 3 * r;
            const long long p = row0 + r;
            if (p < N) {
                const float* h = &hd[r * LB_HD];
                const float dir = expf(fminf(h[c], net.exp_max));
                float lt = dir;
                if (net.probe) {
                    const float ind = expf(fminf(h[3 + c], net.exp_max));
                    const float oc = fminf(fmaxf(h[6] * 0.5f + 0.5f, 0.0f), 1.0f);
                    const float io = ind * oc;
                    lt = io + dir * (1.0f - oc);
                    if (net.indirect != nullptr) net.indirect[p * 3 + c] = io;
                    if (net.occ != nullptr && c == 0) net.occ[p] = oc;
                }
                if (net.light != nullptr) net.light[p * 3 + c] = lt;
                if (net.direct != nullptr) net.direct[p * 3 + c] = dir;
            }
        }
        if (net.raw != nullptr && tid < TM * LB_HD) {
            const int r = tid / LB_HD, c = tid - LB_HD * r;
            const int live = net.probe ? 7 : 3;
            if (row0 + r < N) net.raw[(long long)(row0 + r) * LB_HD + c] = c < live ? hd[tid] : 0.f;
        }
        __syncthreads();            // the tile's LDS is free for the next tile
    }
}

// The learned illumination at N rows (direction dirs [N,3], roughness kinv [N] = the IDE's kappa_inv, point x):
//   x == NULL: the origin for every row; x_stride == 0: the one point x[0..2] for every row; else row p reads x + p * x_stride.
//   probe == 0: light = direct = exp(min(outer_light(row), exp_max)), the row laid out as nu_spec_encode writes it (net->ld_ol).
//   probe != 0 (needs x): additionally inner_light / inner_weight on [pos_enc(x, pos_freq) | ...] laid out as nu_s2_shade_encode_fwd
//   writes ILin / IWin; indirect is already multiplied by occ, light = indirect + direct (1 - occ).
// Every output pointer may be NULL.  enc_dbg [N, ld_ol (+ 128 + 96 with probe)] / raw_dbg [N, 8] (direct 3, indirect 3, occlusion 1
// before their activations, 0): test outputs.  Reads the fp32 packed tables of NuShadeNet.
extern "C" int nu_light_bake_fwd(const NuShadeNet* net, const float* dirs, const float* kinv, const float* x, int x_stride, int pos_freq,
                                 int N, int probe, float* light, float* direct, float* indirect, float* occ, float* enc_dbg,
                                 float* raw_dbg, hipStream_t stream) {
    if (N < 0 || !net || !dirs || !kinv) return NU_ERR_ARG;
    if (probe && !x) return NU_ERR_ARG;
    if (x && x_stride != 0 && x_stride < 3) return NU_ERR_ARG;
    if (N == 0) return NU_OK;
    const int sphere = net->sphere ? 1 : 0;
    if (net->ld_ol != (sphere ? 160 : 96)) return NU_ERR_ARG;
    LbNet n = {};
    int nl = 0;
    auto push = [&](const NuLin* P, int Kp0, int a_off, int a_ld, int pr, int no) -> bool {
        for (int j = 0; j < 3; ++j) {
            const NuLin& L = P[j];
            if (!L.Wp || !L.bias || L.N != 256 || L.Kp != (j == 0 ? Kp0 : 256)) return false;
            n.Wp[nl] = L.Wp; n.bias[nl] = L.bias; n.Kp[nl] = L.Kp;
            n.a_off[nl] = j == 0 ? a_off : LB_ACT; n.a_ld[nl] = j == 0 ? a_ld : FM_ALD;
            n.head[nl] = j == 2 ? pr : -1;
            ++nl;
        }
        const NuLin& H = P[3];
        if (!H.Wp || !H.bias || H.N != no || H.Kp != 256) return false;
        n.Wh[pr] = H.Wp; n.bh[pr] = H.bias;
        return true;
    };
    if (!push(net->outer_light, net->ld_ol, LB_OL, LB_OLD, 0, 3) || net->outer_light[0].K != (sphere ? 144 : 72)) return NU_ERR_ARG;
    const int pe = 3 + 6 * pos_freq;
    if (probe) {
        if (pos_freq < 0 || pos_freq > 8) return NU_ERR_ARG;         // pe + 72 <= 128 and pe + 39 <= 96
        if (!push(net->inner_light, 128, LB_IL, LB_ILD, 1, 3) || net->inner_light[0].K != pe + 72) return NU_ERR_ARG;
        if (!push(net->inner_weight, 96, LB_IW, LB_WLD, 2, 1) || net->inner_weight[0].K != pe + 39) return NU_ERR_ARG;
    }
    n.nl = nl;
    n.exp_max = net->exp_max; n.sphere = sphere; n.ld_ol = net->ld_ol; n.pe = pe; n.probe = probe ? 1 : 0;
    n.dirs = dirs; n.kinv = kinv; n.x = x; n.x_stride = x ? x_stride : 0;
    n.light = light; n.direct = direct; n.indirect = indirect; n.occ = occ; n.enc = enc_dbg; n.raw = raw_dbg;
    const int ntiles = nu_cdiv(N, 32);
    hipLaunchKernelGGL(light_bake_fwd_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, N);
    return nu_launch_status();
}
