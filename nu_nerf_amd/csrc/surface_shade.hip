// surface_shade.hip -- the appearance a trained model learned, at a caller's surface points, as ONE no-gradient kernel:
// (x, v, n, raw material heads) -> n^, v^, NoV, r, rho -> the seven predictor rows (outer_light x 3, inner_light x 2, inner_weight,
// refrac_light) -> exp / clamp -> occlusion mix, split-sum FG table, Schlick, transmission mix -> sRGB.
//
// Reference: AppShadingNetwork.forward in its stage-1 form (network/field.py:684-777; AppShadingNetwork_SpecInner is the same form with
// light_pos_freq 8, refrac_freq 2 and a refraction light capped at exp(-0.2), :1321-1445).  The human-light stack is never evaluated:
// for a model trained with shader_config.human_light the photographer's term is left out (human_weight = 0), as nu_light_bake_fwd does.
// Inside the training step and in shading_glue.shade this is the layered composition nu_s2_shade_encode_fwd -> the four stacks (three NT
// GEMMs + nu_skinny_fwd each) -> nu_shade_combine_fwd, which writes every encoded row, 21 hidden buffers of [rows, 256] and the ReLU sign
// masks of a backward nobody runs here.
//
// Design: the pipeline of csrc/fused_mlp.h over per-pass input tiles, as in light_bake_fwd_kernel (csrc/light_bake.hip) -- here still in
// this file's own text (SS_ macros below, ss_embed_col).  On the header's fm_layer this kernel's chunk loop comes out with one
// s_waitcnt lgkmcnt(0) where it has two in a row, and with the header's helpers alone it measured 0.1 - 0.3 % slower; it moves when that
// is a measured change of its own (profiles/r07/README.md).  A workgroup owns 32 points for ALL 21 layers of the seven
// predictor passes.  Per tile: one wave per point forms the geometry record (x, n^, v^, r, NoV, rho: nu_s2_dirs' arithmetic, restated)
// in LDS.  Per pass: the pass's input tile (32 x 164, ONE region reused by all seven passes -- seven tiles at once would not fit beside the
// activation tile and the weight stages) is built right before its first layer, one wave per row, lanes below 36 evaluating the IDE terms
// with the helpers of the encoding kernels (ide.h); then Kp -> 256 ReLU -> 256 ReLU -> 256 ReLU over the activation tile (32 x 260) as
// exact fp32 MFMA in the k order of gemm_nt2, the weights streamed through two 256 x 36 LDS stages in 32-deep chunks behind ONE cursor
// that crosses every layer and pass boundary (outer_light is streamed three times and inner_light twice from L2: the simple choice);
// head: one wave per row with the arithmetic of skinny_fwd_kernel<NO, 256>.  Raw heads wait in a 32 x 20 LDS record; after the last pass
// one thread per point does the mix with the expression shapes of shade_combine_kernel (csrc/render.hip) and stores.  Nothing else goes
// to HBM.
// LDS: 33 296 (act) + 21 008 (input) + 2 560 (heads) + 2 560 (geometry) + 73 728 (weight stages) = 133 152 B of the CU's 163 840: one
// workgroup per CU.  Row strides 260 / 164 / 36 are odd multiples of 4 floats (no ds_read_b128 bank conflict, as in light_bake.hip).
#include "gemm.h"
#include "ide.h"

#define SS_ALD 260                 // activation row stride (floats)
#define SS_ILD 164                 // input-tile row stride (Kp <= 160)
#define SS_BLD 36                  // weight-stage row stride
#define SS_BSTAGE (256 * SS_BLD)
#define SS_ACT 0                   // offsets into the tile array (+ 4 each: a layer's last chunk prefetches the fragment slot behind
#define SS_IN (32 * SS_ALD + 4)    //  the last row; never used)
#define SS_TILE (SS_IN + 32 * SS_ILD + 4)
#define SS_NPASS 7                 // outer_light: diffuse | specular | mirror; inner_light: specular | mirror; inner_weight; refrac_light
#define SS_MAXL (3 * SS_NPASS)
#define SS_HD 20                   // raw-head record per row: the passes' heads in order (3 3 3 3 3 1 3), one unused
#define SS_LONE 2                  // the colour channel the combine kernel's vectoriser leaves to scalar code (see the mix)
#define SS_GD 20                   // geometry record per row: x (3), n^ (3), v^ (3), r (3), NoV, rho, unused

struct SsNet {                     // kernel-argument block: the layer list in stream order
    const float* Wp[SS_MAXL]; const float* bias[SS_MAXL];
    int Kp[SS_MAXL];
    const float* Wh[SS_NPASS]; const float* bh[SS_NPASS];      // the head after each pass and its bias
    const float* lut;
    float exp_max, refrac_exp_max;
    int sphere, ld_ol, pe, rdim, ld_rl, linear;                 // pe = 3 + 6 pos_freq, rdim = 3 + 6 refrac_freq columns
    const float *X, *V, *Nrm, *Mraw;
    int x_ld, v_ld, n_ld, ldm;
    float *color, *diffuse_color, *specular_color, *diffuse_light, *specular_light, *indirect_light, *refraction_light;   // [P,3]
    float *occ_prob, *reflection_weight;                        // [P]
    float *enc, *raw;                                           // test outputs: [P, 3 ld_ol + 352 + ld_rl], [P, 20]
};

// The argument block again, behind a pointer the optimiser cannot see through: fields read through it are loaded from the kernel-argument
// segment where they are used, instead of being hoisted out of the tile loop and held in SGPRs across the main loop (which spilled).
typedef const __attribute__((address_space(4))) SsNet* SsArgs;
#define SS_ARGS(q, net) SsArgs q = (SsArgs)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(q))      /* `net` is the first argument */

// n^ = n / max(|n|, 1e-12), v^ likewise; NoV = n^ . v^; r = 2 NoV n^ - v^   (nu_s2_dirs of csrc/encode.hip).  The encoded rows carry the
// bits of nu_s2_shade_encode_fwd only if these few sums round as they do there, and contraction is the compiler's choice per kernel: the
// sums are written out with the fused steps that kernel's gfx950 code has (a . a = a2 a2 + fma(a1, a1, a0 a0), not fused at the top;
// r = fma(NoV n^, 2, -v^)) and nothing else may fuse.
static __device__ inline void ss_dirs(const float* n, const float* v, float* nh, float* vh, float* r, float& nov) {
#pragma clang fp contract(off)
    const float nn = n[2] * n[2] + __builtin_fmaf(n[1], n[1], n[0] * n[0]);
    const float vv = v[2] * v[2] + __builtin_fmaf(v[1], v[1], v[0] * v[0]);
    const float inorm = 1.0f / fmaxf(sqrtf(nn), 1e-12f);
    const float ivn = 1.0f / fmaxf(sqrtf(vv), 1e-12f);
#pragma unroll
    for (int c = 0; c < 3; ++c) { nh[c] = n[c] * inorm; vh[c] = v[c] * ivn; }
    nov = nh[2] * vh[2] + __builtin_fmaf(nh[0], vh[0], nh[1] * vh[1]);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = __builtin_fmaf(nov * nh[c], 2.0f, -vh[c]);
}

// nu_embed_col(x, 3, col) of ide.h with the coordinate picked by selects (an array indexed by the lane would live in private memory)
static __device__ inline float ss_embed_col(const float* x, int col) {
    const int q = col < 3 ? 0 : col - 3;
    const int k = q / 6;
    const int r = q - k * 6;
    const int c = col < 3 ? col : (r >= 3 ? r - 3 : r);
    const float xc = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
    if (col < 3) return xc;
    const float a = xc * (float)(1 << k);
    return r >= 3 ? cosf(a) : sinf(a);
}

// texel centres at (i+0.5)/256, bilinear, clamp to edge (nu_lut of csrc/render.hip, the value part).  Fused steps as in the gfx950 code of
// shade_combine_kernel<false, false>: top = fma(tx, l01, (1 - tx) l00), bot = fma(1 - tx, l10, tx l11), value = (1 - ty) top + ty bot unfused.
static __device__ inline void ss_lut(const float* __restrict__ lut, float u, float v, float& A, float& B) {
#pragma clang fp contract(off)
    const float fx_raw = __builtin_fmaf(u, 256.0f, -0.5f), fy_raw = __builtin_fmaf(v, 256.0f, -0.5f);
    const float fx = fminf(fmaxf(fx_raw, 0.f), 255.f), fy = fminf(fmaxf(fy_raw, 0.f), 255.f);
    const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    const int x1 = x0 + 1 < 255 ? x0 + 1 : 255, y1 = y0 + 1 < 255 ? y0 + 1 : 255;
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const float* l00 = lut + ((long long)y0 * 256 + x0) * 2;
    const float* l01 = lut + ((long long)y0 * 256 + x1) * 2;
    const float* l10 = lut + ((long long)y1 * 256 + x0) * 2;
    const float* l11 = lut + ((long long)y1 * 256 + x1) * 2;
    float val[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float top = __builtin_fmaf(tx, l01[c], (1 - tx) * l00[c]);
        const float bot = __builtin_fmaf(1 - tx, l10[c], tx * l11[c]);
        val[c] = (1 - ty) * top + ty * bot;
    }
    A = val[0]; B = val[1];
}

__global__ __launch_bounds__(256, 1) void surface_shade_fwd_kernel(SsNet net, int P) {
    constexpr int TM = 32;
    __shared__ __attribute__((aligned(16))) float tl[SS_TILE];
    __shared__ __attribute__((aligned(16))) float hd[TM * SS_HD];
    __shared__ __attribute__((aligned(16))) float gd[TM * SS_GD];
    __shared__ __attribute__((aligned(16))) float bst[2 * SS_BSTAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wc = tid >> 6;                                  // this wave's 64 output columns
    const int li = lane & 31, lh = lane >> 5;
    const int c4 = tid & 7, r0 = tid >> 3;                    // weight loader: rows r0 + 32 i (i < 8), 16-byte slot c4
    const int b0_off = (wc * 64 + li) * SS_BLD + 4 * lh, b1_off = b0_off + 32 * SS_BLD;
    const int w_off = r0 * SS_BLD + 4 * c4;
    const int ntiles = (P + TM - 1) / TM;
    const int ld_ol = net.ld_ol, pe = net.pe, rdim = net.rdim, ld_rl = net.ld_rl;
    const int ld_enc = 3 * ld_ol + 352 + ld_rl;
    float* const act = &tl[SS_ACT];
    float* const inp = &tl[SS_IN];

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
            if (ld_l == SS_MAXL - 1) { --ld_kt; return; }
            ld_kt = 0;
            ++ld_l;
        }
        set_cursor();
    };
    struct Frag { f32x4 a0, b0, b1; };
    const NuIdeLane IL = nu_ide_lane(lane);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * TM;
        {
            // ---- geometry record: one wave per point as in the encoding kernel (every lane the same arithmetic), lanes below 14 store ----
            SS_ARGS(q, net);
            for (int r = wc; r < TM; r += 4) {
                int p = row0 + r;
                p = p < P ? p : P - 1;
                const float* xp = q->X + (long long)p * q->x_ld;
                const float* vp = q->V + (long long)p * q->v_ld;
                const float* np_ = q->Nrm + (long long)p * q->n_ld;
                const float n[3] = {np_[0], np_[1], np_[2]}, v[3] = {vp[0], vp[1], vp[2]};
                float nh[3], vh[3], rr[3], nov;
                ss_dirs(n, v, nh, vh, rr, nov);
                const float rho = nu_sigmoid(q->Mraw[(long long)p * q->ldm + 1]);
                if (lane < 14) {
                    float o = rho;
                    if (lane < 3) o = lane == 0 ? xp[0] : (lane == 1 ? xp[1] : xp[2]);
                    else if (lane < 6) o = lane == 3 ? nh[0] : (lane == 4 ? nh[1] : nh[2]);
                    else if (lane < 9) o = lane == 6 ? vh[0] : (lane == 7 ? vh[1] : vh[2]);
                    else if (lane < 12) o = lane == 9 ? rr[0] : (lane == 10 ? rr[1] : rr[2]);
                    else if (lane == 12) o = nov;
                    gd[r * SS_GD + lane] = o;
                }
            }
        }
        // ---- weight pipeline prologue: chunk 0 -> stage 0, chunk 1 -> registers (the stages are free: the barrier that ends a tile) ----
        ld_l = 0; ld_kt = 0;
        set_cursor();
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(&bst[w_off + 32 * i * SS_BLD]) = rb4[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
        advance();
        __syncthreads();
        int cur = 0;
        Frag F0, F1;

        for (int l = 0; l < SS_MAXL; ++l) {
            const int pass = l / 3, lj = l - 3 * pass;
            if (lj == 0) {
                // ---- the pass's input tile: one wave per row, the rows of nu_s2_shade_encode_fwd.  The tile's last reader was the first
                // layer of the pass before, two layers of barriers ago ----
                const int kin = net.Kp[l];
                for (int r = wc; r < TM; r += 4) {
                    const float* g = &gd[r * SS_GD];
                    const float x[3] = {g[0], g[1], g[2]}, nh[3] = {g[3], g[4], g[5]}, vh[3] = {g[6], g[7], g[8]}, rf[3] = {g[9], g[10], g[11]};
                    const float rho = g[13];
                    float* row = &inp[r * SS_ILD];
                    if (pass < 3) {
                        const float d[3] = {pass == 0 ? nh[0] : rf[0], pass == 0 ? nh[1] : rf[1], pass == 0 ? nh[2] : rf[2]};
                        const NuIdeDir td = nu_ide_dir(IL, d[0], d[1], d[2]);
                        const float att_rho = nu_ide_att(IL, rho);
                        const float att = pass == 0 ? IL.att1 : (pass == 1 ? att_rho : 1.0f);
                        if (net.sphere) {
                            const NuSph s = nu_sph_point(x, d);
                            nu_ide_store(row, lane, IL, td, att, 72);
                            nu_ide_store(row + 72, lane, IL, nu_ide_dir(IL, s.s[0], s.s[1], s.s[2]), pass == 0 ? IL.att1 : att_rho, ld_ol - 72);
                        } else {
                            nu_ide_store(row, lane, IL, td, att, ld_ol);
                        }
                    } else if (pass < 5) {
                        const float e = lane < pe ? ss_embed_col(x, lane) : 0.f;
                        const NuIdeDir tr = nu_ide_dir(IL, rf[0], rf[1], rf[2]);
                        if (lane < pe) row[lane] = e;
                        nu_ide_store(row + pe, lane, IL, tr, pass == 3 ? nu_ide_att(IL, rho) : 1.0f, 128 - pe);
                    } else if (pass == 5) {
                        const float e = lane < pe ? ss_embed_col(x, lane) : 0.f;
                        if (lane < pe) row[lane] = e;
                        if (lane < 39) row[pe + lane] = ss_embed_col(rf, lane);
                        for (int c = pe + 39 + lane; c < 96; c += 64) row[c] = 0.f;
                    } else {
                        const float e = lane < pe ? ss_embed_col(x, lane) : 0.f;
                        if (lane < rdim) {
                            row[lane] = e;                      // the rf-frequency code is a prefix of the pos_freq one (rdim <= pe)
                            row[rdim + lane] = ss_embed_col(vh, lane);
                        }
                        for (int c = 2 * rdim + lane; c < ld_rl; c += 64) row[c] = 0.f;
                    }
                }
                __syncthreads();
                if (net.enc != nullptr) {       // test output: the rows as the predictors read them
                    const int eoff = pass < 3 ? pass * ld_ol : (pass < 5 ? 3 * ld_ol + (pass - 3) * 128 : (pass == 5 ? 3 * ld_ol + 256 : 3 * ld_ol + 352));
                    for (int idx = tid; idx < TM * kin; idx += 256) {
                        const int r = idx / kin, c = idx - r * kin;
                        if (row0 + r >= P) break;
                        net.enc[(long long)(row0 + r) * ld_enc + eoff + c] = inp[r * SS_ILD + c];
                    }
                }
                if (l == 0) {
                    F0.b0 = *reinterpret_cast<const f32x4*>(&bst[b0_off]);
                    F0.b1 = *reinterpret_cast<const f32x4*>(&bst[b1_off]);
                }
            }
            const int nk = net.Kp[l] / 32;
            const int a0_off = (lj == 0 ? SS_IN + li * SS_ILD : SS_ACT + li * SS_ALD) + 4 * lh;
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
            // first A fragment of the layer (the A tile was rewritten just before)
            F0.a0 = *reinterpret_cast<const f32x4*>(&tl[a0_off]);
#define SS_PIN __builtin_amdgcn_sched_barrier(0);
#define SS_M(F, e, j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a0[e], F.b##j[e], acc[j], 0, 0, 0); SS_PIN
#define SS_RA(F, k0, kk) F.a0 = *reinterpret_cast<const f32x4*>(&tl[a0_off + (k0) + (kk) * 8]); SS_PIN
#define SS_RB(F, S, kk, m) F.m = *reinterpret_cast<const f32x4*>(&(S)[m##_off + (kk) * 8]); SS_PIN
#define SS_W(i) *reinterpret_cast<f32x4*>(&so[w_off + 32 * (i) * SS_BLD]) = rb4[i]; SS_PIN
#define SS_L(i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + (i) * bstep); SS_PIN
            const float* sc = &bst[cur * SS_BSTAGE];
            for (int kt = 0; kt < nk; ++kt) {
                float* so = &bst[(cur ^ 1) * SS_BSTAGE];
                const int k0 = kt * 32;
                // k-group 0: fragment reads of k-group 1
                SS_M(F0, 0, 0) SS_M(F0, 0, 1) SS_RA(F1, k0, 1)
                SS_M(F0, 1, 0) SS_M(F0, 1, 1)
                SS_M(F0, 2, 0) SS_M(F0, 2, 1) SS_RB(F1, sc, 1, b0)
                SS_M(F0, 3, 0) SS_M(F0, 3, 1) SS_RB(F1, sc, 1, b1)
                // k-group 1: the next weight chunk registers -> other stage; fragment reads of k-group 2
                SS_M(F1, 0, 0) SS_W(0) SS_M(F1, 0, 1) SS_RA(F0, k0, 2) SS_W(1)
                SS_M(F1, 1, 0) SS_W(2) SS_M(F1, 1, 1) SS_W(3)
                SS_M(F1, 2, 0) SS_W(4) SS_M(F1, 2, 1) SS_RB(F0, sc, 2, b0) SS_W(5)
                SS_M(F1, 3, 0) SS_W(6) SS_M(F1, 3, 1) SS_RB(F0, sc, 2, b1) SS_W(7)
                // k-group 2: the chunk after that global -> registers; fragment reads of k-group 3
                SS_M(F0, 0, 0) SS_L(0) SS_M(F0, 0, 1) SS_RA(F1, k0, 3) SS_L(1)
                SS_M(F0, 1, 0) SS_L(2) SS_M(F0, 1, 1) SS_L(3)
                SS_M(F0, 2, 0) SS_L(4) SS_M(F0, 2, 1) SS_RB(F1, sc, 3, b0) SS_L(5)
                SS_M(F0, 3, 0) SS_L(6) SS_M(F0, 3, 1) SS_RB(F1, sc, 3, b1) SS_L(7)
                advance();
                __syncthreads();        // the other stage is complete; every wave holds its last fragments of this chunk
                // k-group 3: first fragments of the next chunk (weights: the other stage, also across a layer boundary).  The A read is
                // unconditional and after a layer's last chunk returns bytes nobody uses (the next layer re-reads its first fragment)
                SS_M(F1, 0, 0) SS_M(F1, 0, 1) SS_RA(F0, k0 + 32, 0)
                SS_M(F1, 1, 0) SS_M(F1, 1, 1)
                SS_M(F1, 2, 0) SS_M(F1, 2, 1) SS_RB(F0, so, 0, b0)
                SS_M(F1, 3, 0) SS_M(F1, 3, 1) SS_RB(F0, so, 0, b1)
                cur ^= 1;
                sc = so;
            }
#undef SS_M
#undef SS_RA
#undef SS_RB
#undef SS_W
#undef SS_L
#undef SS_PIN
            // ---- epilogue: bias + ReLU into the activation tile (every read of the A tile retired at the last barrier) ----
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                const float bv = net.bias[l][col];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                    act[row * SS_ALD + col] = fmaxf(acc[tn][r] + bv, 0.0f);
                }
            }
            __syncthreads();
            if (lj == 2) {
                // head of the pass on its last hidden layer: one wave per row, the arithmetic of skinny_fwd_kernel<NO, 256> -> the row's
                // head record.  The next writer of the activation tile is an epilogue behind the barriers of a whole layer.
#pragma clang fp contract(off)
                const int no = pass == 5 ? 1 : 3;
                const int hoff = pass < 6 ? 3 * pass : 16;
                for (int j = 0; j < no; ++j) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(net.Wh[pass] + j * 256 + 4 * lane);
                    const float b = net.bh[pass][j];
                    for (int r = wc; r < TM; r += 4) {
                        const f32x4 h = *reinterpret_cast<const f32x4*>(&act[r * SS_ALD + 4 * lane]);
                        float a = 0.f;
                        a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                        if (lane == 0) hd[r * SS_HD + hoff + j] = a + b;
                    }
                }
            }
        }
        __syncthreads();            // every head record of the tile is written
        // ---- the mix: one thread per point, the expression shapes of shade_combine_kernel<false, false> ----
        if (tid < TM && row0 + tid < P) {
            SS_ARGS(q, net);
            const long long p = row0 + tid;
            const float* h = &hd[tid * SS_HD];
            const float* mr = q->Mraw + p * q->ldm;
            const float exp_max = q->exp_max;
            const float met = nu_sigmoid(mr[0]), rho = nu_sigmoid(mr[1]), T = nu_sigmoid(mr[5]);
            const float alb[3] = {nu_sigmoid(mr[2]), nu_sigmoid(mr[3]), nu_sigmoid(mr[4])};
            const float nov = gd[tid * SS_GD + 12];
            float Ld[3], dir[3], dir0[3], ind[3], ind0[3], refr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ld[c] = expf(fminf(h[c], exp_max));
                dir[c] = expf(fminf(h[3 + c], exp_max));
                dir0[c] = expf(fminf(h[6 + c], exp_max));
                ind[c] = expf(fminf(h[9 + c], exp_max));
                ind0[c] = expf(fminf(h[12 + c], exp_max));
                refr[c] = expf(fminf(fminf(h[16 + c], q->refrac_exp_max), exp_max));
            }
            {
            // Contraction is the compiler's choice per kernel, and the colour carries the bits of nu_shade_combine_fwd only if every sum
            // rounds as it does there: the fused steps below are those of that kernel's gfx950 code (its vectoriser pairs two colour
            // channels and leaves channel SS_LONE to scalar code, which fuses differently in two places); nothing else may fuse.
#pragma clang fp contract(off)
            const float occ = __builtin_fmaf(h[15], 0.5f, 0.5f);
            const float oc = fminf(fmaxf(occ, 0.f), 1.f);
            const float t = fminf(fmaxf(1.0f - nov, 0.f), 1.f);
            const float t2 = t * t, t4 = t2 * t2;
            const float sch = __builtin_fmaf(0.96f * t4, t, 0.04f);
            const float F = fminf(fmaxf(sch, 0.f), 1.f);
            const float u = fminf(fmaxf(nov, 0.f), 1.f), v = fminf(fmaxf(rho, 0.f), 1.f);
            float LA, LB;
            ss_lut(q->lut, u, v, LA, LB);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float dalb = (1.0f - met) * alb[c];
                const float diffuse = dalb * Ld[c];
                const float sa = c == SS_LONE ? __builtin_fmaf(0.04f, 1.0f - met, met * alb[c]) : __builtin_fmaf(met, alb[c], 0.04f * (1.0f - met));
                const float light = __builtin_fmaf(ind[c], oc, dir[c] * (1.0f - oc));
                const float light0 = __builtin_fmaf(ind0[c], oc, dir0[c] * (1.0f - oc));
                const float spec = __builtin_fmaf(sa, LA, LB) * light;
                const float base = __builtin_fmaf(dalb, Ld[c], spec);
                const float mixT = __builtin_fmaf(1.0f - F, refr[c], F * light0);
                const float lin = c == SS_LONE ? mixT * T + base * (1.0f - T) : __builtin_fmaf(mixT, T, base * (1.0f - T));
                if (q->color != nullptr) q->color[p * 3 + c] = q->linear ? lin : nu_linear_to_srgb(lin);
                // the validation images of field.py:751-770 before their display clamps; the two light images stay linear
                if (q->diffuse_color != nullptr) q->diffuse_color[p * 3 + c] = nu_linear_to_srgb(diffuse);
                if (q->specular_color != nullptr)
                    q->specular_color[p * 3 + c] = nu_linear_to_srgb(spec) * (1.0f - T) + F * light0 * T;
                if (q->diffuse_light != nullptr) q->diffuse_light[p * 3 + c] = Ld[c];
                if (q->specular_light != nullptr) q->specular_light[p * 3 + c] = light0;
                if (q->indirect_light != nullptr) q->indirect_light[p * 3 + c] = ind[c] * oc;
                if (q->refraction_light != nullptr) q->refraction_light[p * 3 + c] = nu_linear_to_srgb((1.0f - F) * refr[c] * T);
            }
            if (q->occ_prob != nullptr) q->occ_prob[p] = occ;
            if (q->reflection_weight != nullptr) q->reflection_weight[p] = F;
            }
        }
        if (net.raw != nullptr) {
            SS_ARGS(q, net);
            for (int idx = tid; idx < TM * SS_HD; idx += 256) {
                const int r = idx / SS_HD, c = idx - SS_HD * r;
                if (row0 + r < P) q->raw[(long long)(row0 + r) * SS_HD + c] = (c == 19) ? 0.f : hd[idx];
            }
        }
        __syncthreads();            // the tile's LDS is free for the next tile
    }
}

// Stage-1-form shading of P explicit surface points; the contract is stated at nu_surface_shade_fwd in include/nu_nerf.h.
extern "C" int nu_surface_shade_fwd(const NuShadeNet* net, const float* X, int x_ld, const float* V, int v_ld, const float* Nrm, int n_ld,
                                    const float* Mraw, int ldm, int P, int pos_freq, float refrac_exp_max, int flags, float* color,
                                    float* diffuse_color, float* specular_color, float* diffuse_light, float* specular_light,
                                    float* indirect_light, float* refraction_light, float* occ_prob, float* reflection_weight,
                                    float* enc_dbg, float* raw_dbg, hipStream_t stream) {
    if (P < 0 || !net || !X || !V || !Nrm || !Mraw) return NU_ERR_ARG;
    if (x_ld < 3 || v_ld < 3 || n_ld < 3 || ldm < 6) return NU_ERR_ARG;
    if (flags & ~NU_SHADE_LINEAR) return NU_ERR_ARG;
    if (P == 0) return NU_OK;
    const int sphere = net->sphere ? 1 : 0;
    if (!net->lut || net->ld_ol != (sphere ? 160 : 96)) return NU_ERR_ARG;
    if (pos_freq < 0 || pos_freq > 8) return NU_ERR_ARG;                 // pe + 72 <= 128 and pe + 39 <= 96
    const int pe = 3 + 6 * pos_freq, rdim = net->refrac_dim, ld_rl = net->ld_rl;
    if (rdim < 3 || rdim > pe || ld_rl < 2 * rdim || ld_rl > 160 || ld_rl % 32 != 0) return NU_ERR_ARG;
    SsNet n = {};
    int nl = 0, np = 0;
    auto push = [&](const NuLin* Pd, int Kp0, int no) -> bool {
        for (int j = 0; j < 3; ++j) {
            const NuLin& L = Pd[j];
            if (!L.Wp || !L.bias || L.N != 256 || L.Kp != (j == 0 ? Kp0 : 256)) return false;
            n.Wp[nl] = L.Wp; n.bias[nl] = L.bias; n.Kp[nl] = L.Kp;
            ++nl;
        }
        const NuLin& H = Pd[3];
        if (!H.Wp || !H.bias || H.N != no || H.Kp != 256) return false;
        n.Wh[np] = H.Wp; n.bh[np] = H.bias;
        ++np;
        return true;
    };
    for (int q = 0; q < 3; ++q)
        if (!push(net->outer_light, net->ld_ol, 3)) return NU_ERR_ARG;
    if (net->outer_light[0].K != (sphere ? 144 : 72)) return NU_ERR_ARG;
    for (int q = 0; q < 2; ++q)
        if (!push(net->inner_light, 128, 3)) return NU_ERR_ARG;
    if (net->inner_light[0].K != pe + 72) return NU_ERR_ARG;
    if (!push(net->inner_weight, 96, 1) || net->inner_weight[0].K != pe + 39) return NU_ERR_ARG;
    if (!push(net->refrac_light, ld_rl, 3) || net->refrac_light[0].K != 2 * rdim) return NU_ERR_ARG;
    n.lut = net->lut;
    n.exp_max = net->exp_max; n.refrac_exp_max = refrac_exp_max;
    n.sphere = sphere; n.ld_ol = net->ld_ol; n.pe = pe; n.rdim = rdim; n.ld_rl = ld_rl; n.linear = (flags & NU_SHADE_LINEAR) ? 1 : 0;
    n.X = X; n.V = V; n.Nrm = Nrm; n.Mraw = Mraw;
    n.x_ld = x_ld; n.v_ld = v_ld; n.n_ld = n_ld; n.ldm = ldm;
    n.color = color; n.diffuse_color = diffuse_color; n.specular_color = specular_color; n.diffuse_light = diffuse_light;
    n.specular_light = specular_light; n.indirect_light = indirect_light; n.refraction_light = refraction_light;
    n.occ_prob = occ_prob; n.reflection_weight = reflection_weight; n.enc = enc_dbg; n.raw = raw_dbg;
    const int ntiles = nu_cdiv(P, 32);
    hipLaunchKernelGGL(surface_shade_fwd_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, P);
    return nu_launch_status();
}
