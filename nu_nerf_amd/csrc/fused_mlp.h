// fused_mlp.h -- the weight-streaming MLP pipeline of the fused per-point kernels (exact fp32, no gradient), written once.
//
// Users: sdf_fused_fwd_kernel<1|2> (fused_sdf.hip), material_bake_fwd_kernel (bake.hip), light_bake_fwd_kernel (light_bake.hip),
// sdf_grad_fwd_kernel (sdf_grad.hip), sdf_jet_fwd_kernel (sdf_jet.hip), sdf_trace_kernel (sdf_trace.hip).  Each of those files keeps what
// is its own -- inputs and encodings, epilogues, where its heads go, marching logic, host entry -- and takes everything below from here,
// so a change to the pipeline is one edit that every one of them inherits, and the kernels whose rows must carry each other's bits
// (their tests compare with torch.equal) cannot drift apart.  surface_shade.hip still carries a copy of its own: see its header.
//
// Design.  A workgroup (256 threads, four waves) owns a tile of 32 TMN rows (TMN = 1 or 2) for ALL layers of a layer list.  The rows'
// activations live in LDS, k-contiguous per row, and ARE the A operand of every layer.  The weights ([N <= 256, Kp] packed fp32, Kp a
// multiple of 32) stream through two LDS stages of [256 x 32 k] in 32-deep chunks exactly as in gemm_nt2_kernel: registers -> other
// stage in the middle of a chunk, global -> registers behind it, one barrier per chunk, one memory instruction per MFMA gap -- across
// layer boundaries too, so the next layer's first chunk is already staged when a layer's epilogue runs.  Each wave computes 32 TMN rows
// x 64 of the 256 output columns on v_mfma_f32_32x32x2f32 (wave wc: columns 64 wc ..).  A layer's epilogue writes the accumulators
// straight back over the activation tile: every wave has finished reading it at the last chunk's barrier.  An accumulator register r
// of a 32-row block is row (r & 3) + 8 (r >> 2) + 4 lh, column li of its 32-column block.
// Arithmetic order is that of the layered path (same MFMA, same k order per accumulator, same head reduction as skinny_fwd_kernel):
// results are BIT-identical to it and between the kernels.
//
// LDS layout.  Row strides 260 (activations), 36 (weight stages), and the kernels' own input tiles (292, 164, 132, 100) are all
// = 4 mod 32 floats, i.e. odd multiples of 4: a ds_read_b128 is served in groups of 16 lanes over 64 banks, the 16 rows of a group have
// 16 different residues mod 16, and an odd stride / 4 maps them onto the 16 different 16-byte slots of the 256-byte bank row -- the
// fragment reads hit every slot once per 16 rows, no conflict.  An A tile is followed by FM_APAD floats (see fm_layer).
// The weight stages are 73 728 B; with a 64-row activation tile (66 576 B) that is one workgroup per CU by LDS.
#pragma once
#include "gemm.h"
#include "ide.h"

#define FM_ALD 260                 // activation row stride (floats)
#define FM_ELD 40                  // embedding row stride
#define FM_BLD 36                  // weight-stage row stride (as NT_LDS)
#define FM_BSTAGE (256 * FM_BLD)   // floats per weight stage: 256 output columns x 32 k (+ 4 pad)
#define FM_APAD 4                  // floats behind an A tile: a layer's last chunk prefetches the fragment slot behind the last row; never used

// ---- per-thread coordinates ----
struct FmThread {
    int lane, wc;                  // lane of the wave; the wave = its 64 output columns
    int li, lh;                    // MFMA operand row (lane & 31) and k half (lane >> 5)
    int c4, r0;                    // weight loader: rows r0 + 32 i (i < 8), 16-byte slot c4
    int b0_off, b1_off;            // this lane's B fragments in a weight stage (columns 64 wc + li and + 32)
    int w_off;                     // this thread's slot of row r0 in a weight stage
};
static __device__ __forceinline__ FmThread fm_thread() {
    FmThread T;
    const int tid = threadIdx.x;
    T.lane = tid & 63; T.wc = tid >> 6;
    T.li = T.lane & 31; T.lh = T.lane >> 5;
    T.c4 = tid & 7; T.r0 = tid >> 3;
    T.b0_off = (T.wc * 64 + T.li) * FM_BLD + 4 * T.lh; T.b1_off = T.b0_off + 32 * FM_BLD;
    T.w_off = T.r0 * FM_BLD + 4 * T.c4;
    return T;
}

struct FmFrag { f32x4 a0, a1, b0, b1; };      // one k-group's operand fragments of a lane (a1: the second 32-row block, TMN == 2)

// ---- the weight stream: a cursor over the 32-deep chunks of the layers Wp[0 .. nl) (row length Kp[l]) of the kernel's own argument
// block `net`, in order; past the end it stays on the last chunk.  It reads the block where it uses it and keeps no pointer into it
// (how the state is packaged decides the register allocation around the main loop: scripts/kernel_regs.py after any change here) ----
struct FmStream {
    int ld_l, ld_kt;
    const float* bp;               // this thread's slot of row r0 of the chunk at the cursor
    long long bstep;               // 32 rows further
    f32x4 rb4[8];                  // the chunk in flight
    int cur;                       // the stage the current chunk is read from

    template <class Net> __device__ __forceinline__ void set_cursor(const Net& net, const FmThread& T) {
        bp = net.Wp[ld_l] + (long long)T.r0 * net.Kp[ld_l] + 4 * T.c4 + ld_kt * 32;
        bstep = 32LL * net.Kp[ld_l];
    }
    template <class Net> __device__ __forceinline__ void advance(const Net& net, int nl, const FmThread& T) {
        // branch-free (past the end the cursor is set again to where it is): written as `if (wrap) { if (last) return; ... }` the two
        // advances of the prologue come out as two code paths whose row offsets are both hoisted out of the tile loop and held in SGPRs
        // across the main loop -- 10 to 20 SGPR spills per kernel
        const bool wrap = ld_kt + 1 == net.Kp[ld_l] / 32, last = ld_l == nl - 1;
        ld_kt = wrap ? (last ? ld_kt : 0) : ld_kt + 1;
        ld_l += wrap && !last;
        set_cursor(net, T);
    }
    __device__ __forceinline__ void load() {                   // the chunk at the cursor, global -> registers
#pragma unroll
        for (int i = 0; i < 8; ++i) rb4[i] = *reinterpret_cast<const f32x4*>(bp + i * bstep);
    }
    // prologue of a tile: chunk 0 -> stage 0, chunk 1 -> registers, barrier (both stages must be free: the barrier that ends a tile)
    template <class Net> __device__ __forceinline__ void prologue(const Net& net, int nl, float* bst, const FmThread& T) {
        ld_l = 0; ld_kt = 0;
        set_cursor(net, T);
        load();
        advance(net, nl, T);
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(&bst[T.w_off + 32 * i * FM_BLD]) = rb4[i];
        load();
        advance(net, nl, T);
        __syncthreads();
        cur = 0;
    }
    // ... and the first B fragments, which every later chunk (also across a layer boundary) fetches in its last k-group
    __device__ __forceinline__ void first_b(FmFrag& F0, const float* bst, const FmThread& T) const {
        F0.b0 = *reinterpret_cast<const f32x4*>(&bst[T.b0_off]);
        F0.b1 = *reinterpret_cast<const f32x4*>(&bst[T.b1_off]);
    }
};

// ---- one layer's main loop: acc[i][j] = rows 32 i .. of the A tile x columns 64 wc + 32 j .. of the layer's weights, nk chunks deep.
// `tile` + a0_off is this lane's first A fragment (row li, k = 4 lh; a tile of any row stride = 4 mod 32), a1_off the same of the second
// 32-row block (TMN == 2).  F0 carries the B fragments of the layer's first chunk in and those of the next layer's out.
// The schedule is hand-placed: every memory instruction sits in its own MFMA gap, pinned by a sched_barrier(0) behind each statement ----
template <int TMN> struct FmAcc { f32x16 v[TMN][2]; };
// An A fragment is read as 16 bytes DECLARED 4-byte aligned, which is what a cast of &array[i] gave these loads while every kernel had its
// own loop.  Where the offset is a compile-time expression LLVM proves 16 bytes and emits one ds_read_b128; for a per-layer tile whose
// offset comes from the argument block (light_bake, surface_shade) it emits two ds_read2_b32.  Every tile in use IS 16-byte aligned
// (bases, strides and fragment offsets are multiples of 4 floats); declaring it so is a change of its own, to be measured on its own.
typedef f32x4 fm_afrag __attribute__((aligned(4)));

template <int TMN, class Net>
static __device__ __forceinline__ FmAcc<TMN> fm_layer(FmStream& S, const Net& net, int nl, int nk, const float* tile, int a0_off, int a1_off,
                                                      float* bst, FmFrag& F0, const FmThread& T) {
    FmAcc<TMN> A;
    FmFrag F1;
#pragma unroll
    for (int i = 0; i < TMN; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) A.v[i][j][r] = 0.0f;
    // first A fragments of the layer (its tile was rewritten just before, by an epilogue or an encoder)
    F0.a0 = *reinterpret_cast<const fm_afrag*>(&tile[a0_off]);
    if constexpr (TMN == 2) F0.a1 = *reinterpret_cast<const fm_afrag*>(&tile[a1_off]);
#define FM_PIN __builtin_amdgcn_sched_barrier(0);
#define FM_M(F, e, i, j) if constexpr (i < TMN) { A.v[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a##i[e], F.b##j[e], A.v[i][j], 0, 0, 0); FM_PIN }
#define FM_RA0(F, k0, kk) F.a0 = *reinterpret_cast<const fm_afrag*>(&tile[a0_off + (k0) + (kk) * 8]); FM_PIN
#define FM_RA1(F, k0, kk) if constexpr (TMN == 2) { F.a1 = *reinterpret_cast<const fm_afrag*>(&tile[a1_off + (k0) + (kk) * 8]); FM_PIN }
#define FM_RB(F, St, kk, m) F.m = *reinterpret_cast<const f32x4*>(&(St)[T.m##_off + (kk) * 8]); FM_PIN
#define FM_W(i) *reinterpret_cast<f32x4*>(&so[T.w_off + 32 * (i) * FM_BLD]) = S.rb4[i]; FM_PIN
#define FM_L(i) S.rb4[i] = *reinterpret_cast<const f32x4*>(S.bp + (i) * S.bstep); FM_PIN
    const float* sc = &bst[S.cur * FM_BSTAGE];
    for (int kt = 0; kt < nk; ++kt) {
        float* so = &bst[(S.cur ^ 1) * FM_BSTAGE];
        const int k0 = kt * 32;
        // k-group 0: fragment reads of k-group 1
        FM_M(F0, 0, 0, 0) FM_M(F0, 0, 0, 1) FM_RA0(F1, k0, 1) FM_M(F0, 0, 1, 0) FM_M(F0, 0, 1, 1)
        FM_M(F0, 1, 0, 0) FM_M(F0, 1, 0, 1) FM_RA1(F1, k0, 1) FM_M(F0, 1, 1, 0) FM_M(F0, 1, 1, 1)
        FM_M(F0, 2, 0, 0) FM_M(F0, 2, 0, 1) FM_RB(F1, sc, 1, b0) FM_M(F0, 2, 1, 0) FM_M(F0, 2, 1, 1)
        FM_M(F0, 3, 0, 0) FM_M(F0, 3, 0, 1) FM_RB(F1, sc, 1, b1) FM_M(F0, 3, 1, 0) FM_M(F0, 3, 1, 1)
        // k-group 1: the next weight chunk registers -> other stage; fragment reads of k-group 2
        FM_M(F1, 0, 0, 0) FM_W(0) FM_M(F1, 0, 0, 1) FM_RA0(F0, k0, 2) FM_M(F1, 0, 1, 0) FM_W(1) FM_M(F1, 0, 1, 1)
        FM_M(F1, 1, 0, 0) FM_W(2) FM_M(F1, 1, 0, 1) FM_RA1(F0, k0, 2) FM_M(F1, 1, 1, 0) FM_W(3) FM_M(F1, 1, 1, 1)
        FM_M(F1, 2, 0, 0) FM_W(4) FM_M(F1, 2, 0, 1) FM_RB(F0, sc, 2, b0) FM_M(F1, 2, 1, 0) FM_W(5) FM_M(F1, 2, 1, 1)
        FM_M(F1, 3, 0, 0) FM_W(6) FM_M(F1, 3, 0, 1) FM_RB(F0, sc, 2, b1) FM_M(F1, 3, 1, 0) FM_W(7) FM_M(F1, 3, 1, 1)
        // k-group 2: the chunk after that global -> registers; fragment reads of k-group 3
        FM_M(F0, 0, 0, 0) FM_L(0) FM_M(F0, 0, 0, 1) FM_RA0(F1, k0, 3) FM_M(F0, 0, 1, 0) FM_L(1) FM_M(F0, 0, 1, 1)
        FM_M(F0, 1, 0, 0) FM_L(2) FM_M(F0, 1, 0, 1) FM_RA1(F1, k0, 3) FM_M(F0, 1, 1, 0) FM_L(3) FM_M(F0, 1, 1, 1)
        FM_M(F0, 2, 0, 0) FM_L(4) FM_M(F0, 2, 0, 1) FM_RB(F1, sc, 3, b0) FM_M(F0, 2, 1, 0) FM_L(5) FM_M(F0, 2, 1, 1)
        FM_M(F0, 3, 0, 0) FM_L(6) FM_M(F0, 3, 0, 1) FM_RB(F1, sc, 3, b1) FM_M(F0, 3, 1, 0) FM_L(7) FM_M(F0, 3, 1, 1)
        S.advance(net, nl, T);
        __syncthreads();        // the other stage is complete; every wave holds its last fragments of this chunk
        // k-group 3: first fragments of the next chunk (weights: the other stage, also across a layer boundary).  The A reads are
        // unconditional -- a branch around them would make hipcc drain the weight loads at the join -- and after a layer's last chunk
        // they return bytes nobody uses, from the FM_APAD floats behind the tile at most (the next layer re-reads its first fragments
        // behind the epilogue)
        FM_M(F1, 0, 0, 0) FM_M(F1, 0, 0, 1) FM_RA0(F0, k0 + 32, 0) FM_M(F1, 0, 1, 0) FM_M(F1, 0, 1, 1)
        FM_M(F1, 1, 0, 0) FM_M(F1, 1, 0, 1) FM_RA1(F0, k0 + 32, 0) FM_M(F1, 1, 1, 0) FM_M(F1, 1, 1, 1)
        FM_M(F1, 2, 0, 0) FM_M(F1, 2, 0, 1) FM_RB(F0, so, 0, b0) FM_M(F1, 2, 1, 0) FM_M(F1, 2, 1, 1)
        FM_M(F1, 3, 0, 0) FM_M(F1, 3, 0, 1) FM_RB(F0, so, 0, b1) FM_M(F1, 3, 1, 0) FM_M(F1, 3, 1, 1)
        S.cur ^= 1;
        sc = so;
    }
#undef FM_M
#undef FM_RA0
#undef FM_RA1
#undef FM_RB
#undef FM_W
#undef FM_L
#undef FM_PIN
    return A;
}

// ---- get_embedder(6, 3): column col < 39 of the positional embedding of x (nu_embed_col of the encoding kernels) ----
static __device__ __forceinline__ float fm_embed_col(const float* x, int col) { return nu_embed_col(x, 3, col); }

// jet component j of column col (0 for col >= 39) at x: 0 the value (the expression of fm_embed_col), 1..3 d/dx, d/dy, d/dz (2^k cos /
// -2^k sin on the column's own axis), 4..6 d2/dxx, yy, zz (-4^k sin / -4^k cos), 7..9 the mixed second derivatives (0).  ORDER = the
// highest order asked for (1: j <= 3, 2: j <= 9), so that a first-order caller carries no second-order code
template <int ORDER>
static __device__ inline float fm_embed_jet(const float* x, int col, int j) {
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
    if constexpr (ORDER >= 2) {
        if (j == 4 + c) return r >= 3 ? -(fk * fk) * cosf(a) : -(fk * fk) * sinf(a);
    }
    return 0.f;
}

// ---- the SDF network's skip: layer 4's input is [h4 (217) | embedding (39)] (the 1 / sqrt 2 is folded into the packed weights); the
// tile's embedding rows, kept in LDS, go back in behind layer 3's epilogue ----
static __device__ __forceinline__ void fm_skip_reinsert(float* act, const float* emb, int rows) {
    for (int idx = threadIdx.x; idx < rows * 39; idx += 256) {
        const int r = idx / 39, c = idx - r * 39;
        act[r * FM_ALD + 217 + c] = emb[r * FM_ELD + c];
    }
}

// ---- a 256-wide head on one row, by one wave: the arithmetic of skinny_fwd_kernel<NO, 256> (16 bytes per lane -- w = the head row's
// floats 4 lane .. --, xor-shuffle reduction, nothing contracted).  Every lane returns the sum; the bias is the caller's ----
static __device__ __forceinline__ float fm_row_dot(const float* row, const f32x4& w, int lane) {
#pragma clang fp contract(off)
    const f32x4 h = *reinterpret_cast<const f32x4*>(&row[4 * lane]);
    float a = 0.f;
    a += (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}
