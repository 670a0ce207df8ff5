// wgrad_rm.h -- what gemm_tn.hip (dispatch) and wgrad_rm.hip (the row-major-staged weight-gradient kernels) share.
#pragma once
#include "gemm.h"

// Several weight-gradient problems in ONE launch: the (tile, split) blocks of problem i are the linear block ids
// [blk0[i], blk0[i + 1]), tile fastest.  Each problem keeps its own operands, extents, split count and slab (NuGemmTN).
#define NU_TN_BATCH_MAX 16
struct NuGemmTNBatch {
    NuGemmTN p[NU_TN_BATCH_MAX];
    int blk0[NU_TN_BATCH_MAX + 1];
    int n, pad_;
};
#ifdef __HIPCC__
// which problem a block of a batched launch belongs to, and its (tile, split) there; `tiles` = output tiles of that problem
static __device__ __forceinline__ int tn_batch_decode(const NuGemmTNBatch& b, int tile_edge, int& bx, int& split) {
    int pi = 0;
    for (int i = 1; i < b.n; ++i) pi = ((int)blockIdx.x >= b.blk0[i]) ? i : pi;
    const int tiles = ((b.p[pi].N1 + tile_edge - 1) / tile_edge) * ((b.p[pi].N2 + tile_edge - 1) / tile_edge);
    const int local = (int)blockIdx.x - b.blk0[pi];
    split = local / tiles;
    bx = local - split * tiles;
    return pi;
}
#endif

// Can the row-major kernels take this exact-fp32 problem?  Every operand base (each group's too) on a 16-byte boundary, rows a
// whole number of quads, every operand below 4 GiB (32-bit byte offsets).  The shape rule (nu_tn_big_tile) stays with the caller.
bool nu_wgrad_rm_ok(const NuGemmTN& g);
// one problem, grid (tiles, S, groups); N1 and N2 multiples of 256
int nu_wgrad_rm256_launch(const NuGemmTN& g, hipStream_t stream);
// a batch of such problems (groups already unrolled), `blocks` = b.blk0[b.n]
int nu_wgrad_rm256_launch_batch(const NuGemmTNBatch& b, int blocks, hipStream_t stream);
// the same on 128 x 128 tiles: any N1, N2
int nu_wgrad_rm128_launch(const NuGemmTN& g, hipStream_t stream);
int nu_wgrad_rm128_launch_batch(const NuGemmTNBatch& b, int blocks, hipStream_t stream);
