// env_prefilter.hip -- prefiltering of an environment into the roughness pyramid of the split-sum appearance model (gfx950).
//
// A zonal kernel regression on the sphere: for a weighted point set (s_j, w_j, rgb_j), j < M, query directions d_i, i < N, and L lobes
//     out[l, i] = sum_j w_j f_l(c_ij) rgb_j / sum_j w_j f_l(c_ij),        c_ij = d_i . s_j
// with f_l a function of c alone (include/nu_nerf.h: cosine, GGX at N = V = R, von Mises-Fisher).  The quotient normalises itself: a
// constant map comes back as the constant at any resolution, no lobe needs its analytic normaliser and the poles of a lat-long source
// need no special case (w = sin theta > 0 at texel centres).
//
// Shape: N-body.  One query per thread, 256 queries per workgroup; the source is streamed through LDS in tiles of NU_PF_TILE entries
// (direction and w * (r, g, b, 1), two 16-byte entries that all lanes read at the same address: a broadcast, no bank conflict).  c is
// formed once per pair and serves every lobe.  A tile's contribution is summed from zero in source order and then added to the
// running total, tile after tile: every sum has ONE order, which also keeps the fp32 error of a long sum small.  No atomics.
//   * A query's arithmetic does not depend on N, on its position, on its neighbours or on the other lobes of the call: the operations of
//     a (pair, lobe) are written once (pf_lobe), FMA contraction is off and the fused operations are spelled out.
//   * When the query blocks alone cannot fill the chip the tile range is split over gridDim.y workgroups; each writes its tiles'
//     contributions to the workspace and pf_reduce_kernel folds them in tile order -- the additions of the unsplit kernel, the same bits.
// No trigonometry here: the host builds the source table (environment.latlong_dirs, w = sin theta, in float64).
#include "nu_common.h"

#pragma clang fp contract(off)

#define NU_PF_BLOCK 256
#define NU_PF_TILE 256               // source entries per LDS tile: 8 KiB
#define NU_PF_JB 8                   // pairs whose lobe kind is decided together (the kind is wave-uniform: a scalar branch per NU_PF_JB pairs)
#define NU_PF_WS_MAX (256LL << 20)   // the split is not taken when its workspace would exceed this

struct PfLobes {                     // kernel argument: per lobe its kind and two constants made on the host
    int kind[NU_ENV_MAX_LOBES];
    float a[NU_ENV_MAX_LOBES];       // GGX: alpha^2            vMF: kappa * log2(e)
    float b[NU_ENV_MAX_LOBES];       // GGX: (1 - alpha^2) / 2  vMF: unused
    float k[NU_ENV_MAX_LOBES];       // GGX: alpha^2 / pi
};

// One (pair, lobe): acc += f(c) * (w r, w g, w b, w).  u = 1 - c (exact for c >= 1/2: the subtraction that matters for a narrow lobe).
static __device__ inline void pf_lobe(int kind, float a, float b, float k, float c, float u, const float4 s, float* acc) {
    float f;
    if (kind == NU_LOBE_COSINE) {
        f = fmaxf(c, 0.0f);
    } else if (kind == NU_LOBE_GGX) {
        // NoH^2 = (1 + c) / 2: NoH^2 (alpha^2 - 1) + 1 = alpha^2 + (1 - alpha^2) (1 - c) / 2, free of cancellation at the peak
        const float t = __builtin_fmaf(b, u, a);
        const float r = __builtin_amdgcn_rcpf(t);
        f = (fmaxf(c, 0.0f) * k) * (r * r);
    } else {
        f = __builtin_amdgcn_exp2f(-a * u);
    }
    acc[0] = __builtin_fmaf(f, s.x, acc[0]);
    acc[1] = __builtin_fmaf(f, s.y, acc[1]);
    acc[2] = __builtin_fmaf(f, s.z, acc[2]);
    acc[3] = __builtin_fmaf(f, s.w, acc[3]);
}

// The contribution of one staged tile (cnt entries, padded with zero weights to a multiple of NU_PF_JB) to the query d: part[l] from zero.
template <int NL>
static __device__ inline void pf_tile(const PfLobes& lobes, const float4* __restrict__ sd, const float4* __restrict__ sc, int cnt,
                                      float d0, float d1, float d2, float (*part)[4]) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
        for (int q = 0; q < 4; ++q) part[l][q] = 0.0f;
    for (int j = 0; j < cnt; j += NU_PF_JB) {
        float c[NU_PF_JB], u[NU_PF_JB];
        float4 s[NU_PF_JB];
#pragma unroll
        for (int e = 0; e < NU_PF_JB; ++e) {
            const float4 dir = sd[j + e];
            s[e] = sc[j + e];
            c[e] = __builtin_fmaf(d2, dir.z, __builtin_fmaf(d1, dir.y, d0 * dir.x));
            u[e] = 1.0f - c[e];
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int kind = lobes.kind[l];
            const float a = lobes.a[l], b = lobes.b[l], k = lobes.k[l];
            if (kind == NU_LOBE_COSINE) {
#pragma unroll
                for (int e = 0; e < NU_PF_JB; ++e) pf_lobe(NU_LOBE_COSINE, a, b, k, c[e], u[e], s[e], part[l]);
            } else if (kind == NU_LOBE_GGX) {
#pragma unroll
                for (int e = 0; e < NU_PF_JB; ++e) pf_lobe(NU_LOBE_GGX, a, b, k, c[e], u[e], s[e], part[l]);
            } else {
#pragma unroll
                for (int e = 0; e < NU_PF_JB; ++e) pf_lobe(NU_LOBE_VMF, a, b, k, c[e], u[e], s[e], part[l]);
            }
        }
    }
}

// grid (query blocks, splits).  SPLIT = false: gridDim.y = 1, out [NL, N, 4] = the quotient.  SPLIT = true: split y takes the tiles
// [y * tiles_per, (y + 1) * tiles_per) and writes ws [n_tiles, NL, N, 4], each tile's contribution.
template <int NL, bool SPLIT>
__global__ __launch_bounds__(NU_PF_BLOCK) void pf_kernel(const float4* __restrict__ src_dir, const float4* __restrict__ src_rgb, int M,
                                                         const float* __restrict__ dirs, int N, PfLobes lobes, int n_tiles,
                                                         int tiles_per, float4* __restrict__ out) {
    __shared__ float4 sd[NU_PF_TILE];
    __shared__ float4 sc[NU_PF_TILE];
    const int i = blockIdx.x * NU_PF_BLOCK + threadIdx.x;
    const bool live = i < N;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    if (live) { d0 = dirs[i * 3LL]; d1 = dirs[i * 3LL + 1]; d2 = dirs[i * 3LL + 2]; }
    float total[NL][4], part[NL][4];
#pragma unroll
    for (int l = 0; l < NL; ++l)
        for (int q = 0; q < 4; ++q) total[l][q] = 0.0f;
    const int t0 = SPLIT ? blockIdx.y * tiles_per : 0;
    const int t1 = SPLIT ? min(t0 + tiles_per, n_tiles) : n_tiles;
    for (int t = t0; t < t1; ++t) {
        const int base = t * NU_PF_TILE;
        const int cnt = min(NU_PF_TILE, M - base);
        __syncthreads();                                     // the previous tile has been read by every wave
        {
            const int j = threadIdx.x;                       // NU_PF_BLOCK == NU_PF_TILE: one entry per thread
            float4 dir = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rgb = dir;
            if (j < cnt) {
                dir = src_dir[base + j];
                rgb = src_rgb[base + j];
            }
            const float4 col = make_float4(dir.w * rgb.x, dir.w * rgb.y, dir.w * rgb.z, dir.w);
            sd[j] = dir;                                     // entries past cnt: weight 0, they add +0 to every sum
            sc[j] = col;
        }
        __syncthreads();
        pf_tile<NL>(lobes, sd, sc, nu_rup(cnt, NU_PF_JB), d0, d1, d2, part);
        if (SPLIT) {
            if (live) {
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    const float4 p = {part[l][0], part[l][1], part[l][2], part[l][3]};
                    out[((long long)t * NL + l) * N + i] = p;
                }
            }
        } else {
#pragma unroll
            for (int l = 0; l < NL; ++l)
                for (int q = 0; q < 4; ++q) total[l][q] = total[l][q] + part[l][q];
        }
    }
    if (!SPLIT && live) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const float4 o = {total[l][0] / total[l][3], total[l][1] / total[l][3], total[l][2] / total[l][3], 1.0f};
            out[(long long)l * N + i] = o;
        }
    }
}

// Second pass of the split: one thread per (lobe, query) folds the tiles' contributions in tile order, as the unsplit kernel does.
__global__ __launch_bounds__(256) void pf_reduce_kernel(const float4* __restrict__ ws, int n_tiles, long long LN, float4* __restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= LN) return;
    float total[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < n_tiles; ++t) {
        const float4 p = ws[(long long)t * LN + e];
        total[0] = total[0] + p.x; total[1] = total[1] + p.y; total[2] = total[2] + p.z; total[3] = total[3] + p.w;
    }
    const float4 o = {total[0] / total[3], total[1] / total[3], total[2] / total[3], 1.0f};
    out[e] = o;
}

// The split rule, a pure function of the counts: how many workgroups share the tile range (1 = no split, no workspace).
static int pf_splits(int N, int M, int L) {
    if (N <= 0 || M <= 0 || L <= 0) return 1;
    const int blocks = nu_cdiv(N, NU_PF_BLOCK), n_tiles = nu_cdiv(M, NU_PF_TILE);
    if (blocks >= 128 || n_tiles < 2) return 1;              // half the chip's CUs have a workgroup already, or there is nothing to split
    if ((long long)n_tiles * L * N * 16 > NU_PF_WS_MAX) return 1;
    return min(n_tiles, nu_cdiv(512, blocks));
}

extern "C" long long nu_env_prefilter_workspace_bytes(int N, int M, int L) {
    if (N < 0 || M < 0 || L < 1 || L > NU_ENV_MAX_LOBES) return NU_ERR_ARG;
    return pf_splits(N, M, L) > 1 ? (long long)nu_cdiv(M, NU_PF_TILE) * L * N * 16 : 0;
}

template <int NL>
static void pf_launch(const float* src_dir, const float* src_rgb, int M, const float* dirs, int N, const PfLobes& lobes, float* out, void* ws,
                      hipStream_t stream) {
    const int blocks = nu_cdiv(N, NU_PF_BLOCK), n_tiles = nu_cdiv(M, NU_PF_TILE), splits = pf_splits(N, M, NL);
    if (splits == 1) {
        hipLaunchKernelGGL((pf_kernel<NL, false>), dim3(blocks), dim3(NU_PF_BLOCK), 0, stream, (const float4*)src_dir, (const float4*)src_rgb, M,
                           dirs, N, lobes, n_tiles, n_tiles, (float4*)out);
        return;
    }
    const int tiles_per = nu_cdiv(n_tiles, splits);
    hipLaunchKernelGGL((pf_kernel<NL, true>), dim3(blocks, nu_cdiv(n_tiles, tiles_per)), dim3(NU_PF_BLOCK), 0, stream, (const float4*)src_dir,
                       (const float4*)src_rgb, M, dirs, N, lobes, n_tiles, tiles_per, (float4*)ws);
    const long long LN = (long long)NL * N;
    hipLaunchKernelGGL(pf_reduce_kernel, dim3((unsigned)nu_cdivl(LN, 256)), dim3(256), 0, stream, (const float4*)ws, n_tiles, LN, (float4*)out);
}

extern "C" int nu_env_prefilter(const float* src_dir, const float* src_rgb, int M, const float* dirs, int N, const int* lobe_kind,
                                const float* lobe_param, int L, float* out, void* ws, long long ws_bytes, hipStream_t stream) {
    if (N < 0 || M < 0 || L < 1 || L > NU_ENV_MAX_LOBES || !lobe_kind || !lobe_param) return NU_ERR_ARG;
    if ((M > 0 && (!src_dir || !src_rgb)) || (N > 0 && (!dirs || !out))) return NU_ERR_ARG;       // an empty array may have no address
    PfLobes lobes = {};
    for (int l = 0; l < L; ++l) {
        const int kind = lobe_kind[l];
        const double p = lobe_param[l];
        lobes.kind[l] = kind;
        if (kind == NU_LOBE_COSINE) continue;
        if (!(p > 0.0) || !(p < 3e38)) return NU_ERR_ARG;
        if (kind == NU_LOBE_GGX) {
            lobes.a[l] = (float)(p * p);
            lobes.b[l] = (float)((1.0 - p * p) * 0.5);
            lobes.k[l] = (float)(p * p / 3.14159265358979323846);
        } else if (kind == NU_LOBE_VMF) {
            lobes.a[l] = (float)(p * 1.4426950408889634);
        } else {
            return NU_ERR_ARG;
        }
    }
    if (N == 0 || M == 0) return NU_OK;
    const long long need = nu_env_prefilter_workspace_bytes(N, M, L);
    if (need > 0 && (!ws || ws_bytes < need)) return NU_ERR_WORKSPACE;
    switch (L) {
#define NU_PF_CASE(n) case n: pf_launch<n>(src_dir, src_rgb, M, dirs, N, lobes, out, ws, stream); break;
        NU_PF_CASE(1) NU_PF_CASE(2) NU_PF_CASE(3) NU_PF_CASE(4) NU_PF_CASE(5) NU_PF_CASE(6) NU_PF_CASE(7) NU_PF_CASE(8)
        NU_PF_CASE(9) NU_PF_CASE(10) NU_PF_CASE(11) NU_PF_CASE(12) NU_PF_CASE(13) NU_PF_CASE(14) NU_PF_CASE(15) NU_PF_CASE(16)
#undef NU_PF_CASE
    }
    return nu_launch_status();
}
