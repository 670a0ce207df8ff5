// mlp.hip -- support kernels around the MFMA GEMMs: weight packing (weight-norm folded), gradient
// unpacking (weight-norm chain rule), skinny output heads (N <= 8), column sums, row scaling.
//
// Reference semantics restated here:
//   nn.utils.weight_norm (legacy, dim=0)  W = v * (g / ||v||_row)        network/field.py:121-122, :386-393
//   the 1-, 3-wide output layers of make_predictor / NeRFNetwork heads     network/field.py:393, :260-261
#include "gemm.h"

// ------------------------------------------------------------------------------------------------
// pack / unpack
// ------------------------------------------------------------------------------------------------
// NuPackDesc: see include/nu_nerf.h

static __device__ inline int nu_find_desc(const NuPackDesc* __restrict__ d, int nd, int row) {
    int lo = 0, hi = nd - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (d[mid].row_begin <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(64) void pack_kernel(const NuPackDesc* __restrict__ descs, int nd) {
    const int row = blockIdx.x;
    const int lane = threadIdx.x;
    const NuPackDesc d = descs[nu_find_desc(descs, nd, row)];
    const int n = row - d.row_begin;
    const float* __restrict__ v = d.v + (long long)n * d.K;
    float s = d.scale;
    if (d.g) {
        float ss = 0.f;
        for (int k = lane; k < d.K; k += 64) ss += v[k] * v[k];
        ss = nu_wave_sum(ss);
        s *= d.g[n] / sqrtf(ss);
    }
    for (int k = lane; k < d.K; k += 64) {
        const int kp = (d.colmap ? d.colmap[k] : k) + d.col_off;
        const float w = v[k] * s;
        d.Wp[(long long)n * d.Kp + kp] = w;
        if (d.WpT) d.WpT[(long long)kp * d.ldT + n] = w;
        if (d.planes == 3) {
            // exact three-way split (nu_split3's arithmetic), layout of NuGemmNT.B6
#pragma clang fp contract(off)
            const __bf16 h1 = (__bf16)w;
            const float r1 = w - (float)h1;
            const __bf16 h2 = (__bf16)r1;
            const __bf16 h3 = (__bf16)(r1 - (float)h2);
            auto at = [](void* tbl, int row, int col, int ld) -> __bf16* {
                return reinterpret_cast<__bf16*>(tbl) + ((long long)(row >> 8) * (ld >> 4) + (col >> 4)) * 12288 + (row & 255) * 48 + ((col & 15) ^ (row & 8));
            };
            if (d.Wp16) {
                __bf16* q = at(d.Wp16, d.w6_row0 + n, kp, d.w6_ld);
                q[0] = h1; q[16] = h2; q[32] = h3;
            }
            if (d.WpT16) {
                __bf16* q = at(d.WpT16, d.t6_row0 + kp, d.t6_col0 + n, d.t6_ld);
                q[0] = h1; q[16] = h2; q[32] = h3;
            }
        } else {
            if (d.Wp16) reinterpret_cast<__bf16*>(d.Wp16)[(long long)n * d.Kp + kp] = (__bf16)w;
            if (d.WpT16) reinterpret_cast<__bf16*>(d.WpT16)[(long long)kp * d.ldT + n] = (__bf16)w;
        }
    }
    if (lane == 0 && d.bias_p) d.bias_p[n] = d.bias[n];
}

__global__ __launch_bounds__(64) void unpack_kernel(const NuPackDesc* __restrict__ descs, int nd,
                                                    float* __restrict__ flat, int row0) {
    const int row = blockIdx.x + row0;
    const int lane = threadIdx.x;
    const NuPackDesc d = descs[nu_find_desc(descs, nd, row)];
    const int n = row - d.row_begin;
    const float* __restrict__ v = d.v + (long long)n * d.K;
    const float* __restrict__ dw = d.dWp + (long long)n * d.ldd;
    float* __restrict__ dv = flat + d.dv_off + (long long)n * d.K;
    if (d.g) {
        float ss = 0.f, dot = 0.f;
        for (int k = lane; k < d.K; k += 64) {
            const int kp = (d.colmap ? d.colmap[k] : k) + d.col_off;
            const float vv = v[k];
            ss += vv * vv;
            dot += d.scale * dw[kp] * vv;
        }
        ss = nu_wave_sum(ss);
        dot = nu_wave_sum(dot);
        const float norm = sqrtf(ss);
        const float gn = d.g[n] / norm;
        const float c2 = gn * dot / ss;
        for (int k = lane; k < d.K; k += 64) {
            const int kp = (d.colmap ? d.colmap[k] : k) + d.col_off;
            dv[k] = gn * d.scale * dw[kp] - c2 * v[k];
        }
        if (lane == 0) flat[d.dg_off + n] = dot / norm;
    } else {
        for (int k = lane; k < d.K; k += 64) {
            const int kp = (d.colmap ? d.colmap[k] : k) + d.col_off;
            dv[k] = d.scale * dw[kp];
        }
    }
}

extern "C" int nu_pack_layers(const void* descs, int ndesc, int total_rows, hipStream_t stream) {
    if (total_rows <= 0) return NU_OK;
    hipLaunchKernelGGL(pack_kernel, dim3(total_rows), dim3(64), 0, stream, (const NuPackDesc*)descs, ndesc);
    return nu_launch_status();
}
extern "C" int nu_unpack_grads(const void* descs, int ndesc, int total_rows, float* flat_grads, hipStream_t stream) {
    if (total_rows <= 0) return NU_OK;
    hipLaunchKernelGGL(unpack_kernel, dim3(total_rows), dim3(64), 0, stream, (const NuPackDesc*)descs, ndesc, flat_grads, 0);
    return nu_launch_status();
}
extern "C" int nu_unpack_grads_range(const void* descs, int ndesc, int row0, int nrows, float* flat_grads, hipStream_t stream) {
    if (nrows <= 0) return NU_OK;
    if (row0 < 0) return NU_ERR_ARG;
    hipLaunchKernelGGL(unpack_kernel, dim3(nrows), dim3(64), 0, stream, (const NuPackDesc*)descs, ndesc, flat_grads, row0);
    return nu_launch_status();
}
extern "C" int nu_pack_desc_size() { return (int)sizeof(NuPackDesc); }
extern "C" int nu_reduce_desc_size() { return (int)sizeof(NuReduceDesc); }

// ------------------------------------------------------------------------------------------------
// skinny heads: out[p, j] = sum_k H[p, k] * Ws[j, k] + b[j],  j < NO <= 8.   HBM-bound (reads H once).
// ------------------------------------------------------------------------------------------------
// H16 (bf16-storage mode, NuOpCtx.h16): the hidden rows H -- and the dH the backward writes -- are __bf16 behind the float*
// (leading dimensions in elements); arithmetic stays fp32
template <bool H16> static __device__ __forceinline__ f32x4 sk_ld4(const float* base, long long idx) {
    if (H16) {
        const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(base) + idx * 2);
        f32x4 o;
        o[0] = __uint_as_float(r.x << 16); o[1] = __uint_as_float(r.x & 0xffff0000u);
        o[2] = __uint_as_float(r.y << 16); o[3] = __uint_as_float(r.y & 0xffff0000u);
        return o;
    }
    return *reinterpret_cast<const f32x4*>(base + idx);
}
template <bool H16> static __device__ __forceinline__ void sk_st4(float* base, long long idx, f32x4 v) {
    if (H16) *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(base) + idx * 2) = nu_to_bf16x4(v);
    else *reinterpret_cast<f32x4*>(base + idx) = v;
}

// One wave per row (K = 128: two rows per wave), head weights held in registers, two rows in flight per wave.
template <int NO, int K, bool H16 = false>
__global__ __launch_bounds__(256) void skinny_fwd_kernel(const float* __restrict__ H, int ldh, int P,
                                                         const float* __restrict__ Ws, int ldw,
                                                         const float* __restrict__ b, float* __restrict__ out, int ldo) {
    constexpr int KQ = K >= 256 ? K / 256 : 1;
    constexpr int RPW = K >= 256 ? 1 : 2;
    constexpr int LPR = 64 / RPW;
    const int lane = threadIdx.x & 63;
    const int sub = lane / LPR, ln = lane % LPR;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwave = (gridDim.x * blockDim.x) >> 6;
    f32x4 w[NO][KQ];
    float bj[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        bj[j] = b ? b[j] : 0.f;
#pragma unroll
        for (int t = 0; t < KQ; ++t) w[j][t] = *reinterpret_cast<const f32x4*>(Ws + (long long)j * ldw + 4 * ln + 256 * t);
    }
    // the row arithmetic is inlined three times (two rows in flight + tail): contraction off, so that a row's result does
    // not depend on which copy ran it (ray-independence is tested bit-exactly)
    auto finish = [&](int p, const f32x4* h) {
#pragma clang fp contract(off)
        float acc[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            float a = 0.f;
#pragma unroll
            for (int t = 0; t < KQ; ++t) a += (h[t][0] * w[j][t][0] + h[t][1] * w[j][t][1]) + (h[t][2] * w[j][t][2] + h[t][3] * w[j][t][3]);
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) a += __shfl_xor(a, o);
            acc[j] = a;
        }
        if (ln == 0) {
#pragma unroll
            for (int j = 0; j < NO; ++j) out[(long long)p * ldo + j] = acc[j] + bj[j];
        }
    };
    const int step = nwave * RPW;
    int p = wave * RPW + sub;
    for (; p + step < P; p += 2 * step) {
        f32x4 ha[KQ], hb[KQ];
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            ha[t] = sk_ld4<H16>(H, (long long)p * ldh + 4 * ln + 256 * t);
            hb[t] = sk_ld4<H16>(H, (long long)(p + step) * ldh + 4 * ln + 256 * t);
        }
        finish(p, ha);
        finish(p + step, hb);
    }
    if (p < P) {
        f32x4 ha[KQ];
#pragma unroll
        for (int t = 0; t < KQ; ++t) ha[t] = sk_ld4<H16>(H, (long long)p * ldh + 4 * ln + 256 * t);
        finish(p, ha);
    }
}

static int skinny_fwd_launch(const float* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO, float* out, int ldo,
                             bool h16, hipStream_t stream);
extern "C" int nu_skinny_fwd(const float* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO,
                             float* out, int ldo, hipStream_t stream) {
    return skinny_fwd_launch(H, ldh, P, K, Ws, ldw, b, NO, out, ldo, false, stream);
}
// H is __bf16 [P, ldh] (bf16-storage mode)
extern "C" int nu_skinny_fwd_h16(const void* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO,
                                 float* out, int ldo, hipStream_t stream) {
    return skinny_fwd_launch(static_cast<const float*>(H), ldh, P, K, Ws, ldw, b, NO, out, ldo, true, stream);
}
static int skinny_fwd_launch(const float* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO, float* out, int ldo,
                             bool h16, hipStream_t stream) {
    if (P <= 0) return NU_OK;
    if ((K & 3) || (ldh & 3) || (ldw & 3)) return NU_ERR_ARG;
    const int blocks = nu_cdiv(P, 8) < 2048 ? nu_cdiv(P, 8) : 2048;
    dim3 grid(blocks), block(256);
#define NU_CASE(n, k) if (NO == n && K == k) { if (h16) hipLaunchKernelGGL((skinny_fwd_kernel<n, k, true>), grid, block, 0, stream, H, ldh, P, Ws, ldw, b, out, ldo); \
                                               else hipLaunchKernelGGL((skinny_fwd_kernel<n, k, false>), grid, block, 0, stream, H, ldh, P, Ws, ldw, b, out, ldo); \
                                               return nu_launch_status(); }
    NU_CASE(1, 128) NU_CASE(2, 128) NU_CASE(3, 128) NU_CASE(4, 128)
    NU_CASE(1, 256) NU_CASE(2, 256) NU_CASE(3, 256) NU_CASE(4, 256)
    NU_CASE(6, 1024)
#undef NU_CASE
    return NU_ERR_ARG;
}

// backward of a skinny head (feeding a ReLU hidden layer):
//   dH[p,k]   = (sum_j dy[p,j] Ws[j,k]) * (relu_mask ? H[p,k] > 0 : 1)      (written, or added to dH if accumulate)
//   dWs[j,k]  = sum_p dy[p,j] H[p,k]      (per-block partial -> slab[blk][j][k])
//   db[j]     = sum_p dy[p,j]             (per-block partial -> bslab[blk][j])
// One wave per row of a K-column slice (K = 256: 16 B per lane; K = 128: two rows per wave, 32 lanes each; a wider head
// is cut into 256-column slices along grid.y -- dH and dWs are column-local), four waves per block on interleaved
// rows, two rows in flight per wave; the four waves' weight-gradient partials are summed through LDS in a fixed order
// before the block writes its slab.
template <int NO, int K, bool H16 = false>
__global__ __launch_bounds__(256) void skinny_bwd_kernel(const float* __restrict__ dy, int ldy,
                                                         const float* __restrict__ H, int ldh, int P,
                                                         const float* __restrict__ Ws, int ldw, float* __restrict__ dH,
                                                         int lddh, int relu_mask, int accumulate,
                                                         float* __restrict__ slab, float* __restrict__ bslab, int Ktot) {
    constexpr int KQ = 1;                               // float4 chunks per lane
    constexpr int RPW = K >= 256 ? 1 : 2;               // rows per wave per pass
    const int cb = blockIdx.y * K;                      // first column of this block's slice
    Ws += cb;                                           // (H and dH: the column offset goes into the element index)
    constexpr int LPR = 64 / RPW;                       // lanes per row
    __shared__ float red[4 * K];
    __shared__ float bred[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane / LPR, ln = lane % LPR;
    int rows_per = (P + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * rows_per;
    int p1 = p0 + rows_per;
    p1 = p1 < P ? p1 : P;
    f32x4 w[NO][KQ], acc[NO][KQ];
    float bacc[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        bacc[j] = 0.f;
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            w[j][t] = *reinterpret_cast<const f32x4*>(Ws + (long long)j * ldw + 4 * ln + 256 * t);
            acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    constexpr int STEP = 4 * RPW;                       // rows the block advances per pass
    auto row_body = [&](int p, const f32x4* h) {
#pragma clang fp contract(off)      // inlined three times: same rounding in every copy
        float g[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            g[j] = dy[(long long)p * ldy + j];
            bacc[j] += g[j];
        }
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                d += g[j] * w[j][t];
                acc[j][t] += g[j] * h[t];
            }
            if (relu_mask) {
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = h[t][e] > 0.f ? d[e] : 0.f;
            }
            const long long qi = (long long)p * lddh + cb + 4 * ln + 256 * t;
            if (accumulate) d += sk_ld4<H16>(dH, qi);
            sk_st4<H16>(dH, qi, d);
        }
    };
    int p = p0 + wave * RPW + sub;
    for (; p + STEP < p1; p += 2 * STEP) {              // two rows in flight
        f32x4 ha[KQ], hb[KQ];
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            ha[t] = sk_ld4<H16>(H, (long long)p * ldh + cb + 4 * ln + 256 * t);
            hb[t] = sk_ld4<H16>(H, (long long)(p + STEP) * ldh + cb + 4 * ln + 256 * t);
        }
        row_body(p, ha);
        row_body(p + STEP, hb);
    }
    for (; p < p1; p += STEP) {
        f32x4 ha[KQ];
#pragma unroll
        for (int t = 0; t < KQ; ++t) ha[t] = sk_ld4<H16>(H, (long long)p * ldh + cb + 4 * ln + 256 * t);
        row_body(p, ha);
    }
    // block reduction, one output row j at a time: red[wave][k] (for K = 128 the two half-waves add first)
#pragma unroll
    for (int j = 0; j < NO; ++j) {
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            f32x4 v = acc[j][t];
            if (RPW == 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], 32);
            }
            if (sub == 0) *reinterpret_cast<f32x4*>(&red[wave * K + 4 * ln + 256 * t]) = v;
        }
        __syncthreads();
        for (int k = tid; k < K; k += 256)
            slab[((long long)blockIdx.x * NO + j) * Ktot + cb + k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
        __syncthreads();
    }
    // bias partials: every lane of a (half-)wave holds the same sum over its rows
    if (ln == 0) {
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            float v = bacc[j];
            if (RPW == 2) v += __shfl_xor(v, 32);
            if (sub == 0) bred[wave][j] = v;
        }
    }
    __syncthreads();
    if (tid < NO && blockIdx.y == 0)
        bslab[(long long)blockIdx.x * NO + tid] = (bred[0][tid] + bred[1][tid]) + (bred[2][tid] + bred[3][tid]);
}

#define NU_SKINNY_BLOCKS 1024
extern "C" long long nu_skinny_bwd_workspace_bytes(int K, int NO) {
    return (long long)NU_SKINNY_BLOCKS * NO * (K + 1) * sizeof(float);
}

static int skinny_bwd_launch(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws, int ldw, int NO, float* dH,
                             int lddh, int relu_mask, int accumulate, float* dWs, int lddw, float* db, void* workspace,
                             long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, bool h16, hipStream_t stream);
extern "C" int nu_skinny_bwd_enqueue(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws,
                                     int ldw, int NO, float* dH, int lddh, int relu_mask, int accumulate, float* dWs,
                                     int lddw, float* db, void* workspace, long long workspace_bytes,
                                     NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream) {
    return skinny_bwd_launch(dy, ldy, H, ldh, P, K, Ws, ldw, NO, dH, lddh, relu_mask, accumulate, dWs, lddw, db, workspace, workspace_bytes,
                             descs, ndesc, cap, false, stream);
}
// H and dH are __bf16 (bf16-storage mode); dy, the head weights and every reduction stay fp32
extern "C" int nu_skinny_bwd_enqueue_h16(const float* dy, int ldy, const void* H, int ldh, int P, int K, const float* Ws,
                                         int ldw, int NO, void* dH, int lddh, int relu_mask, int accumulate, float* dWs,
                                         int lddw, float* db, void* workspace, long long workspace_bytes,
                                         NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream) {
    return skinny_bwd_launch(dy, ldy, static_cast<const float*>(H), ldh, P, K, Ws, ldw, NO, static_cast<float*>(dH), lddh, relu_mask,
                             accumulate, dWs, lddw, db, workspace, workspace_bytes, descs, ndesc, cap, true, stream);
}
static int skinny_bwd_launch(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws, int ldw, int NO, float* dH,
                             int lddh, int relu_mask, int accumulate, float* dWs, int lddw, float* db, void* workspace,
                             long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, bool h16, hipStream_t stream) {
    if (P <= 0) return NU_ERR_ARG;
    if (workspace_bytes < nu_skinny_bwd_workspace_bytes(K, NO)) return NU_ERR_WORKSPACE;
    if (*ndesc + 2 > cap) return NU_ERR_WORKSPACE;
    int blocks = nu_cdiv(P, 64);
    blocks = blocks < NU_SKINNY_BLOCKS ? blocks : NU_SKINNY_BLOCKS;
    float* slab = (float*)workspace;
    float* bslab = slab + (long long)NU_SKINNY_BLOCKS * NO * K;
#define NU_ARGS dy, ldy, H, ldh, P, Ws, ldw, dH, lddh, relu_mask, accumulate, slab, bslab, K
    if ((ldh & 3) || (lddh & 3) || (ldw & 3)) return NU_ERR_ARG;
    if (K == 128) {
        switch (NO) {
            case 1: if (h16) hipLaunchKernelGGL((skinny_bwd_kernel<1, 128, true>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); else hipLaunchKernelGGL((skinny_bwd_kernel<1, 128, false>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); break;
            case 3: if (h16) hipLaunchKernelGGL((skinny_bwd_kernel<3, 128, true>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); else hipLaunchKernelGGL((skinny_bwd_kernel<3, 128, false>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); break;
            default: return NU_ERR_ARG;
        }
    } else if (K == 256) {
        switch (NO) {
            case 1: if (h16) hipLaunchKernelGGL((skinny_bwd_kernel<1, 256, true>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); else hipLaunchKernelGGL((skinny_bwd_kernel<1, 256, false>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); break;
            case 3: if (h16) hipLaunchKernelGGL((skinny_bwd_kernel<3, 256, true>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); else hipLaunchKernelGGL((skinny_bwd_kernel<3, 256, false>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); break;
            // the four-wide head of the human-light predictor (h, w; field.py:615): fp32 rows only
            case 4: if (h16) return NU_ERR_ARG; hipLaunchKernelGGL((skinny_bwd_kernel<4, 256, false>), dim3(blocks), dim3(256), 0, stream, NU_ARGS); break;
            default: return NU_ERR_ARG;
        }
    } else if (K == 1024) {
        switch (NO) {
            case 6: if (h16) hipLaunchKernelGGL((skinny_bwd_kernel<6, 256, true>), dim3(blocks, 4), dim3(256), 0, stream, NU_ARGS); else hipLaunchKernelGGL((skinny_bwd_kernel<6, 256, false>), dim3(blocks, 4), dim3(256), 0, stream, NU_ARGS); break;
            default: return NU_ERR_ARG;
        }
    } else {
        return NU_ERR_ARG;
    }
#undef NU_ARGS
    int rc = nu_launch_status();
    if (rc) return rc;
    // slab is [blocks][NO][K]: `blocks` slabs of an NO x K matrix
    rc = nu_reduce_push(descs, ndesc, cap, slab, blocks, NO, K, K, (long long)NO * K, dWs, lddw, 1.0f, 0);
    if (rc == NU_OK && db) rc = nu_reduce_push(descs, ndesc, cap, bslab, blocks, NO, 1, 1, NO, db, 1, 1.0f, 0);
    return rc;
}

extern "C" int nu_skinny_bwd(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws, int ldw,
                             int NO, float* dH, int lddh, int relu_mask, int accumulate, float* dWs, int lddw,
                             float* db, void* workspace, long long workspace_bytes, hipStream_t stream) {
    NuReduceDesc descs[2];
    int n = 0;
    int rc = nu_skinny_bwd_enqueue(dy, ldy, H, ldh, P, K, Ws, ldw, NO, dH, lddh, relu_mask, accumulate, dWs, lddw, db,
                                   workspace, workspace_bytes, descs, &n, 2, stream);
    if (rc) return rc;
    return nu_slab_reduce_batched(descs, n, stream);
}

// ------------------------------------------------------------------------------------------------
// column sums (deterministic two-stage):  out[c] (+)= sum_p A[p, c],  c < ncols
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ A, int lda, int P, int ncols,
                                                             float* __restrict__ part) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    int rows_per = (P + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * rows_per;
    int p1 = p0 + rows_per;
    p1 = p1 < P ? p1 : P;
    if (c >= ncols) return;
    float s = 0.f;
    for (int p = p0; p < p1; ++p) s += A[(long long)p * lda + c];
    part[(long long)blockIdx.x * ncols + c] = s;
}

#define NU_COLSUM_BLOCKS 512
extern "C" long long nu_colsum_workspace_bytes(int ncols) { return (long long)NU_COLSUM_BLOCKS * ncols * sizeof(float); }
extern "C" int nu_colsum_enqueue(const float* A, int lda, int P, int ncols, float* out, int accumulate, void* workspace,
                                 long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream) {
    if (P <= 0 || ncols <= 0) return NU_ERR_ARG;
    if (workspace_bytes < nu_colsum_workspace_bytes(ncols)) return NU_ERR_WORKSPACE;
    int blocks = nu_cdiv(P, 128);
    blocks = blocks < NU_COLSUM_BLOCKS ? blocks : NU_COLSUM_BLOCKS;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(blocks, nu_cdiv(ncols, 256)), dim3(256), 0, stream, A, lda, P, ncols,
                       (float*)workspace);
    int rc = nu_launch_status();
    if (rc) return rc;
    return nu_reduce_push(descs, ndesc, cap, (const float*)workspace, blocks, 1, ncols, ncols, ncols, out, ncols, 1.0f,
                          accumulate);
}

extern "C" int nu_colsum(const float* A, int lda, int P, int ncols, float* out, int accumulate, void* workspace,
                         long long workspace_bytes, hipStream_t stream) {
    NuReduceDesc d[1];
    int n = 0;
    int rc = nu_colsum_enqueue(A, lda, P, ncols, out, accumulate, workspace, workspace_bytes, d, &n, 1, stream);
    if (rc) return rc;
    return nu_slab_reduce_batched(d, n, stream);
}

// ------------------------------------------------------------------------------------------------
// D[p, k] = w[k] * sp'(H[p, k])   -- seed of the SDF reverse sweep (delta_7 = W8[sdf row] * softplus'(a_7))
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowscale_dsp_kernel(const float* __restrict__ H, int ldh, long long P, int K,
                                                           const float* __restrict__ w, float* __restrict__ D, int ldd) {
    const int kq = K >> 2;
    const long long total = P * kq;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long p = i / kq;
        const int c = (int)(i - p * kq) * 4;
        const f32x4 h = *reinterpret_cast<const f32x4*>(H + p * ldh + c);
        const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ww[e] * nu_softplus100_grad_from_h(h[e]);
        *reinterpret_cast<f32x4*>(D + p * ldd + c) = o;
    }
}
extern "C" int nu_rowscale_dsp(const float* H, int ldh, int P, int K, const float* w, float* D, int ldd,
                               hipStream_t stream) {
    if (P <= 0) return NU_OK;
    if ((K & 3) || (ldh & 3) || (ldd & 3)) return NU_ERR_ARG;
    const long long total = (long long)P * (K >> 2);
    long long blocks = nu_cdivl(total, 256);
    blocks = blocks < 8192 ? blocks : 8192;
    hipLaunchKernelGGL(rowscale_dsp_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, H, ldh, (long long)P, K, w, D, ldd);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Fused Adam over many parameter tensors (train/trainer_zero.py:74-85 builds torch.optim.Adam; the update below is its
// single-tensor formula: exp_avg.lerp_(g, 1-b1); exp_avg_sq = b2*v + (1-b2) g^2; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)).
// Descriptors travel in the kernel-argument block (no host -> device copy), NU_ADAM_MAX tensors per launch.
// ------------------------------------------------------------------------------------------------
struct NuAdamBatch {
    NuAdamDesc d[NU_ADAM_MAX];
    int n;
    float lr_over_bc1, inv_sqrt_bc2, w1, beta2, w2, eps;   // w = 1 - beta, formed in double on the host like torch does
};
#define NU_ADAM_ELEMS 2048   // elements per block
__global__ __launch_bounds__(256) void adam_kernel(NuAdamBatch b) {
    int di = 0;
    for (int i = 1; i < b.n; ++i) di = ((int)blockIdx.x >= b.d[i].blk_begin) ? i : di;
    float* __restrict__ p = b.d[di].p;
    const float* __restrict__ g = b.d[di].g;
    float* __restrict__ m = b.d[di].m;
    float* __restrict__ v = b.d[di].v;
    const long long n = b.d[di].n;
    const long long base = (long long)((int)blockIdx.x - b.d[di].blk_begin) * NU_ADAM_ELEMS;
    const float w1 = b.w1, w2 = b.w2;
#pragma unroll
    for (int u = 0; u < NU_ADAM_ELEMS / 256; ++u) {
        const long long i = base + u * 256 + threadIdx.x;
        if (i >= n) break;
        const float gi = g[i];
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * w1;
        vi = vi * b.beta2 + (gi * gi) * w2;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * b.inv_sqrt_bc2 + b.eps;
        p[i] = p[i] - b.lr_over_bc1 * (mi / denom);
    }
}
extern "C" int nu_adam_desc_size(void) { return (int)sizeof(NuAdamDesc); }
extern "C" int nu_adam_step(const NuAdamDesc* descs, int n, double lr, double beta1_d, double beta2_d, double eps_d, int step,
                            hipStream_t stream) {
    if (n < 0 || step < 1) return NU_ERR_ARG;
    const float beta2 = (float)beta2_d, eps = (float)eps_d;
    const double bc1 = 1.0 - pow(beta1_d, (double)step), bc2 = 1.0 - pow(beta2_d, (double)step);
    int i = 0;
    while (i < n) {
        NuAdamBatch b;
        int blocks = 0, k = 0;
        for (; i < n && k < NU_ADAM_MAX; ++i) {
            if (descs[i].n <= 0) continue;
            b.d[k] = descs[i];
            b.d[k].blk_begin = blocks;
            blocks += (int)nu_cdivl(descs[i].n, NU_ADAM_ELEMS);
            ++k;
        }
        if (k == 0) break;
        b.n = k;
        b.lr_over_bc1 = (float)(lr / bc1);
        b.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        b.w1 = (float)(1.0 - (double)beta1_d); b.beta2 = beta2; b.w2 = (float)(1.0 - (double)beta2_d); b.eps = eps;
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, stream, b);
        const int rc = nu_launch_status();
        if (rc) return rc;
    }
    return NU_OK;
}
