// relight.hip -- relighting of the baked mesh under a lat-long HDR environment (gfx950): the resolve pass and the debug entries.
//
// Replaces the reference's hand-off to Blender (relight.py -> blender_backend/relight_backend.py: Principled BSDF from vertex colours,
// world environment texture, Cycles) with the project's own direct-light estimator, DESIGN.md 20.  Three passes per chunk of work:
//   nu_relight_gbuffer     closest hit per pixel centre -> face id + G-buffer row            (lbvh.hip: instantiates the traversal)
//   nu_relight_visibility  any-hit shadow ray per (hit pixel, sample), made in registers     (lbvh.hip)
//   nu_relight_resolve     per pixel: the same directions again, environment tap, BRDF weight, summed in sample order   (here)
// The sample sequence, the shadow ray, the environment lookup and the weight are relight.h, shared by all of them.  No allocation, no
// synchronisation, every launch on the caller's stream; no atomics: a pixel is summed by one thread, sample after sample, into the
// caller's accumulator, so the sum is the same bits however the pixels, images or sample ranges are chunked.
#include "relight.h"

__global__ __launch_bounds__(256) void relight_resolve_kernel(const float* __restrict__ gbuf, const int* __restrict__ pix, int n_pix, int S,
                                                              int s0, int s_count, unsigned seed, const float4* __restrict__ env, int eh,
                                                              int ew, const unsigned char* __restrict__ vis, float scale,
                                                              float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const long long row = pix[i];
    float g[NU_RL_ROW];
#pragma unroll
    for (int k = 0; k < NU_RL_ROW; k += 4) {
        const float4 q = *(const float4*)(gbuf + row * NU_RL_ROW + k);
        g[k] = q.x; g[k + 1] = q.y; g[k + 2] = q.z; g[k + 3] = q.w;
    }
    float acc[3];
    for (int c = 0; c < 3; ++c) acc[c] = out[row * 4 + c];
    const unsigned char* lit = vis + (long long)i * s_count;
    for (int c = 0; c < s_count; ++c) {
        if (!lit[c]) continue;
        int lobe;
        float l[3], hv[3], rad[3], wgt[3];
        unsigned bits[2];
        nu_relight_sample(g, S, s0 + c, seed, lobe, l, hv, bits);
        nu_relight_env(env, eh, ew, l, rad);
        nu_relight_weight(g, lobe, l, hv, wgt);
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (wgt[k] * rad[k]) * scale;
    }
    for (int c = 0; c < 3; ++c) out[row * 4 + c] = acc[c];
    out[row * 4 + 3] = 1.0f;
}

extern "C" int nu_relight_resolve(const float* gbuf, const int* pix, int n_pix, int samples, int s0, int s_count, int seed,
                                  const float* env, int env_h, int env_w, const unsigned char* vis, float scale, float* out,
                                  hipStream_t stream) {
    if (n_pix < 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples || env_h <= 0 || env_w <= 0)
        return NU_ERR_ARG;
    if (!gbuf || !pix || !env || !vis || !out) return NU_ERR_ARG;
    if (n_pix == 0 || s_count == 0) return NU_OK;
    hipLaunchKernelGGL(relight_resolve_kernel, dim3(nu_cdiv(n_pix, 256)), dim3(256), 0, stream, gbuf, pix, n_pix, samples, s0, s_count,
                       (unsigned)seed, (const float4*)env, env_h, env_w, vis, scale, out);
    return nu_launch_status();
}

// Resolve of the nested object: one thread per listed pixel (sel = indices into kind / chain / inner_rows, opix = the
// G-buffer row each of them writes).  An inner pixel adds T * weight * (1 - F_exit) * env(d_out) * scale of the samples [s0, s0 + s_count)
// in sample order (rec: their records, weights regenerated from the inner row); with last != 0 -- the call that ends a pixel -- the
// reflection term F_entry * env(r) * vis and, for an exit pixel, T * env(d_exit) * vis are added after the samples.  No atomics.
__global__ __launch_bounds__(256) void relight_nested_resolve_kernel(const float* __restrict__ irow, const float* __restrict__ chain,
                                                                     const int* __restrict__ kind, const int* __restrict__ opix,
                                                                     const int* __restrict__ sel, int n_sel, int S, int s0, int s_count,
                                                                     unsigned seed, const float4* __restrict__ env, int eh, int ew,
                                                                     const float4* __restrict__ rec, float scale, int last,
                                                                     float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel) return;
    const long long j = sel[i], row = opix[j];
    const float* ch = chain + j * NU_RLN_CHAIN;
    const int what = kind[j];
    const float T = ch[0];
    float acc[3];
    for (int c = 0; c < 3; ++c) acc[c] = out[row * 4 + c];
    if (what == NU_RLN_INNER && s_count > 0) {
        float g[NU_RL_ROW];
#pragma unroll
        for (int k = 0; k < NU_RL_ROW; k += 4) {
            const float4 q = *(const float4*)(irow + j * NU_RL_ROW + k);
            g[k] = q.x; g[k + 1] = q.y; g[k + 2] = q.z; g[k + 3] = q.w;
        }
        const float4* r = rec + (long long)i * s_count;
        for (int c = 0; c < s_count; ++c) {
            const float4 e = r[c];
            if (e.w == 0.0f) continue;
            int lobe;
            float l[3], hv[3], rad[3], wgt[3];
            unsigned bits[2];
            nu_relight_sample(g, S, s0 + c, seed, lobe, l, hv, bits);
            const float dout[3] = {e.x, e.y, e.z};
            nu_relight_env(env, eh, ew, dout, rad);
            nu_relight_weight(g, lobe, l, hv, wgt);
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (T * ((wgt[k] * e.w) * rad[k])) * scale;
        }
    }
    if (last) {
        float rad[3];
        if (ch[8] > 0.0f && ch[9] > 0.0f) {
            nu_relight_env(env, eh, ew, ch + 5, rad);
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + ch[8] * rad[k];
        }
        if (what == NU_RLN_EXIT && ch[4] > 0.0f) {
            nu_relight_env(env, eh, ew, ch + 1, rad);
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + T * rad[k];
        }
    }
    for (int c = 0; c < 3; ++c) out[row * 4 + c] = acc[c];
    out[row * 4 + 3] = 1.0f;
}

extern "C" int nu_relight_nested_resolve(const float* inner_rows, const float* chain, const int* kind, const int* opix, const int* sel,
                                         int n_sel, int samples, int s0, int s_count, int seed, const float* env, int env_h, int env_w,
                                         const float* rec, float scale, int last, float* out, hipStream_t stream) {
    if (n_sel < 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples || env_h <= 0 || env_w <= 0)
        return NU_ERR_ARG;
    if (n_sel == 0 || (s_count == 0 && !last)) return NU_OK;
    if (!inner_rows || !chain || !kind || !opix || !sel || !env || !out || (s_count > 0 && !rec)) return NU_ERR_ARG;
    hipLaunchKernelGGL(relight_nested_resolve_kernel, dim3(nu_cdiv(n_sel, 256)), dim3(256), 0, stream, inner_rows, chain, kind, opix, sel,
                       n_sel, samples, s0, s_count, (unsigned)seed, (const float4*)env, env_h, env_w, (const float4*)rec, scale, last, out);
    return nu_launch_status();
}

// exactly the rays nu_relight_visibility makes (the same device function), written out: rays [n_pix * s_count, 6]; bits (optional)
// [n_pix * s_count, 3] = the two 24-bit sample integers and 1 where the ray is traced
__global__ __launch_bounds__(256) void relight_shadow_rays_kernel(const float* __restrict__ gbuf, const int* __restrict__ pix, int n_pix,
                                                                  int S, int s0, int s_count, unsigned seed, float eps,
                                                                  float* __restrict__ rays, int* __restrict__ bits_out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long long)n_pix * s_count) return;
    const int i = (int)(r / s_count), c = (int)(r - (long long)i * s_count);
    float o[3], d[3];
    unsigned bits[2];
    const bool traced = nu_relight_shadow_ray(gbuf + (long long)pix[i] * NU_RL_ROW, S, s0 + c, seed, eps, o, d, bits);
    for (int k = 0; k < 3; ++k) { rays[r * 6 + k] = o[k]; rays[r * 6 + 3 + k] = d[k]; }
    if (bits_out) { bits_out[r * 3] = (int)bits[0]; bits_out[r * 3 + 1] = (int)bits[1]; bits_out[r * 3 + 2] = traced ? 1 : 0; }
}

extern "C" int nu_relight_shadow_rays(const float* gbuf, const int* pix, int n_pix, int samples, int s0, int s_count, int seed, float eps,
                                      float* rays, int* bits, hipStream_t stream) {
    if (n_pix < 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples) return NU_ERR_ARG;
    if (!gbuf || !pix || !rays) return NU_ERR_ARG;
    const long long N = (long long)n_pix * s_count;
    if (N == 0) return NU_OK;
    if (nu_cdivl(N, 256) > 0x7fffffffLL) return NU_ERR_ARG;
    hipLaunchKernelGGL(relight_shadow_rays_kernel, dim3((unsigned)nu_cdivl(N, 256)), dim3(256), 0, stream, gbuf, pix, n_pix, samples, s0,
                       s_count, (unsigned)seed, eps, rays, bits);
    return nu_launch_status();
}

__global__ __launch_bounds__(256) void relight_env_lookup_kernel(const float4* __restrict__ env, int eh, int ew,
                                                                 const float* __restrict__ dirs, int N, float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float d[3] = {dirs[r * 3LL], dirs[r * 3LL + 1], dirs[r * 3LL + 2]};
    float rgb[3];
    nu_relight_env(env, eh, ew, d, rgb);
    for (int k = 0; k < 3; ++k) out[r * 3LL + k] = rgb[k];
}

extern "C" int nu_relight_env_lookup(const float* env, int env_h, int env_w, const float* dirs, int N, float* out, hipStream_t stream) {
    if (N < 0 || env_h <= 0 || env_w <= 0 || !env || (N > 0 && (!dirs || !out))) return NU_ERR_ARG;
    if (N == 0) return NU_OK;
    hipLaunchKernelGGL(relight_env_lookup_kernel, dim3(nu_cdiv(N, 256)), dim3(256), 0, stream, (const float4*)env, env_h, env_w, dirs, N,
                       out);
    return nu_launch_status();
}

// ---- split-sum relighting from a prefiltered pyramid ---------------------------------------------------------------------
struct RlLevels {                    // kernel argument: the ascending roughness levels of the pyramid
    float v[NU_ENV_MAX_LOBES];
};

// L(d, rho) of the pyramid pyr [L, ph, pw] RGBA: rho clamped to the levels' range, the two levels around it tapped as nu_relight_env does
// and mixed linearly.  At a level the weight of the other tap is exactly 0, so the value has the bits of that level's tap.
static __device__ inline void nu_rl_pyramid(const float4* __restrict__ pyr, int L, int ph, int pw, const RlLevels& lv, const float* d,
                                            float rho, float* rgb) {
    if (L == 1) {
        nu_relight_env(pyr, ph, pw, d, rgb);
        return;
    }
    const float r = fminf(fmaxf(rho, lv.v[0]), lv.v[L - 1]);
    int i = 0;
    float lo = lv.v[0], hi = lv.v[1];
#pragma unroll
    for (int k = 1; k < NU_ENV_MAX_LOBES - 1; ++k)
        if (k < L - 1 && r >= lv.v[k]) { i = k; lo = lv.v[k]; hi = lv.v[k + 1]; }
    const float t = (r - lo) / (hi - lo);
    float a[3], b[3];
    const long long plane = (long long)ph * pw;
    nu_relight_env(pyr + i * plane, ph, pw, d, a);
    nu_relight_env(pyr + (i + 1) * plane, ph, pw, d, b);
    for (int c = 0; c < 3; ++c) rgb[c] = (1.0f - t) * a[c] + t * b[c];
}

__global__ __launch_bounds__(256) void relight_pyramid_lookup_kernel(const float4* __restrict__ pyr, int L, int ph, int pw, RlLevels lv,
                                                                     const float* __restrict__ dirs, const float* __restrict__ rho, int N,
                                                                     float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float d[3] = {dirs[r * 3LL], dirs[r * 3LL + 1], dirs[r * 3LL + 2]};
    float rgb[3];
    nu_rl_pyramid(pyr, L, ph, pw, lv, d, rho[r], rgb);
    for (int k = 0; k < 3; ++k) out[r * 3LL + k] = rgb[k];
}

// The levels of a call as a kernel argument; false when they are not finite and strictly ascending.
static bool nu_rl_levels(const float* levels, int L, RlLevels& lv) {
    for (int k = 0; k < NU_ENV_MAX_LOBES; ++k) lv.v[k] = 0.0f;
    for (int k = 0; k < L; ++k) {
        if (!(levels[k] > -3e38f && levels[k] < 3e38f) || (k > 0 && !(levels[k] > levels[k - 1]))) return false;
        lv.v[k] = levels[k];
    }
    return true;
}

extern "C" int nu_env_pyramid_lookup(const float* pyr, int L, int ph, int pw, const float* levels, const float* dirs, const float* rho, int N,
                                     float* out, hipStream_t stream) {
    if (N < 0 || L < 1 || L > NU_ENV_MAX_LOBES || ph <= 0 || pw <= 0 || !pyr || !levels || (N > 0 && (!dirs || !rho || !out)))
        return NU_ERR_ARG;
    RlLevels lv;
    if (!nu_rl_levels(levels, L, lv)) return NU_ERR_ARG;
    if (N == 0) return NU_OK;
    hipLaunchKernelGGL(relight_pyramid_lookup_kernel, dim3(nu_cdiv(N, 256)), dim3(256), 0, stream, (const float4*)pyr, L, ph, pw, lv, dirs,
                       rho, N, out);
    return nu_launch_status();
}

// (A, B) of the split-sum table fg [256,256,2] at (u, v) in [0,1]^2: the values of nu_lut (render.hip) -- texel centres at (i + 1/2) / 256,
// bilinear, clamped to the edge -- restated without its derivatives.
static __device__ inline void nu_rl_fg(const float* __restrict__ fg, float u, float v, float& A, float& B) {
    const float fx = fminf(fmaxf(u * 256.0f - 0.5f, 0.f), 255.f), fy = fminf(fmaxf(v * 256.0f - 0.5f, 0.f), 255.f);
    const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    const int x1 = x0 + 1 < 255 ? x0 + 1 : 255, y1 = y0 + 1 < 255 ? y0 + 1 : 255;
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const float2 l00 = *(const float2*)(fg + (y0 * 256 + x0) * 2), l01 = *(const float2*)(fg + (y0 * 256 + x1) * 2);
    const float2 l10 = *(const float2*)(fg + (y1 * 256 + x0) * 2), l11 = *(const float2*)(fg + (y1 * 256 + x1) * 2);
    A = (l00.x * (1 - tx) + l01.x * tx) * (1 - ty) + (l10.x * (1 - tx) + l11.x * tx) * ty;
    B = (l00.y * (1 - tx) + l01.y * tx) * (1 - ty) + (l10.y * (1 - tx) + l11.y * tx) * ty;
}

// One thread per listed hit pixel: rgb = (1 - m) a Ld(n) + (F0 A + B) L(reflect(v, n), rho), written.
__global__ __launch_bounds__(256) void relight_splitsum_kernel(const float* __restrict__ gbuf, const int* __restrict__ pix, int n_pix,
                                                               const float4* __restrict__ pyr, int L, int ph, int pw, RlLevels lv,
                                                               const float4* __restrict__ diffuse, int dh, int dw,
                                                               const float* __restrict__ fg, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const long long row = pix[i];
    float g[NU_RL_ROW];
#pragma unroll
    for (int k = 0; k < NU_RL_ROW; k += 4) {
        const float4 q = *(const float4*)(gbuf + row * NU_RL_ROW + k);
        g[k] = q.x; g[k + 1] = q.y; g[k + 2] = q.z; g[k + 3] = q.w;
    }
    const float* n = g + 7;
    const float* v = g + 15;
    const float m = g[13], rho = g[14];
    const float nov = nu_rl_dot3(n, v);
    float r[3], ld[3], ls[3], A, B;
    for (int c = 0; c < 3; ++c) r[c] = (2.0f * nov) * n[c] - v[c];
    nu_relight_env(diffuse, dh, dw, n, ld);
    nu_rl_pyramid(pyr, L, ph, pw, lv, r, rho, ls);
    nu_rl_fg(fg, fminf(fmaxf(nov, 0.f), 1.f), fminf(fmaxf(rho, 0.f), 1.f), A, B);
    float4 o;
    float rgb[3];
    for (int c = 0; c < 3; ++c) {
        const float f0 = 0.04f * (1.0f - m) + m * g[10 + c];
        rgb[c] = ((1.0f - m) * g[10 + c]) * ld[c] + (f0 * A + B) * ls[c];
    }
    o.x = rgb[0]; o.y = rgb[1]; o.z = rgb[2]; o.w = 1.0f;
    *(float4*)(out + row * 4) = o;
}

extern "C" int nu_relight_splitsum(const float* gbuf, const int* pix, int n_pix, const float* pyr, int L, int ph, int pw, const float* levels,
                                   const float* diffuse, int dh, int dw, const float* fg, float* out, hipStream_t stream) {
    if (n_pix < 0 || L < 1 || L > NU_ENV_MAX_LOBES || ph <= 0 || pw <= 0 || dh <= 0 || dw <= 0) return NU_ERR_ARG;
    if (!gbuf || (n_pix > 0 && !pix) || !pyr || !levels || !diffuse || !fg || !out) return NU_ERR_ARG;      // an empty hit list may have no address
    RlLevels lv;
    if (!nu_rl_levels(levels, L, lv)) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    hipLaunchKernelGGL(relight_splitsum_kernel, dim3(nu_cdiv(n_pix, 256)), dim3(256), 0, stream, gbuf, pix, n_pix, (const float4*)pyr, L, ph,
                       pw, lv, (const float4*)diffuse, dh, dw, fg, out);
    return nu_launch_status();
}

// ---- visibility transfer: the shadowed split-sum resolve and the test entry of the bake's rays ---------------------------
// exactly the rays nu_transfer_bake makes (the same device functions), written out: rays [n * samples, 6], bits [n * samples, 2] = the
// two 24-bit sample integers
__global__ __launch_bounds__(256) void transfer_rays_kernel(const float* __restrict__ points, const float* __restrict__ normals, int n,
                                                            int id0, int S, unsigned seed, float eps, float* __restrict__ rays,
                                                            int* __restrict__ bits_out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long long)n * S) return;
    const int i = (int)(r / S), s = (int)(r - (long long)i * S);
    float p[3], nn[3], o[3], d[3];
    for (int k = 0; k < 3; ++k) { p[k] = points[i * 3LL + k]; nn[k] = normals[i * 3LL + k]; }
    unsigned bits[2];
    nu_transfer_uniforms((int)((unsigned)id0 + (unsigned)i), seed, S, s, bits);
    nu_transfer_ray(p, nn, eps, bits, o, d);
    for (int k = 0; k < 3; ++k) { rays[r * 6 + k] = o[k]; rays[r * 6 + 3 + k] = d[k]; }
    if (bits_out) { bits_out[r * 2] = (int)bits[0]; bits_out[r * 2 + 1] = (int)bits[1]; }
}

extern "C" int nu_transfer_rays(const float* points, const float* normals, int n, int id0, int samples, int seed, float eps, float* rays,
                                int* bits, hipStream_t stream) {
    if (n < 0 || samples < 16 || (samples & 15) || !(eps > -3e38f && eps < 3e38f)) return NU_ERR_ARG;
    const long long N = (long long)n * samples;
    if (N > 0x7fffffffLL) return NU_ERR_ARG;
    if (N == 0) return NU_OK;
    if (!points || !normals || !rays) return NU_ERR_ARG;
    hipLaunchKernelGGL(transfer_rays_kernel, dim3((unsigned)nu_cdivl(N, 256)), dim3(256), 0, stream, points, normals, n, id0, samples,
                       (unsigned)seed, eps, rays, bits);
    return nu_launch_status();
}

// One thread per listed hit pixel: nu_relight_splitsum's two terms D and Sp from its device functions in its order, then the transfer
// row at the hit point (relight.h) shadows them:  NU_OCC_AO  ao D + so Sp;  NU_OCC_SH  (1 - m) a max(sum_k T_k L_k, 0) + so Sp.
__global__ __launch_bounds__(256) void relight_splitsum_occluded_kernel(const float* __restrict__ gbuf, const int* __restrict__ face,
                                                                        const int* __restrict__ pix, int n_pix, const float* __restrict__ V,
                                                                        const int* __restrict__ F, const float* __restrict__ transfer,
                                                                        const float4* __restrict__ envsh, int mode,
                                                                        const float4* __restrict__ pyr, int L, int ph, int pw, RlLevels lv,
                                                                        const float4* __restrict__ diffuse, int dh, int dw,
                                                                        const float* __restrict__ fg, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const long long row = pix[i];
    float g[NU_RL_ROW];
#pragma unroll
    for (int k = 0; k < NU_RL_ROW; k += 4) {
        const float4 q = *(const float4*)(gbuf + row * NU_RL_ROW + k);
        g[k] = q.x; g[k + 1] = q.y; g[k + 2] = q.z; g[k + 3] = q.w;
    }
    const float* n = g + 7;
    const float* v = g + 15;
    const float m = g[13], rho = g[14];
    const float nov = nu_rl_dot3(n, v);
    float r[3], ld[3], ls[3], A, B;
    for (int c = 0; c < 3; ++c) r[c] = (2.0f * nov) * n[c] - v[c];
    nu_relight_env(diffuse, dh, dw, n, ld);
    nu_rl_pyramid(pyr, L, ph, pw, lv, r, rho, ls);
    nu_rl_fg(fg, fminf(fmaxf(nov, 0.f), 1.f), fminf(fmaxf(rho, 0.f), 1.f), A, B);
    float tr[NU_TR_LIVE];
    nu_transfer_at(V, F, transfer, face[row], g + 1, tr);
    const float ao = tr[9];
    const float so = nu_transfer_spec_occlusion(nov, ao, rho);
    float4 o;
    float rgb[3];
    for (int c = 0; c < 3; ++c) {
        const float f0 = 0.04f * (1.0f - m) + m * g[10 + c];
        const float kd = (1.0f - m) * g[10 + c];
        const float sp = (f0 * A + B) * ls[c];
        if (mode == NU_OCC_AO) {
            rgb[c] = ao * (kd * ld[c]) + so * sp;
        } else {
            float e = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float4 lk = envsh[k];
                e = e + tr[k] * (c == 0 ? lk.x : (c == 1 ? lk.y : lk.z));
            }
            rgb[c] = kd * fmaxf(e, 0.0f) + so * sp;
        }
    }
    o.x = rgb[0]; o.y = rgb[1]; o.z = rgb[2]; o.w = 1.0f;
    *(float4*)(out + row * 4) = o;
}

extern "C" int nu_relight_splitsum_occluded(const float* gbuf, const int* face, const int* pix, int n_pix, const float* V, const int* F,
                                            const float* transfer, const float* envsh, int mode, const float* pyr, int L, int ph, int pw,
                                            const float* levels, const float* diffuse, int dh, int dw, const float* fg, float* out,
                                            hipStream_t stream) {
    if (n_pix < 0 || L < 1 || L > NU_ENV_MAX_LOBES || ph <= 0 || pw <= 0 || dh <= 0 || dw <= 0) return NU_ERR_ARG;
    if (mode != NU_OCC_AO && mode != NU_OCC_SH) return NU_ERR_ARG;
    if (!gbuf || !face || (n_pix > 0 && !pix) || !V || !F || !transfer || (mode == NU_OCC_SH && !envsh) || !pyr || !levels || !diffuse || !fg
        || !out)
        return NU_ERR_ARG;
    RlLevels lv;
    if (!nu_rl_levels(levels, L, lv)) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    hipLaunchKernelGGL(relight_splitsum_occluded_kernel, dim3(nu_cdiv(n_pix, 256)), dim3(256), 0, stream, gbuf, face, pix, n_pix, V, F,
                       transfer, (const float4*)envsh, mode, (const float4*)pyr, L, ph, pw, lv, (const float4*)diffuse, dh, dw, fg, out);
    return nu_launch_status();
}
