// human_light.hip -- the photographer's reflection of stage-1 shading (shader_config.human_light, field.py:411-445, :614-634).
//
// The specular query of an inner point looks along its reflection direction r; where that ray meets the XY plane of the "human"
// frame of the ray's camera (renderer.get_human_coordinate_poses) inside a disc, a small predictor sees the integrated positional
// encoding of the hit point and returns a light h and a weight w that replace part of the direct light (csrc/render.hip,
// shade_combine_kernel<.., .., true>).  This file holds the predictor's input rows and their backward:
//
//   x' = R x + t,  r' = R r,  plane = |r'_z| > 1e-4,  dist = -x'_z / r'_z,  inter = x' + dist r'
//   mean = 0.3 inter.xy,  var = rho (0.3 dist)^2,  hit = plane and |mean| < 1.5 and dist > 0
//   HLin[(k, c)]      = exp(-0.5 4^k var) sin(2^k mean_c)              k = 0..5, c = x, y (c fastest)
//   HLin[12 + (k, c)] = exp(-0.5 4^k var) sin(2^k mean_c + 0.5 pi)     (the fp32 sum, as IPE forms it -- not cos)
//
// A row that does not hit encodes mean = var = 0 and receives no gradient.  The reference multiplies by the hit flag; here the
// values are SELECTED, so that an infinite or undefined dist of a near-parallel row never meets a multiplication by zero.  Every
// comparison is written so that a NaN operand gives "no hit".
//
// One row per lane.  sinf / expf are the library functions: the arguments reach 32 * 1.5 = 48.
#include "nu_common.h"

#define NU_HL_COLS 24
#define NU_HL_SCALE 0.3f
#define NU_HL_HALF_PI 1.57079632679489661923f

// n^, v^ = -d^, r = 2 (n^.v^) n^ - v^ of a point record, as the shading encoder forms them (csrc/encode.hip nu_shade_dirs)
static __device__ inline void hl_dirs(const float* n, const float* d, float* nh, float* vh, float* r, float& nov, float& inv_norm) {
    const float nn = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    inv_norm = 1.0f / fmaxf(nn, 1e-12f);
    const float vn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float ivn = 1.0f / fmaxf(vn, 1e-12f);
#pragma unroll
    for (int c = 0; c < 3; ++c) { nh[c] = n[c] * inv_norm; vh[c] = -d[c] * ivn; }
    nov = nh[0] * vh[0] + nh[1] * vh[1] + nh[2] * vh[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = nov * nh[c] * 2.0f - vh[c];
}

struct HlPlane {
    float xz, rp[3];        // x'_z and r' in the human frame
    float dist, mean[2];
    bool hit;
};
static __device__ inline HlPlane hl_plane(const float* __restrict__ pose, const float* x, const float* r) {
    HlPlane o;
    float xp[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* row = pose + i * 4;
        xp[i] = row[0] * x[0] + row[1] * x[1] + row[2] * x[2] + row[3];
        o.rp[i] = row[0] * r[0] + row[1] * r[1] + row[2] * r[2];
    }
    o.xz = xp[2];
    const bool plane = fabsf(o.rp[2]) > 1e-4f;
    o.dist = -xp[2] / o.rp[2];
    o.mean[0] = (xp[0] + o.dist * o.rp[0]) * NU_HL_SCALE;
    o.mean[1] = (xp[1] + o.dist * o.rp[1]) * NU_HL_SCALE;
    const float nrm = sqrtf(o.mean[0] * o.mean[0] + o.mean[1] * o.mean[1]);
    o.hit = plane && (nrm < 1.5f) && (o.dist > 0.f);
    return o;
}

__global__ __launch_bounds__(256) void human_encode_fwd_kernel(const float* __restrict__ nrm, const float* __restrict__ pt, int pt_ld,
                                                               const float* __restrict__ Mraw, int ldm, const int* __restrict__ idx,
                                                               int S, const float* __restrict__ poses, int n_poses, int P, int ld_hl,
                                                               float* __restrict__ HLin, float* __restrict__ rec) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float n[3], d[3], x[3], nh[3], vh[3], r[3], nov, inorm;
#pragma unroll
    for (int c = 0; c < 3; ++c) { n[c] = nrm[p * 3LL + c]; d[c] = pt[(long long)p * pt_ld + 4 + c]; x[c] = pt[(long long)p * pt_ld + c]; }
    hl_dirs(n, d, nh, vh, r, nov, inorm);
    const float rho = nu_sigmoid(Mraw[(long long)p * ldm + 1]);
    const int ray = idx[p] / S;
    HlPlane h{};                                   // out-of-range ray index: no hit, nothing indeterminate is read
    if (ray >= 0 && ray < n_poses) h = hl_plane(poses + (long long)ray * 12, x, r);
    const float sd = h.dist * NU_HL_SCALE;
    const float mean0 = h.hit ? h.mean[0] : 0.f, mean1 = h.hit ? h.mean[1] : 0.f;
    const float var = h.hit ? rho * (sd * sd) : 0.f;
    float* out = HLin + (long long)p * ld_hl;
    float scale = 1.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float a = expf(-0.5f * (var * (scale * scale)));
        const float m0 = mean0 * scale, m1 = mean1 * scale;
        out[2 * k] = a * sinf(m0);
        out[2 * k + 1] = a * sinf(m1);
        out[12 + 2 * k] = a * sinf(m0 + NU_HL_HALF_PI);
        out[12 + 2 * k + 1] = a * sinf(m1 + NU_HL_HALF_PI);
        scale *= 2.0f;
    }
    for (int c = NU_HL_COLS; c < ld_hl; ++c) out[c] = 0.f;
    f32x4 rc = {h.hit ? 1.0f : 0.f, h.hit ? h.dist : 0.f, mean0, mean1};
    *reinterpret_cast<f32x4*>(rec + (long long)p * 4) = rc;
}

extern "C" int nu_human_encode_fwd(const float* nrm, const float* pt, int pt_ld, const float* Mraw, int ldm, const int* idx, int S,
                                   const float* poses, int n_poses, int P, int ld_hl, float* HLin, float* rec, hipStream_t stream) {
    if (P <= 0) return NU_OK;
    if (S <= 0 || n_poses <= 0 || ld_hl < NU_HL_COLS || pt_ld < 7 || ldm < 2 || ((uintptr_t)rec & 15)) return NU_ERR_ARG;
    hipLaunchKernelGGL(human_encode_fwd_kernel, dim3(nu_cdiv(P, 256)), dim3(256), 0, stream, nrm, pt, pt_ld, Mraw, ldm, idx, S, poses,
                       n_poses, P, ld_hl, HLin, rec);
    return nu_launch_status();
}

// backward: dHLin [P, ld_hl] -> dn [P,3] += (through r and n^ = n / |n|, w.r.t. the RAW normal), dMraw[p,1] += d rho rho (1 - rho).
// Both ACCUMULATE: nu_shade_encode_bwd has written the rows on the same stream.  Points and poses carry no gradient.
//   d mean_c = sum_k a_k 2^k (g_kc cos(2^k mean_c) + g'_kc cos(2^k mean_c + pi/2)),   a_k = exp(-0.5 4^k var)
//   d var    = sum_kc -0.5 4^k a_k (g_kc sin(.) + g'_kc sin(. + pi/2))
//   d dist   = 0.3 (d mean . r'_xy) + d var rho 2 0.09 dist;   d r'_xy = 0.3 dist d mean;   d r'_z = -d dist dist / r'_z
//   d r = R^T d r';   d rho = d var (0.3 dist)^2
__global__ __launch_bounds__(256) void human_encode_bwd_kernel(const float* __restrict__ nrm, const float* __restrict__ pt, int pt_ld,
                                                               const float* __restrict__ Mraw, int ldm, const int* __restrict__ idx,
                                                               int S, const float* __restrict__ poses, int n_poses,
                                                               const float* __restrict__ rec, const float* __restrict__ dHLin,
                                                               int ld_hl, int P, float* __restrict__ dn, float* __restrict__ dMraw,
                                                               int lddm) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const f32x4 rc = *reinterpret_cast<const f32x4*>(rec + (long long)p * 4);
    if (!(rc[0] > 0.5f)) return;                       // no hit: exactly no gradient
    const int ray = idx[p] / S;
    if (ray < 0 || ray >= n_poses) return;
    float n[3], d[3], nh[3], vh[3], r[3], nov, inorm;
#pragma unroll
    for (int c = 0; c < 3; ++c) { n[c] = nrm[p * 3LL + c]; d[c] = pt[(long long)p * pt_ld + 4 + c]; }
    hl_dirs(n, d, nh, vh, r, nov, inorm);
    const float rho = nu_sigmoid(Mraw[(long long)p * ldm + 1]);
    const float* pose = poses + (long long)ray * 12;
    float rp[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) rp[i] = pose[i * 4] * r[0] + pose[i * 4 + 1] * r[1] + pose[i * 4 + 2] * r[2];
    const float dist = rc[1], mean0 = rc[2], mean1 = rc[3];
    const float sd = dist * NU_HL_SCALE;
    const float var = rho * (sd * sd);
    const float* g = dHLin + (long long)p * ld_hl;
    float dm0 = 0.f, dm1 = 0.f, dvar = 0.f, scale = 1.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float s2 = scale * scale;
        const float a = expf(-0.5f * (var * s2));
        const float m0 = mean0 * scale, m1 = mean1 * scale;
        const float g0 = g[2 * k], g1 = g[2 * k + 1], h0 = g[12 + 2 * k], h1 = g[12 + 2 * k + 1];
        dm0 += a * scale * (g0 * cosf(m0) + h0 * cosf(m0 + NU_HL_HALF_PI));
        dm1 += a * scale * (g1 * cosf(m1) + h1 * cosf(m1 + NU_HL_HALF_PI));
        dvar -= 0.5f * s2 * a * (g0 * sinf(m0) + g1 * sinf(m1) + h0 * sinf(m0 + NU_HL_HALF_PI) + h1 * sinf(m1 + NU_HL_HALF_PI));
        scale *= 2.0f;
    }
    const float di0 = dm0 * NU_HL_SCALE, di1 = dm1 * NU_HL_SCALE;
    const float ddist = di0 * rp[0] + di1 * rp[1] + dvar * rho * 2.0f * (NU_HL_SCALE * NU_HL_SCALE) * dist;
    const float drp[3] = {di0 * dist, di1 * dist, -ddist * dist / rp[2]};
    float dr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dr[c] = pose[c] * drp[0] + pose[4 + c] * drp[1] + pose[8 + c] * drp[2];
    // r = 2 NoV n^ - v^ ; NoV = n^ . v^ ; n^ = n / |n|
    const float dnov = 2.0f * (dr[0] * nh[0] + dr[1] * nh[1] + dr[2] * nh[2]);
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = 2.0f * nov * dr[c] + dnov * vh[c];
    const float dotp = t[0] * nh[0] + t[1] * nh[1] + t[2] * nh[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) dn[p * 3LL + c] += (t[c] - nh[c] * dotp) * inorm;
    dMraw[(long long)p * lddm + 1] += dvar * (sd * sd) * rho * (1.0f - rho);
}

extern "C" int nu_human_encode_bwd(const float* nrm, const float* pt, int pt_ld, const float* Mraw, int ldm, const int* idx, int S,
                                   const float* poses, int n_poses, const float* rec, const float* dHLin, int ld_hl, int P, float* dn,
                                   float* dMraw, int lddm, hipStream_t stream) {
    if (P <= 0) return NU_OK;
    if (S <= 0 || n_poses <= 0 || ld_hl < NU_HL_COLS || pt_ld < 7 || ldm < 2 || lddm < 2 || ((uintptr_t)rec & 15)) return NU_ERR_ARG;
    hipLaunchKernelGGL(human_encode_bwd_kernel, dim3(nu_cdiv(P, 256)), dim3(256), 0, stream, nrm, pt, pt_ld, Mraw, ldm, idx, S, poses,
                       n_poses, rec, dHLin, ld_hl, P, dn, dMraw, lddm);
    return nu_launch_status();
}
