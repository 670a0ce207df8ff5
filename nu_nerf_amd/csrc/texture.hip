// texture.hip -- the per-triangle texture atlas of the relightable asset (gfx950): texels -> surface points for the material
// bake, the bilinear lookup, and the pass that puts texture values into the material columns of a G-buffer; and the same
// lookup on the atlas's normal lanes, for a list of points and into the shading-normal columns of a G-buffer.
//
// The atlas is a square of T x T texels cut into cols x cols square cells of c = T / cols texels; cell k holds faces 2k (its lower
// triangle) and 2k + 1 (the point mirror of it), nu_atlas_layout below and texture.atlas_layout in Python are the same arithmetic.  A
// texel carries the value at EXTRAPOLATED barycentrics, so a face's values are affine over everything it owns and a bilinear lookup
// inside its triangle never needs a texel of another face.  Everything here is one thread per item, no LDS, no atomics, no workspace,
// no allocation, every launch on the caller's stream; FMA contraction is off, each operation is one fp32 rounding in the order written.
#include "relight.h"

#pragma clang fp contract(off)

struct AtlasLayout {
    int T, nf, pad, cols, c, L;
};

// cols = ceil(sqrt(ceil(nf / 2))), c = T / cols, L = c - 3 - 3 pad >= 2
static bool nu_atlas_layout(int n_faces, int T, int pad, AtlasLayout& a) {
    if (n_faces < 1 || T < 1 || T > NU_ATLAS_MAX_SIZE || pad < 0 || pad > NU_ATLAS_MAX_PAD) return false;
    const long long cells = ((long long)n_faces + 1) / 2;
    long long cols = 1;
    while (cols * cols < cells) ++cols;
    if (cols > T) return false;
    a.T = T; a.nf = n_faces; a.pad = pad; a.cols = (int)cols;
    a.c = T / (int)cols;
    a.L = a.c - 3 - 3 * pad;
    return a.L >= 2;
}

// Owner of texel (x, y): the face id, or -1; (s, t) = its cell-local coordinates in the frame of that face (mirrored for an upper face).
static __device__ inline int nu_atlas_owner(const AtlasLayout& a, int x, int y, int& s, int& t) {
    const int cx = x / a.c, cy = y / a.c;
    if (cx >= a.cols || cy >= a.cols) return -1;
    const int i = x - cx * a.c, j = y - cy * a.c;
    if (i + j == a.c - 1) return -1;                                   // the diagonal belongs to nobody
    const int h = i + j >= a.c ? 1 : 0;
    const long long f = 2LL * ((long long)cy * a.cols + cx) + h;
    if (f >= a.nf) return -1;
    s = h ? a.c - 1 - i : i;
    t = h ? a.c - 1 - j : j;
    return (int)f;
}

// rows [y0, y0 + rows) of the atlas, one thread per texel: blockIdx.y is the row, a block covers 256 consecutive texels of it (a wave
// stores 1 KB contiguous); one 16-byte store per texel and output
__global__ __launch_bounds__(256) void atlas_texels_kernel(const float* __restrict__ V, int nv, const int* __restrict__ F,
                                                           const float* __restrict__ VN, AtlasLayout a, int y0,
                                                           float4* __restrict__ texel, float4* __restrict__ normal) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.T) return;
    const int y = y0 + (int)blockIdx.y;
    const long long r = (long long)blockIdx.y * a.T + x;
    int s = 0, t = 0;
    int id = nu_atlas_owner(a, x, y, s, t);
    int vi[3] = {0, 0, 0};
    if (id >= 0) {
        for (int k = 0; k < 3; ++k) vi[k] = F[id * 3LL + k];
        if ((unsigned)vi[0] >= (unsigned)nv || (unsigned)vi[1] >= (unsigned)nv || (unsigned)vi[2] >= (unsigned)nv) id = -1;
    }
    float4 p = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 nq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (id >= 0) {
        const float b1 = (float)(s - a.pad) / (float)a.L, b2 = (float)(t - a.pad) / (float)a.L;
        const float b0 = (1.0f - b1) - b2;
        float v0[3], v1[3], v2[3], q[3];
        for (int k = 0; k < 3; ++k) {
            v0[k] = V[vi[0] * 3LL + k]; v1[k] = V[vi[1] * 3LL + k]; v2[k] = V[vi[2] * 3LL + k];
            q[k] = (b0 * v0[k] + b1 * v1[k]) + b2 * v2[k];
        }
        p = make_float4(q[0], q[1], q[2], __int_as_float(id));
        if (normal) {
            float n[3], e1[3], e2[3], ng[3];
            for (int k = 0; k < 3; ++k) {
                n[k] = (b0 * VN[vi[0] * 3LL + k] + b1 * VN[vi[1] * 3LL + k]) + b2 * VN[vi[2] * 3LL + k];
                e1[k] = v1[k] - v0[k];
                e2[k] = v2[k] - v0[k];
            }
            float len = sqrtf(nu_rl_dot3(n, n));
            if (len > 0.0f && len < 1e30f) {
                for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
            } else {                                                   // nu_rl_surface's fallback: the unit geometric normal; none: zero
                nu_rl_cross(e1, e2, ng);
                len = sqrtf(nu_rl_dot3(ng, ng));
                for (int k = 0; k < 3; ++k) n[k] = (len > 0.0f && len < 1e30f) ? ng[k] / len : 0.0f;
            }
            nq = make_float4(n[0], n[1], n[2], 0.0f);
        }
    }
    texel[r] = p;
    if (normal) normal[r] = nq;
}

// The bilinear lookup at barycentrics (u, v) of face f (0 <= f < nf): out[0..2] albedo, out[3] metallic, out[4] roughness.
// atlas = two planes of T x T float4: (albedo rgb, metallic), then (roughness, spare x 3).  (u, v) is clamped into the triangle, taps and
// fractions are formed in cell-local texel coordinates (so their precision does not depend on T) in the frame of the face, then mapped
// to the atlas.  The mix is t00 + fs (t10 - t00) per row and the same between the rows, a tap whose weight is zero is not part of
// it at all: texels that agree give their value exactly, a corner gives its texel's bits.  With t <= (2 pad + L) - s every tap that
// takes part has i + j <= c - 2 - pad in the face's frame, i.e. belongs to the face.
// nu_atlas_taps / nu_atlas_mix are that lookup's two halves -- where the four taps are, and the mix of one channel -- shared with the
// lookup of the normal lanes below; nu_atlas_lookup is their composition, operation for operation what it was before the split.
struct AtlasTaps {
    long long o00, o10, o01, o11;                                      // texel offsets of the four taps in a plane
    float fs, ft;
};

static __device__ inline AtlasTaps nu_atlas_taps(const AtlasLayout& a, int f, float u, float v) {
    const int k = f >> 1, h = f & 1;
    const int ox = (k % a.cols) * a.c, oy = (k / a.cols) * a.c;
    u = fminf(fmaxf(u, 0.0f), 1.0f);
    v = fminf(fmaxf(v, 0.0f), 1.0f - u);
    const float s = (float)a.pad + u * (float)a.L;
    float t = (float)a.pad + v * (float)a.L;
    t = fminf(t, (float)(2 * a.pad + a.L) - s);
    const float s0 = floorf(s), t0 = floorf(t);
    const int i0 = (int)s0, j0 = (int)t0;
    const int i1 = min(i0 + 1, a.c - 1), j1 = min(j0 + 1, a.c - 1);
    const int x0 = ox + (h ? a.c - 1 - i0 : i0), x1 = ox + (h ? a.c - 1 - i1 : i1);
    const int y0 = oy + (h ? a.c - 1 - j0 : j0), y1 = oy + (h ? a.c - 1 - j1 : j1);
    AtlasTaps p;
    p.o00 = (long long)y0 * a.T + x0; p.o10 = (long long)y0 * a.T + x1; p.o01 = (long long)y1 * a.T + x0; p.o11 = (long long)y1 * a.T + x1;
    p.fs = s - s0; p.ft = t - t0;
    return p;
}

static __device__ inline float nu_atlas_mix(const AtlasTaps& p, float t00, float t10, float t01, float t11) {
    const float lo = p.fs == 0.0f ? t00 : t00 + p.fs * (t10 - t00);
    const float hi = p.fs == 0.0f ? t01 : t01 + p.fs * (t11 - t01);
    return p.ft == 0.0f ? lo : lo + p.ft * (hi - lo);
}

static __device__ inline void nu_atlas_lookup(const float4* __restrict__ atlas, const AtlasLayout& a, int f, float u, float v, float* out) {
    const AtlasTaps p = nu_atlas_taps(a, f, u, v);
    const long long plane = (long long)a.T * a.T;
    const float4 A00 = atlas[p.o00], A10 = atlas[p.o10], A01 = atlas[p.o01], A11 = atlas[p.o11];
    out[0] = nu_atlas_mix(p, A00.x, A10.x, A01.x, A11.x);
    out[1] = nu_atlas_mix(p, A00.y, A10.y, A01.y, A11.y);
    out[2] = nu_atlas_mix(p, A00.z, A10.z, A01.z, A11.z);
    out[3] = nu_atlas_mix(p, A00.w, A10.w, A01.w, A11.w);
    out[4] = nu_atlas_mix(p, atlas[plane + p.o00].x, atlas[plane + p.o10].x, atlas[plane + p.o01].x, atlas[plane + p.o11].x);
}

// The same lookup on the three normal lanes (y, z, w of plane 1: the object-space normal pack_atlas puts there), divided by its length:
// m[0..2] = the unit normal and true, or false (m untouched) when the mix has no length in (0, 1e30) -- a texture without normals, an
// unowned or zero texel, NaN.
static __device__ inline bool nu_atlas_lookup_normal(const float4* __restrict__ atlas, const AtlasLayout& a, int f, float u, float v, float* m) {
    const AtlasTaps p = nu_atlas_taps(a, f, u, v);
    const float4* const nrm = atlas + (long long)a.T * a.T;
    const float4 A00 = nrm[p.o00], A10 = nrm[p.o10], A01 = nrm[p.o01], A11 = nrm[p.o11];
    const float n[3] = {nu_atlas_mix(p, A00.y, A10.y, A01.y, A11.y), nu_atlas_mix(p, A00.z, A10.z, A01.z, A11.z),
                        nu_atlas_mix(p, A00.w, A10.w, A01.w, A11.w)};
    const float len = sqrtf(nu_rl_dot3(n, n));
    if (!(len > 0.0f && len < 1e30f)) return false;
    for (int k = 0; k < 3; ++k) m[k] = n[k] / len;
    return true;
}

__global__ __launch_bounds__(256) void atlas_sample_kernel(const float4* __restrict__ atlas, AtlasLayout a, const int* __restrict__ face,
                                                           const float* __restrict__ uv, int N, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    float o[NU_ATLAS_CH] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < a.nf) nu_atlas_lookup(atlas, a, f, uv[i * 2LL], uv[i * 2LL + 1], o);
    for (int ch = 0; ch < NU_ATLAS_CH; ++ch) out[(long long)i * NU_ATLAS_CH + ch] = o[ch];
}

// One thread per listed hit pixel: barycentrics of the stored hit point in its face (nu_transfer_bary), the lookup, columns 10..14.
__global__ __launch_bounds__(256) void atlas_gbuffer_kernel(float* __restrict__ gbuf, const int* __restrict__ face, const int* __restrict__ pix,
                                                            int n_pix, const float* __restrict__ V, int nv, const int* __restrict__ F,
                                                            const float4* __restrict__ atlas, AtlasLayout a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const long long row = pix[i];
    const int f = face[row];
    if (f < 0 || f >= a.nf) return;                                    // a miss row (NU_RL_MISS) that was listed: left as it is
    const int i0 = F[f * 3LL], i1 = F[f * 3LL + 1], i2 = F[f * 3LL + 2];
    if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) return;
    float* g = gbuf + row * NU_RL_ROW;
    float x[3], v0[3], v1[3], v2[3], u, v, o[NU_ATLAS_CH];
    for (int k = 0; k < 3; ++k) { x[k] = g[1 + k]; v0[k] = V[i0 * 3LL + k]; v1[k] = V[i1 * 3LL + k]; v2[k] = V[i2 * 3LL + k]; }
    nu_transfer_bary(x, v0, v1, v2, u, v);
    nu_atlas_lookup(atlas, a, f, u, v, o);
    for (int ch = 0; ch < NU_ATLAS_CH; ++ch) g[10 + ch] = o[ch];
}

__global__ __launch_bounds__(256) void atlas_sample_normal_kernel(const float4* __restrict__ atlas, AtlasLayout a, const int* __restrict__ face,
                                                                  const float* __restrict__ uv, int N, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < a.nf) nu_atlas_lookup_normal(atlas, a, f, uv[i * 2LL], uv[i * 2LL + 1], o);
    for (int k = 0; k < 3; ++k) out[i * 3LL + k] = o[k];
}

// One thread per listed hit pixel: atlas_gbuffer_kernel's barycentrics, the normal lookup, columns 7..9 -- on the side of the
// viewer-facing geometric normal (columns 4..6), nu_rl_surface's rule for the vertex normals.  No normal there: the row keeps its own.
__global__ __launch_bounds__(256) void atlas_gbuffer_normal_kernel(float* __restrict__ gbuf, const int* __restrict__ face,
                                                                   const int* __restrict__ pix, int n_pix, const float* __restrict__ V, int nv,
                                                                   const int* __restrict__ F, const float4* __restrict__ atlas, AtlasLayout a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const long long row = pix[i];
    const int f = face[row];
    if (f < 0 || f >= a.nf) return;
    const int i0 = F[f * 3LL], i1 = F[f * 3LL + 1], i2 = F[f * 3LL + 2];
    if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) return;
    float* g = gbuf + row * NU_RL_ROW;
    float x[3], v0[3], v1[3], v2[3], ng[3], ns[3], u, v;
    for (int k = 0; k < 3; ++k) { x[k] = g[1 + k]; ng[k] = g[4 + k]; v0[k] = V[i0 * 3LL + k]; v1[k] = V[i1 * 3LL + k]; v2[k] = V[i2 * 3LL + k]; }
    nu_transfer_bary(x, v0, v1, v2, u, v);
    if (!nu_atlas_lookup_normal(atlas, a, f, u, v, ns)) return;
    const bool flip = nu_rl_dot3(ns, ng) < 0.0f;
    for (int k = 0; k < 3; ++k) g[7 + k] = flip ? -ns[k] : ns[k];
}

extern "C" int nu_atlas_texels(const float* V, int n_verts, const int* F, int n_faces, const float* vnormals, int size, int pad, int y0,
                               int rows, float* texel, float* normal, hipStream_t stream) {
    AtlasLayout a;
    if (!nu_atlas_layout(n_faces, size, pad, a) || n_verts < 1 || y0 < 0 || rows < 0 || (long long)y0 + rows > size) return NU_ERR_ARG;
    if ((vnormals == nullptr) != (normal == nullptr)) return NU_ERR_ARG;
    if (rows == 0) return NU_OK;
    if (!V || !F || !texel) return NU_ERR_ARG;
    hipLaunchKernelGGL(atlas_texels_kernel, dim3(nu_cdiv(size, 256), rows), dim3(256), 0, stream, V, n_verts, F, vnormals, a, y0,
                       (float4*)texel, (float4*)normal);
    return nu_launch_status();
}

extern "C" int nu_atlas_sample(const float* atlas, int size, int n_faces, int pad, const int* face, const float* uv, int n, float* out,
                               hipStream_t stream) {
    AtlasLayout a;
    if (!nu_atlas_layout(n_faces, size, pad, a) || n < 0) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    if (!atlas || !face || !uv || !out) return NU_ERR_ARG;
    hipLaunchKernelGGL(atlas_sample_kernel, dim3(nu_cdiv(n, 256)), dim3(256), 0, stream, (const float4*)atlas, a, face, uv, n, out);
    return nu_launch_status();
}

extern "C" int nu_atlas_gbuffer(float* gbuf, const int* face, const int* pix, int n_pix, const float* V, int n_verts, const int* F,
                                int n_faces, const float* atlas, int size, int pad, hipStream_t stream) {
    AtlasLayout a;
    if (!nu_atlas_layout(n_faces, size, pad, a) || n_verts < 1 || n_pix < 0) return NU_ERR_ARG;
    if (!gbuf || !face || (n_pix > 0 && !pix) || !V || !F || !atlas) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    hipLaunchKernelGGL(atlas_gbuffer_kernel, dim3(nu_cdiv(n_pix, 256)), dim3(256), 0, stream, gbuf, face, pix, n_pix, V, n_verts, F,
                       (const float4*)atlas, a);
    return nu_launch_status();
}

extern "C" int nu_atlas_sample_normal(const float* atlas, int size, int n_faces, int pad, const int* face, const float* uv, int n, float* out,
                                      hipStream_t stream) {
    AtlasLayout a;
    if (!nu_atlas_layout(n_faces, size, pad, a) || n < 0) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    if (!atlas || !face || !uv || !out) return NU_ERR_ARG;
    hipLaunchKernelGGL(atlas_sample_normal_kernel, dim3(nu_cdiv(n, 256)), dim3(256), 0, stream, (const float4*)atlas, a, face, uv, n, out);
    return nu_launch_status();
}

extern "C" int nu_atlas_gbuffer_normal(float* gbuf, const int* face, const int* pix, int n_pix, const float* V, int n_verts, const int* F,
                                       int n_faces, const float* atlas, int size, int pad, hipStream_t stream) {
    AtlasLayout a;
    if (!nu_atlas_layout(n_faces, size, pad, a) || n_verts < 1 || n_pix < 0) return NU_ERR_ARG;
    if (!gbuf || !face || (n_pix > 0 && !pix) || !V || !F || !atlas) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    hipLaunchKernelGGL(atlas_gbuffer_normal_kernel, dim3(nu_cdiv(n_pix, 256)), dim3(256), 0, stream, gbuf, face, pix, n_pix, V, n_verts, F,
                       (const float4*)atlas, a);
    return nu_launch_status();
}
