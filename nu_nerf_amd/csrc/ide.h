// ide.h -- device helpers of the input encodings that more than one translation unit evaluates: the positional-embedding column,
// the integrated directional encoding (one lane per term) and the bounding-sphere point of a ray.  Moved verbatim out of encode.hip
// for csrc/light_bake.hip; the arithmetic is that of the encoding kernels, so rows built here carry their bits.
#pragma once
#include "nu_common.h"
#include "ide_table.h"

// column -> (is_raw, k, coord, is_cos) for an L-frequency embedding of a D-vector:
// col < D : x[col];  else q = col - D, k = q / (2D), r = q % (2D), c = r % D, cos if r >= D
static __device__ inline float nu_embed_col(const float* x, int D, int col) {
    if (col < D) return x[col];
    const int q = col - D;
    const int k = q / (2 * D);
    const int r = q - k * 2 * D;
    const int c = r >= D ? r - D : r;
    const float a = x[c] * (float)(1 << k);
    return r >= D ? cosf(a) : sinf(a);
}

// ------------------------------------------------------------------------------------------------
// IDE: lane i < 36 evaluates term i.  Returns (re, im) and optionally the partials.
// ------------------------------------------------------------------------------------------------
// Per-lane constants of term i = lane (loaded once per kernel: the Horner loop then runs out of registers with a uniform
// trip count -- coefficients above degree l - m are zero in the table, and leading zeros leave Horner's arithmetic unchanged)
struct NuIdeLane {
    float c[NU_IDE_DEG];
    float sigma, att1;     // l(l+1)/2 and exp(-sigma) (kappa_inv = 1: the diffuse query)
    int m;
    bool live;
};
static __device__ inline NuIdeLane nu_ide_lane(int lane) {
    NuIdeLane L;
    const int i = lane < NU_IDE_TERMS ? lane : NU_IDE_TERMS - 1;
#pragma unroll
    for (int k = 0; k < NU_IDE_DEG; ++k) L.c[k] = c_ide_mat[i][k];
    const int l = c_ide_l[i];
    L.m = c_ide_m[i];
    L.sigma = 0.5f * (float)l * (float)(l + 1);
    L.att1 = expf(-L.sigma);
    L.live = lane < NU_IDE_TERMS;
    return L;
}
// Direction-dependent factors of one term, shared by every kappa the direction is queried with
struct NuIdeDir {
    float are, aim;        // (x+iy)^m
    float pre, pim;        // (x+iy)^(m-1)   (0 for m = 0)
    float poly, dpoly;     // P(z), P'(z)
};
static __device__ inline NuIdeDir nu_ide_dir(const NuIdeLane& L, float x, float y, float z) {
    NuIdeDir t;
    float ar = 1.f, ai = 0.f, pr = 0.f, pi = 0.f;
#pragma unroll
    for (int j = 0; j < NU_IDE_DEG - 1; ++j) {
        if (j < L.m) {
            pr = ar; pi = ai;
            const float nr = ar * x - ai * y;
            const float ni = ar * y + ai * x;
            ar = nr; ai = ni;
        }
    }
    float poly = 0.f, dpoly = 0.f;
#pragma unroll
    for (int k = NU_IDE_DEG - 1; k >= 0; --k) {
        dpoly = dpoly * z + poly;
        poly = poly * z + L.c[k];
    }
    t.are = ar; t.aim = ai; t.pre = pr; t.pim = pi; t.poly = poly; t.dpoly = dpoly;
    return t;
}
static __device__ inline float nu_ide_att(const NuIdeLane& L, float kinv) { return expf(-L.sigma * kinv); }

// write one 72-d IDE row (+ zero pad up to `padto` columns) given the direction factors and the attenuation
static __device__ inline void nu_ide_store(float* row, int lane, const NuIdeLane& L, const NuIdeDir& t, float att, int padto) {
    if (L.live) {
        row[lane] = t.are * t.poly * att;
        row[36 + lane] = t.aim * t.poly * att;
    }
    for (int c = 72 + lane; c < padto; c += 64) row[c] = 0.f;
}

// Point on the unit sphere seen from p (inside, moved to radius 0.999 when outside) along `dir`
// (offset_points_to_sphere + get_sphere_intersection + normalize; field.py:447-464, :642-643, :676-677)
struct NuSph {
    float s[3];       // unit point on the sphere
    float pp[3];      // offset origin p'
    float t, root, snorm;
};
// |x|^2 with its fused step written out, fma(x0, x0, x1 x1) + x2 x2: the shape hipcc gives the sum of nu_sph_point in the encoding kernels
static __device__ inline float nu_sph_norm2(const float* x) {
#pragma clang fp contract(off)
    return __builtin_fmaf(x[0], x[0], x[1] * x[1]) + x[2] * x[2];
}
// n2 = |x|^2 as the caller rounds it.  Points beyond radius 0.999 are scaled by 0.999 / |x|, so rows of two kernels carry each other's
// bits only if both round |x|^2 alike.  nu_sph_point leaves the contraction of that sum to the compiler, which chooses per kernel; a
// kernel in which it chooses otherwise than the encoding kernels (csrc/light_bake.hip on fm_layer: fma(x2, x2, fma(x1, x1, x0 x0)))
// passes nu_sph_norm2(x) here.
static __device__ inline NuSph nu_sph_point_n2(const float* x, const float* dir, float n2) {
    NuSph o;
    const float xn = sqrtf(n2);
    const float sc = xn > 0.999f ? 0.999f / xn : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.pp[c] = xn > 0.999f ? x[c] / xn * 0.999f : x[c];
    (void)sc;
    const float b = o.pp[0] * dir[0] + o.pp[1] * dir[1] + o.pp[2] * dir[2];
    const float cc = o.pp[0] * o.pp[0] + o.pp[1] * o.pp[1] + o.pp[2] * o.pp[2];
    o.root = sqrtf(b * b - cc + 1.0f + 1e-6f);
    o.t = -b + o.root;
    float sv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sv[c] = o.pp[c] + dir[c] * o.t;
    o.snorm = fmaxf(sqrtf(sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2]), 1e-12f);
#pragma unroll
    for (int c = 0; c < 3; ++c) o.s[c] = sv[c] / o.snorm;
    return o;
}
static __device__ inline NuSph nu_sph_point(const float* x, const float* dir) {
    return nu_sph_point_n2(x, dir, x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
}
