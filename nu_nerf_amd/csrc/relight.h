// relight.h -- the device functions the relighting kernels share: the G-buffer row, the per-pixel sample sequence, the
// shadow ray of a (pixel, sample), the lat-long environment lookup and the BRDF weight.  Included by lbvh.hip (the two traced passes
// instantiate the traversal template there: the library is built without relocatable device code) and by relight.hip (resolve and the
// debug entries).  ONE definition of each, compiled under the same flags with FMA contraction off, so that the ray the visibility pass
// traces, the ray nu_relight_shadow_rays dumps and the direction nu_relight_resolve shades are the same bits.
// Further down: the nested object (nu_rl_surface, nu_rln_interface, nu_rln_leave -- a solid glass shell, one interface) and
// the thin shell (nu_rlt_cross, nu_rlt_leave -- the wall crossing of the non-zero-thickness stage-2 model, the geometry of
// s2_shell_core in stage2.hip restated after its sigmoids, with a Schlick factor per face).  At the end: visibility transfer
// (the hemisphere samples of a surface point, its transfer row, the row at a hit point, specular occlusion).
#pragma once
#include "nu_common.h"

#pragma clang fp contract(off)

// G-buffer row of a pixel: NU_RL_ROW floats.  A miss pixel has face = NU_RL_MISS in the face array and an all-zero row.
//   [0] t   [1..3] hit point   [4..6] geometric normal   [7..9] shading normal   [10..12] albedo   [13] metallic   [14] roughness
//   [15..17] view vector (unit, surface -> camera)   [18] image index   [19] pixel index y * w + x of the full frame (both int bits)
// Both normals are unit; the geometric one faces the viewer, the shading one lies on the geometric one's side.
#define NU_RL_ROW 20
#define NU_RL_MISS 10000000
#define NU_RL_ALPHA_MIN 1e-3f        // GGX alpha = max(roughness^2, NU_RL_ALPHA_MIN)
#define NU_RL_NOV_MIN 1e-4f          // N.V of the specular weight is clamped from below (silhouette pixels of a smooth-shaded mesh)

static __device__ inline unsigned nu_rl_fmix32(unsigned h) {        // MurmurHash3's 32-bit finaliser
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// Sample s of S (S even) of a pixel: s < S/2 is index j = s of the S/2 cosine-weighted diffuse directions, s >= S/2 index j = s - S/2 of
// the S/2 GGX half vectors.  Hammersley point (j / M, bit-reversed j), M = S/2, as 32-bit fixed point; Cranley-Patterson shift = two hash
// words of (image, pixel, seed, lobe) added modulo 2^32; the two uniforms are the top 24 bits (exact in fp32).  Integer arithmetic up
// to bits[0], bits[1].
static __device__ inline void nu_relight_uniforms(int img, int pixel, unsigned seed, int S, int s, int& lobe, unsigned* bits) {
    const int M = S >> 1;
    lobe = s >= M ? 1 : 0;
    const unsigned j = (unsigned)(s - lobe * M);
    const unsigned x1 = (unsigned)(((unsigned long long)j << 32) / (unsigned long long)M);
    const unsigned x2 = __brev(j);
    unsigned a = nu_rl_fmix32((unsigned)img + 0x9E3779B9u);
    a = nu_rl_fmix32(a ^ (unsigned)pixel);
    a = nu_rl_fmix32(a ^ seed);
    const unsigned h1 = nu_rl_fmix32(a + 2u * (unsigned)lobe + 1u);
    const unsigned h2 = nu_rl_fmix32(h1 ^ 0x68E31DA4u);
    bits[0] = (x1 + h1) >> 8;
    bits[1] = (x2 + h2) >> 8;
}

// Orthonormal tangent frame of a unit normal (Duff et al. 2017, "Building an Orthonormal Basis, Revisited").
static __device__ inline void nu_rl_frame(const float* n, float* t, float* b) {
    const float sg = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sg + n[2]);
    const float c = n[0] * n[1] * a;
    t[0] = 1.0f + sg * n[0] * n[0] * a; t[1] = sg * c; t[2] = -sg * n[0];
    b[0] = c; b[1] = sg + n[1] * n[1] * a; b[2] = -n[1];
}

// Light direction l (and, for the specular lobe, the half vector hv) of sample s of the pixel whose G-buffer row is g.  Returns true when
// the sample is traced: l above the shading AND the geometric horizon (and V.H > 0 for a specular sample).  A sample that is not
// traced counts as dark.
static __device__ inline bool nu_relight_sample(const float* g, int S, int s, unsigned seed, int& lobe, float* l, float* hv,
                                                unsigned* bits) {
    nu_relight_uniforms(__float_as_int(g[18]), __float_as_int(g[19]), seed, S, s, lobe, bits);
    const float u1 = (float)bits[0] * 5.9604644775390625e-08f, u2 = (float)bits[1] * 5.9604644775390625e-08f;   // 2^-24
    const float* ng = g + 4;
    const float* ns = g + 7;
    const float* v = g + 15;
    float t[3], b[3];
    nu_rl_frame(ns, t, b);
    float sp, cp;
    sincosf(6.283185307179586f * u1, &sp, &cp);
    float ct, st;
    if (lobe == 0) {
        ct = sqrtf(1.0f - u2);
        st = sqrtf(u2);
    } else {
        const float a = fmaxf(g[14] * g[14], NU_RL_ALPHA_MIN);
        const float om = 1.0f - u2;                              // exact: u2 is a multiple of 2^-24
        const float den = om + (a * a) * u2;                     // cos^2 = (1 - u2) / (1 + (a^2 - 1) u2), written so that neither it
        ct = sqrtf(om / den);                                    // nor sin^2 = 1 - cos^2 cancels
        st = sqrtf((a * a) * u2 / den);
    }
    const float lx = st * cp, ly = st * sp;
    float w[3];
    for (int k = 0; k < 3; ++k) w[k] = (lx * t[k] + ly * b[k]) + ct * ns[k];
    bool ok = true;
    if (lobe == 0) {
        for (int k = 0; k < 3; ++k) { l[k] = w[k]; hv[k] = 0.0f; }
    } else {
        const float voh = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
        for (int k = 0; k < 3; ++k) { hv[k] = w[k]; l[k] = 2.0f * voh * w[k] - v[k]; }
        ok = voh > 0.0f;
    }
    const float nsl = (ns[0] * l[0] + ns[1] * l[1]) + ns[2] * l[2];
    const float ngl = (ng[0] * l[0] + ng[1] * l[1]) + ng[2] * l[2];
    return ok && nsl > 0.0f && ngl > 0.0f;
}

// The shadow ray of (pixel row g, sample s): origin = hit point + eps * geometric normal, direction = the sample's l.
static __device__ inline bool nu_relight_shadow_ray(const float* g, int S, int s, unsigned seed, float eps, float* o, float* d,
                                                    unsigned* bits) {
    int lobe;
    float hv[3];
    const bool traced = nu_relight_sample(g, S, s, seed, lobe, d, hv, bits);
    for (int k = 0; k < 3; ++k) o[k] = g[1 + k] + eps * g[4 + k];
    return traced;
}

// ---- the nested object: a transparent outer shell with a per-vertex index of refraction around an opaque inner mesh ----
static __device__ inline float nu_rl_dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static __device__ inline void nu_rl_cross(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// What nu_relight_gbuffer derives at a hit, for the hit of ray (o, d) with face `id` at distance t: the point x, the unit geometric
// normal ng facing the viewer (against d), the unit interpolated normal ns on ng's side (same degenerate fallbacks), the vertex ids
// and the barycentric weights bary = (w0, u, v) -- the operations of the ray / triangle test in its order.
static __device__ inline void nu_rl_surface(const float* __restrict__ V, const int* __restrict__ F, const float* __restrict__ VN,
                                            const float* o, const float* d, int id, float t, float* x, float* ng, float* ns, int* vi,
                                            float* bary) {
    vi[0] = F[id * 3LL]; vi[1] = F[id * 3LL + 1]; vi[2] = F[id * 3LL + 2];
    float v0[3], e1[3], e2[3], pv[3], tv[3], qv[3], view[3];
    for (int k = 0; k < 3; ++k) {
        v0[k] = V[vi[0] * 3LL + k];
        e1[k] = V[vi[1] * 3LL + k] - v0[k];
        e2[k] = V[vi[2] * 3LL + k] - v0[k];
        view[k] = -d[k];
    }
    nu_rl_cross(d, e2, pv);
    const float inv = 1.0f / nu_rl_dot3(e1, pv);
    for (int k = 0; k < 3; ++k) tv[k] = o[k] - v0[k];
    const float u = nu_rl_dot3(tv, pv) * inv;
    nu_rl_cross(tv, e1, qv);
    const float v = nu_rl_dot3(d, qv) * inv;
    const float w0 = (1.0f - u) - v;
    nu_rl_cross(e1, e2, ng);
    float len = sqrtf(nu_rl_dot3(ng, ng));
    if (len > 0.0f) { for (int k = 0; k < 3; ++k) ng[k] = ng[k] / len; }
    else { for (int k = 0; k < 3; ++k) ng[k] = view[k]; }
    if (nu_rl_dot3(ng, view) < 0.0f) { for (int k = 0; k < 3; ++k) ng[k] = -ng[k]; }
    for (int k = 0; k < 3; ++k) ns[k] = (w0 * VN[vi[0] * 3LL + k] + u * VN[vi[1] * 3LL + k]) + v * VN[vi[2] * 3LL + k];
    len = sqrtf(nu_rl_dot3(ns, ns));
    if (len > 0.0f && len < 1e30f) { for (int k = 0; k < 3; ++k) ns[k] = ns[k] / len; }
    else { for (int k = 0; k < 3; ++k) ns[k] = ng[k]; }
    if (nu_rl_dot3(ns, ng) < 0.0f) { for (int k = 0; k < 3; ++k) ns[k] = -ns[k]; }
    for (int k = 0; k < 3; ++k) x[k] = o[k] + t * d[k];
    bary[0] = w0; bary[1] = u; bary[2] = v;
}

// The interface event of direction d (unit) at a point of the outer mesh with unit shading normal ns and index of refraction ior >= 1,
// entering from air (eta = 1 / ior) or leaving (eta = ior).  n = ns oriented against d; cos_i = -n.d; total internal reflection exactly
// as the stage-2 model was trained (s2_refract_fwd_kernel): no refraction when eta^2 sin^2_i > 0.999.  Returns true when the ray
// refracts: dn = eta d + (eta cos_i - sqrt(1 - eta^2 sin^2_i)) n, renormalised; fres = Schlick, F0 + (1 - F0)(1 - c)^5 with
// F0 = ((ior - 1) / (ior + 1))^2 and c the cosine on the AIR side (cos_i entering, the refracted cosine leaving), which makes a
// crossing reciprocal.  F0 = 0 (ior = 1, an index-matched interface) reflects nothing: fres = 0.  Returns false on total internal
// reflection: dn = d + 2 cos_i n, fres = 1 (0 when F0 = 0).
static __device__ inline bool nu_rln_interface(const float* d, const float* ns, float ior, bool entering, float* n, float* dn,
                                               float& fres) {
    const float sg = nu_rl_dot3(ns, d) > 0.0f ? -1.0f : 1.0f;
    for (int k = 0; k < 3; ++k) n[k] = sg * ns[k];
    const float cos_i = -nu_rl_dot3(n, d);
    const float sin2_i = 1.0f - cos_i * cos_i;
    const float eta = entering ? 1.0f / ior : ior;
    const float k2 = eta * eta * sin2_i;
    const float r = (ior - 1.0f) / (ior + 1.0f), f0 = r * r;
    if (k2 > 0.999f) {
        for (int k = 0; k < 3; ++k) dn[k] = d[k] + (2.0f * cos_i) * n[k];
        fres = f0 > 0.0f ? 1.0f : 0.0f;
        return false;
    }
    const float cos_t = sqrtf(1.0f - k2);
    const float f = eta * cos_i - cos_t;
    float tv[3];
    for (int k = 0; k < 3; ++k) tv[k] = eta * d[k] + f * n[k];
    const float len = sqrtf(nu_rl_dot3(tv, tv));
    for (int k = 0; k < 3; ++k) dn[k] = tv[k] / len;
    const float m = fmaxf(1.0f - (entering ? cos_i : cos_t), 0.0f);
    fres = f0 > 0.0f ? f0 + (1.0f - f0) * ((m * m) * (m * m) * m) : 0.0f;
    return true;
}

// The mirror direction of the entry event: reflect(d, n) = d - 2 (n.d) n for the oriented normal n.
static __device__ inline void nu_rln_reflect(const float* d, const float* n, float* r) {
    const float c = -nu_rl_dot3(n, d);
    for (int k = 0; k < 3; ++k) r[k] = d[k] + (2.0f * c) * n[k];
}

// Light path of a sample, second half: the ray (o, d) from the inner object met face `id` of the outer mesh at distance t from inside.
// Returns true when it refracts: (o2, d2) is the exit ray -- the hit point pushed eps along the OUTWARD geometric normal, the refracted
// direction -- and keep = 1 - F_exit.  Returns false on total internal reflection: (o2, d2) is the mirrored ray restarted eps on the
// INSIDE of the hit point (the interior chain goes on with it; a light path takes no interior bounce and is dark).
static __device__ inline bool nu_rln_leave(const float* __restrict__ V, const int* __restrict__ F, const float* __restrict__ VN,
                                                const float* __restrict__ ior, const float* o, const float* d, int id, float t,
                                                float eps, float* o2, float* d2, float& keep) {
    float x[3], ng[3], ns[3], n[3], bary[3], fres;
    int vi[3];
    nu_rl_surface(V, F, VN, o, d, id, t, x, ng, ns, vi, bary);
    // the excess over 1 is what is interpolated (as the G-buffer pass does for the primary hit): a constant index stays that index, bit for bit
    const float index = 1.0f + ((bary[0] * (ior[vi[0]] - 1.0f) + bary[1] * (ior[vi[1]] - 1.0f)) + bary[2] * (ior[vi[2]] - 1.0f));
    const bool refr = nu_rln_interface(d, ns, index, false, n, d2, fres);
    for (int k = 0; k < 3; ++k) o2[k] = refr ? x[k] - eps * ng[k] : x[k] + eps * ng[k];
    keep = 1.0f - fres;
    return refr;
}

// ---- the thin shell: the non-zero-thickness stage-2 model -- a glass wall of thickness th around an air-like cavity ----
#define NU_RLT_CAVITY 1.0001f        // index of the cavity behind the wall (the trained model's inner medium is 1 / 1.0001)

// Schlick reflectance of one face between the media of index n_in (cosine c_in on that side) and n_out (cosine c_out): F0 =
// ((n_in - n_out) / (n_in + n_out))^2, the cosine of the LOWER-index side (so the factor does not depend on the direction of travel),
// F0 = 0 -> 0.  The trained geometry does not orient its normals by the ray, so a cosine may be negative: 1 - c is clamped to [0, 1].
static __device__ inline float nu_rlt_schlick(float n_in, float n_out, float c_in, float c_out) {
    const float r = (n_in - n_out) / (n_in + n_out), f0 = r * r;
    const float m = fminf(fmaxf(1.0f - (n_in <= n_out ? c_in : c_out), 0.0f), 1.0f);
    return f0 > 0.0f ? f0 + (1.0f - f0) * ((m * m) * (m * m) * m) : 0.0f;
}
// x / (|x| + 1e-4), as the trained model normalises
static __device__ inline void nu_rlt_unit_eps(float* x) {
    const float inv = 1.0f / (sqrtf(nu_rl_dot3(x, x)) + 0.0001f);
    for (int k = 0; k < 3; ++k) x[k] = x[k] * inv;
}

// The crossing of the wall by direction d (unit) at the mesh point x: s2_shell_core<float> of stage2.hip after its two sigmoids, operation
// for operation (r = 1 / n_g, inner medium 1 / 1.0001, th as given), compiled here without FMA contraction.  nraw = the OUTWARD shading
// normal (any length; flipped when inside), n_g the glass index, th the wall thickness, gk the Gaussian curvature: the wall at x is two
// concentric spheres of radius R = 1 / sqrt(max(|gk|, 1e-6)), th apart.  inside = false: air -> glass at x -> cavity; inside = true:
// cavity -> glass at the inner sphere (the step back from x) -> air.  Outputs: refracts (the first test, eta^2 sin^2_i <= 0.999 with the
// mesh normal), tir_ok (no later face reflects totally either), nrm = the oriented unit normal at x, pend = the point of the first
// face, (ns, nd) = the ray behind the wall (zero when !refracts), f_a / f_b = Schlick of the first / second face (nu_rlt_schlick;
// !refracts: f_a = 1, or 0 for index-matched media, f_b = 0).  A path goes on only when refracts && tir_ok.
static __device__ inline void nu_rlt_cross(const float* d, const float* x, const float* nraw, float n_g, float th, float gk, bool inside,
                                          bool& refracts, bool& tir_ok, float* nrm, float* pend, float* ns, float* nd, float& f_a,
                                          float& f_b) {
    {
        const float inv = 1.0f / fmaxf(sqrtf(nu_rl_dot3(nraw, nraw)), 1e-12f);
        for (int k = 0; k < 3; ++k) nrm[k] = inside ? -(nraw[k] * inv) : nraw[k] * inv;
    }
    float r = 1.0f / n_g;
    const float inner = 1.0f / 1.0001f;
    float ro = inner / r;
    if (inside) { const float tmp = r; r = 1.0f / ro; ro = 1.0f / tmp; }
    const float n_first_in = inside ? NU_RLT_CAVITY : 1.0f, n_last_out = inside ? 1.0f : NU_RLT_CAVITY;
    const float cos_i = -nu_rl_dot3(nrm, d);
    const float sin2_i = 1.0f - cos_i * cos_i;
    refracts = !(r * r * sin2_i > 0.999f);
    tir_ok = refracts;
    for (int k = 0; k < 3; ++k) { pend[k] = x[k]; ns[k] = 0.0f; nd[k] = 0.0f; }
    f_b = 0.0f;
    if (!refracts) {
        const float q = (n_first_in - n_g) / (n_first_in + n_g);
        f_a = q * q > 0.0f ? 1.0f : 0.0f;
        return;
    }
    const float sin2_t = sin2_i * r * r;
    float R = 1.0f / sqrtf(fmaxf(fabsf(gk), 0.000001f));
    if (R != R) R = 0.1f;
    const float cos_t = sqrtf(fmaxf(1.0f - sin2_t, 0.0001f));
    const bool positive = inside ? (gk <= 0.0f) : (gk >= 0.0f);
    const float two_R_th = R * th * 2.0f, th2 = th * th;
    float pm[3], nm[3], din[3];
    if (!inside) {
        const float f = r * cos_i - cos_t;
        for (int k = 0; k < 3; ++k) { din[k] = r * d[k] + f * nrm[k]; pm[k] = x[k]; nm[k] = nrm[k]; }
        nu_rlt_unit_eps(din);
        f_a = nu_rlt_schlick(n_first_in, n_g, cos_i, cos_t);
    } else {
        const float ci = R * cos_i;
        const float delta2 = positive ? (ci * ci - two_R_th + th2) : (ci * ci + two_R_th + th2);
        const float len = fabsf(ci - sqrtf(fmaxf(delta2, 0.0001f)));
        for (int k = 0; k < 3; ++k) {
            const float center = positive ? (x[k] - nrm[k] * R) : (x[k] + nrm[k] * R);
            pm[k] = x[k] - len * d[k];
            nm[k] = positive ? (pm[k] - center) : (center - pm[k]);
            pend[k] = pm[k];
        }
        nu_rlt_unit_eps(nm);
        const float cos_im = -nu_rl_dot3(nm, d);
        const float xx = (1.0f - cos_im * cos_im) * r * r;
        if (xx > 0.999f) tir_ok = false;
        const float cos_tm = sqrtf(fmaxf(1.0f - fminf(xx, 0.999f), 0.0001f));
        const float f = r * cos_im - cos_tm;
        for (int k = 0; k < 3; ++k) din[k] = r * d[k] + f * nm[k];
        nu_rlt_unit_eps(din);
        f_a = nu_rlt_schlick(n_first_in, n_g, cos_im, cos_tm);
    }
    // the chord through the wall and the second face
    const float cr = R * cos_t;
    const float delta2 = positive ? (cr * cr - two_R_th + th2) : (cr * cr + two_R_th + th2);
    const float len = fabsf(cr - sqrtf(fmaxf(delta2, 0.0001f))) + 0.001f;
    float na[3];
    for (int k = 0; k < 3; ++k) {
        const float center = positive ? (pm[k] - nm[k] * R) : (pm[k] + nm[k] * R);
        ns[k] = pm[k] + din[k] * len;
        na[k] = positive ? (ns[k] - center) : (center - ns[k]);
    }
    nu_rlt_unit_eps(na);
    const float cos_i2 = -nu_rl_dot3(na, din);
    const float x2 = (1.0f - cos_i2 * cos_i2) * ro * ro;
    if (x2 > 0.999f) tir_ok = false;
    const float cos_t2 = sqrtf(fmaxf(1.0f - fminf(x2, 0.999f), 0.0001f));
    const float f2 = ro * cos_i2 - cos_t2;
    for (int k = 0; k < 3; ++k) nd[k] = ro * din[k] + f2 * na[k];
    nu_rlt_unit_eps(nd);
    f_b = nu_rlt_schlick(n_g, n_last_out, cos_i2, cos_t2);
}

// A ray (o, d) of the cavity met face `id` of the outer mesh at distance t: the leaving crossing with index, thickness and curvature
// interpolated from the per-vertex arrays by the barycentrics of the hit (the index as 1 + sum w (n - 1), like the primary hit).  Returns
// true when the ray gets out: (o2, d2) = the ray behind the wall, its origin pushed eps along the OUTWARD geometric normal, and
// keep = (1 - F_a)(1 - F_b).  Returns false when any face reflects totally: the path is dark (no interior bounce is modelled).
static __device__ inline bool nu_rlt_leave(const float* __restrict__ V, const int* __restrict__ F, const float* __restrict__ VN,
                                          const float* __restrict__ ior, const float* __restrict__ thick, const float* __restrict__ curv,
                                          const float* o, const float* d, int id, float t, float eps, float* o2, float* d2, float& keep) {
    float x[3], ng[3], nsh[3], bary[3], nout[3], nrm[3], pend[3], f_a, f_b;
    int vi[3];
    nu_rl_surface(V, F, VN, o, d, id, t, x, ng, nsh, vi, bary);
    const float index = 1.0f + ((bary[0] * (ior[vi[0]] - 1.0f) + bary[1] * (ior[vi[1]] - 1.0f)) + bary[2] * (ior[vi[2]] - 1.0f));
    const float th = (bary[0] * thick[vi[0]] + bary[1] * thick[vi[1]]) + bary[2] * thick[vi[2]];
    const float gk = (bary[0] * curv[vi[0]] + bary[1] * curv[vi[1]]) + bary[2] * curv[vi[2]];
    for (int k = 0; k < 3; ++k) nout[k] = -nsh[k];           // nu_rl_surface's shading normal faces the ray: the outward one is its negative
    bool refr, ok;
    nu_rlt_cross(d, x, nout, index, th, gk, true, refr, ok, nrm, pend, o2, d2, f_a, f_b);
    for (int k = 0; k < 3; ++k) o2[k] = o2[k] - eps * ng[k];
    keep = (1.0f - f_a) * (1.0f - f_b);
    return refr && ok;
}

// Lat-long environment, z up: column u = (1/2 - atan2(d.y, d.x) / 2 pi) * W, row v = atan2(hypot(d.x, d.y), d.z) / pi * H (row 0 = +z);
// texel centres at half-integers, bilinear, wrapping in u and clamping in v.  env = RGBA fp32 [H, W]: a tap is one 16-byte load.
static __device__ inline void nu_relight_env(const float4* __restrict__ env, int eh, int ew, const float* d, float* rgb) {
    const float phi = atan2f(d[1], d[0]);
    const float theta = atan2f(sqrtf(d[0] * d[0] + d[1] * d[1]), d[2]);
    const float fx = (0.5f - phi * 0.15915494309189535f) * (float)ew - 0.5f;
    const float fy = theta * 0.3183098861837907f * (float)eh - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float ax = fx - x0, ay = fy - y0;
    int ix0 = (int)x0 % ew;
    if (ix0 < 0) ix0 += ew;
    const int ix1 = ix0 + 1 == ew ? 0 : ix0 + 1;
    const int iy0 = min(max((int)y0, 0), eh - 1), iy1 = min(max((int)y0 + 1, 0), eh - 1);
    const float4 t00 = env[(long long)iy0 * ew + ix0], t01 = env[(long long)iy0 * ew + ix1];
    const float4 t10 = env[(long long)iy1 * ew + ix0], t11 = env[(long long)iy1 * ew + ix1];
    const float bx = 1.0f - ax, by = 1.0f - ay;
    rgb[0] = by * (bx * t00.x + ax * t01.x) + ay * (bx * t10.x + ax * t11.x);
    rgb[1] = by * (bx * t00.y + ax * t01.y) + ay * (bx * t10.y + ax * t11.y);
    rgb[2] = by * (bx * t00.z + ax * t01.z) + ay * (bx * t10.z + ax * t11.z);
}

// Separable Smith masking of GGX: G1(x) = 2 x / (x + sqrt(a^2 + (1 - a^2) x^2)).
static __device__ inline float nu_rl_g1(float x, float a2) { return 2.0f * x / (x + sqrtf(a2 + (1.0f - a2) * x * x)); }

// Weight of a traced sample (estimator / pdf, without visibility and radiance): diffuse (1 - metallic) * albedo for a cosine-weighted
// direction; specular F G (V.H) / ((N.V) (N.H)) for an NDF-sampled half vector, F = Schlick with F0 = lerp(0.04, albedo, metallic).
static __device__ inline void nu_relight_weight(const float* g, int lobe, const float* l, const float* hv, float* wgt) {
    const float* ns = g + 7;
    const float* v = g + 15;
    const float metallic = g[13];
    if (lobe == 0) {
        for (int c = 0; c < 3; ++c) wgt[c] = (1.0f - metallic) * g[10 + c];
        return;
    }
    const float a = fmaxf(g[14] * g[14], NU_RL_ALPHA_MIN), a2 = a * a;
    const float nov = fmaxf((ns[0] * v[0] + ns[1] * v[1]) + ns[2] * v[2], NU_RL_NOV_MIN);
    const float nol = (ns[0] * l[0] + ns[1] * l[1]) + ns[2] * l[2];
    const float noh = (ns[0] * hv[0] + ns[1] * hv[1]) + ns[2] * hv[2];
    const float voh = (v[0] * hv[0] + v[1] * hv[1]) + v[2] * hv[2];
    const float G = nu_rl_g1(nol, a2) * nu_rl_g1(nov, a2);
    const float m = 1.0f - fminf(voh, 1.0f);
    const float fc = (m * m) * (m * m) * m;
    const float k = G * voh / (nov * noh);
    for (int c = 0; c < 3; ++c) {
        const float f0 = 0.04f + (g[10 + c] - 0.04f) * metallic;
        wgt[c] = (f0 + (1.0f - f0) * fc) * k;
    }
}

// ---- visibility transfer: the hemisphere samples of a surface point, its 16-float transfer row, the row of a hit point ----
// Transfer row of a point: NU_TR_ROW floats.
//   [0..8] T_k = (1/S) sum_s V_s Y_k(w_s), order-2 real SH in the order (0,0) (1,-1) (1,0) (1,1) (2,-2) .. (2,2)
//   [9] ambient occlusion = unoccluded samples / S   [10..12] bent normal (unit)   [13..15] 0
#define NU_TR_ROW 16
#define NU_TR_LIVE 13                // columns a sample contributes to: 9 SH values, 1, its direction

// Sample j of M of the point that hashes as `id`: section 20's sequence with ONE lobe -- Hammersley point (j / M, bit-reversed j) as 32-bit
// fixed point, Cranley-Patterson shift = two hash words of (id, seed), the uniforms are the top 24 bits.  Integers up to bits[0], bits[1].
static __device__ inline void nu_transfer_uniforms(int id, unsigned seed, int M, int j, unsigned* bits) {
    const unsigned x1 = (unsigned)(((unsigned long long)(unsigned)j << 32) / (unsigned long long)M);
    const unsigned x2 = __brev((unsigned)j);
    unsigned a = nu_rl_fmix32((unsigned)id + 0x9E3779B9u);
    a = nu_rl_fmix32(a ^ seed);
    const unsigned h1 = nu_rl_fmix32(a + 1u);
    const unsigned h2 = nu_rl_fmix32(h1 ^ 0x68E31DA4u);
    bits[0] = (x1 + h1) >> 8;
    bits[1] = (x2 + h2) >> 8;
}

// The ray of those two integers at point p with unit normal n: cosine-weighted direction cos = sqrt(1 - u2), sin = sqrt(u2),
// phi = 2 pi u1 in nu_rl_frame(n); origin p + eps n.  u2 < 1, so cos > 0: every sample is above the horizon and is traced.
static __device__ inline void nu_transfer_ray(const float* p, const float* n, float eps, const unsigned* bits, float* o, float* d) {
    const float u1 = (float)bits[0] * 5.9604644775390625e-08f, u2 = (float)bits[1] * 5.9604644775390625e-08f;   // 2^-24
    float t[3], b[3];
    nu_rl_frame(n, t, b);
    float sp, cp;
    sincosf(6.283185307179586f * u1, &sp, &cp);
    const float ct = sqrtf(1.0f - u2), st = sqrtf(u2);
    const float lx = st * cp, ly = st * sp;
    for (int k = 0; k < 3; ++k) {
        d[k] = (lx * t[k] + ly * b[k]) + ct * n[k];
        o[k] = p[k] + eps * n[k];
    }
}

// Order-2 real spherical harmonics of a direction, the order and constants of the row above.
static __device__ inline void nu_transfer_sh9(const float* w, float* y) {
    const float x = w[0], yy = w[1], z = w[2];
    y[0] = 0.282095f;
    y[1] = 0.488603f * yy;
    y[2] = 0.488603f * z;
    y[3] = 0.488603f * x;
    y[4] = 1.092548f * (x * yy);
    y[5] = 1.092548f * (yy * z);
    y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
    y[7] = 1.092548f * (x * z);
    y[8] = 0.546274f * (x * x - yy * yy);
}

// What an unoccluded sample of direction w adds to the NU_TR_LIVE sums of its point.
static __device__ inline void nu_transfer_contrib(const float* w, float* c) {
    nu_transfer_sh9(w, c);
    c[9] = 1.0f;
    c[10] = w[0]; c[11] = w[1]; c[12] = w[2];
}

// Output column c (0 .. NU_TR_ROW - 1) of a row from the NU_TR_LIVE sums over S samples.
static __device__ inline float nu_transfer_finish(const float* sum, const float* n, int S, int c) {
    if (c < 10) return sum[c] / (float)S;
    if (c >= NU_TR_LIVE) return 0.0f;
    const float len = sqrtf((sum[10] * sum[10] + sum[11] * sum[11]) + sum[12] * sum[12]);
    return len < 1e-12f ? n[c - 10] : sum[c] / len;
}

// Barycentric coordinates (u, v) of a point x of the plane of triangle (v0, v1, v2): x = v0 + u (v1 - v0) + v (v2 - v0), least squares.
// THE formula of the occluded resolve (the float64 oracle restates it); a face without area gives u = v = 0, vertex 0.
static __device__ inline void nu_transfer_bary(const float* x, const float* v0, const float* v1, const float* v2, float& u, float& v) {
    float e1[3], e2[3], tv[3];
    for (int k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; tv[k] = x[k] - v0[k]; }
    const float d11 = nu_rl_dot3(e1, e1), d12 = nu_rl_dot3(e1, e2), d22 = nu_rl_dot3(e2, e2);
    const float t1 = nu_rl_dot3(tv, e1), t2 = nu_rl_dot3(tv, e2);
    const float den = d11 * d22 - d12 * d12;
    u = 0.0f; v = 0.0f;
    if (den > 0.0f) {
        u = (d22 * t1 - d12 * t2) / den;
        v = (d11 * t2 - d12 * t1) / den;
    }
}

// The NU_TR_LIVE live columns of the transfer at hit point x of face `id`: r0 + u (r1 - r0) + v (r2 - r0) of the three vertex rows (rows
// that agree in a column give that value exactly), the bent normal renormalised (vertex 0's when the mix has no length).
static __device__ inline void nu_transfer_at(const float* __restrict__ V, const int* __restrict__ F, const float* __restrict__ transfer,
                                             int id, const float* x, float* row) {
    const int i0 = F[id * 3LL], i1 = F[id * 3LL + 1], i2 = F[id * 3LL + 2];
    float v0[3], v1[3], v2[3], u, v;
    for (int k = 0; k < 3; ++k) { v0[k] = V[i0 * 3LL + k]; v1[k] = V[i1 * 3LL + k]; v2[k] = V[i2 * 3LL + k]; }
    nu_transfer_bary(x, v0, v1, v2, u, v);
    const float* r0 = transfer + (long long)i0 * NU_TR_ROW;
    const float* r1 = transfer + (long long)i1 * NU_TR_ROW;
    const float* r2 = transfer + (long long)i2 * NU_TR_ROW;
    for (int k = 0; k < NU_TR_LIVE; ++k) row[k] = (r0[k] + u * (r1[k] - r0[k])) + v * (r2[k] - r0[k]);
    const float len = sqrtf((row[10] * row[10] + row[11] * row[11]) + row[12] * row[12]);
    for (int k = 10; k < NU_TR_LIVE; ++k) row[k] = len > 0.0f ? row[k] / len : r0[k];
}

// Specular occlusion of Lagarde & de Rousiers 2014: clamp((NoV + ao)^(2^(-16 rho - 1)) - 1 + ao, 0, 1); exactly 1 at ao = 1.
static __device__ inline float nu_transfer_spec_occlusion(float nov, float ao, float rho) {
    const float p = powf(fminf(fmaxf(nov, 0.0f), 1.0f) + ao, exp2f(-16.0f * rho - 1.0f));
    return fminf(fmaxf((p - 1.0f) + ao, 0.0f), 1.0f);
}
