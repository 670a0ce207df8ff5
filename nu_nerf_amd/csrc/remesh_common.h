// remesh_common.h -- the mesh tables and the small fp32 helpers shared by the kernels that edit a triangle mesh in rounds
// (remesh.hip: isotropic remeshing; decimate.hip: quadric-error decimation).  The tables are described at the top of remesh.hip.
#pragma once
#include "nu_common.h"

#pragma clang fp contract(off)

#define RM_SENTINEL 0x7fffffffffffffffLL
#define RM_NO_KEY 0xffffffffffffffffull
#define RM_MAX_RING 32            // faces a collapse may rewrite (the faces of both endpoints but the edge's two); more: rejected
#define RM_MISS 10000000          // nu_lbvh_closest's miss index

struct RmMesh {
    const float* V;
    const int* F;
    const int* E;
    const int* he_edge;
    const int* vc_off;
    const int* vc_corner;
    const unsigned char* vlock;
    const unsigned char* vbound;
    int nv, nf;
};

static __device__ inline void rm_ld(const float* V, int v, float* p) {
    for (int k = 0; k < 3; ++k) p[k] = V[3LL * v + k];
}
static __device__ inline float rm_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static __device__ inline void rm_sub(const float* a, const float* b, float* c) {
    for (int k = 0; k < 3; ++k) c[k] = a[k] - b[k];
}
static __device__ inline void rm_cross(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static __device__ inline float rm_dist2(const float* a, const float* b) {
    float e[3];
    rm_sub(a, b, e);
    return rm_dot(e, e);
}
// unnormalised normal (b - a) x (c - a)
static __device__ inline void rm_normal(const float* a, const float* b, const float* c, float* n) {
    float u[3], w[3];
    rm_sub(b, a, u);
    rm_sub(c, a, w);
    rm_cross(u, w, n);
}
// the four surface-distance query points of a triangle: centroid ((a + b) + c) / 3, then the midpoints of ab, bc, ca
static __device__ inline void rm_face_points(const float* a, const float* b, const float* c, float* out) {
    for (int k = 0; k < 3; ++k) {
        out[k] = ((a[k] + b[k]) + c[k]) / 3.0f;
        out[3 + k] = (a[k] + b[k]) * 0.5f;
        out[6 + k] = (b[k] + c[k]) * 0.5f;
        out[9 + k] = (c[k] + a[k]) * 0.5f;
    }
}
static __device__ inline int rm_deg(const RmMesh& m, int v) { return m.vc_off[v + 1] - m.vc_off[v]; }
static __device__ inline bool rm_face_has(const int* F, int g, int v) { return F[3 * g] == v || F[3 * g + 1] == v || F[3 * g + 2] == v; }
// x shares a face with v
static __device__ inline bool rm_adjacent(const RmMesh& m, int v, int x) {
    for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c)
        if (rm_face_has(m.F, m.vc_corner[c] / 3, x)) return true;
    return false;
}

// the interior edge at slot e: f0 = (a, b, c) holds the half-edge a -> b, f1 = (b, a, d); false for a non-edge or locked slot
struct RmQuad {
    int a, b, c, d, f0, f1;
};
static __device__ inline bool rm_quad(const RmMesh& m, int e, RmQuad& q) {
    const int* r = m.E + 4LL * e;
    if (r[2] != 2 || r[3]) return false;
    const int h0 = r[0], h1 = r[1];
    q.f0 = h0 / 3;
    q.f1 = h1 / 3;
    const int s0 = h0 - 3 * q.f0, s1 = h1 - 3 * q.f1;
    q.a = m.F[3 * q.f0 + s0];
    q.b = m.F[3 * q.f0 + (s0 + 1) % 3];
    q.c = m.F[3 * q.f0 + (s0 + 2) % 3];
    q.d = m.F[3 * q.f1 + (s1 + 2) % 3];
    return true;
}

// every vertex of every face of a and b: the set a collapse of (a, b) must hold.  f(v) per vertex (repeats included).
template <typename Fn>
static __device__ inline void rm_for_collapse_ring(const RmMesh& m, const RmQuad& q, Fn f) {
    for (int side = 0; side < 2; ++side) {
        const int v = side ? q.b : q.a;
        for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
            const int g = m.vc_corner[c] / 3;
            for (int t = 0; t < 3; ++t) f(m.F[3 * g + t]);
        }
    }
}

static inline bool rm_mesh_ok(const RmMesh& m) {
    return m.nv > 0 && m.nf > 0 && 3LL * m.nf < (1LL << 31) && m.V && m.F && m.E && m.he_edge && m.vc_off && m.vc_corner && m.vlock &&
           m.vbound;
}
static inline RmMesh rm_mesh(const float* V, int nv, const int* F, int nf, const int* E, const int* he_edge, const int* vc_off,
                             const int* vc_corner, const unsigned char* vlock, const unsigned char* vbound) {
    RmMesh m = {V, F, E, he_edge, vc_off, vc_corner, vlock, vbound, nv, nf};
    return m;
}

#define RM_MESH_ARGS const float *V, int nv, const int *F, int nf, const int *E, const int *he_edge, const int *vc_off, const int *vc_corner, \
                     const unsigned char *vlock, const unsigned char *vbound
#define RM_MESH rm_mesh(V, nv, F, nf, E, he_edge, vc_off, vc_corner, vlock, vbound)
