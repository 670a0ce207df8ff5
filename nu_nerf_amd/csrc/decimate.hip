// decimate.hip -- quadric-error edge-collapse decimation of a triangle mesh to a face budget (Garland & Heckbert 1997), with the
// quadrics rebuilt from the current mesh every round (memoryless: Lindstrom & Turk 1998), so nothing is carried through collapses or
// compaction.  The driver, the sort and the scans are in nu_nerf_amd/decimate.py; the tables are remesh.hip's (remesh_common.h).
//
// One round on a compacted mesh:
//   quadrics  per vertex, one thread: Q_v = sum over its faces in corner order of w (n^, d)(n^, d)^T, n = (p1 - p0) x (p2 - p0),
//             n^ = n / |n|, d = -n^ . p0, w = |n| / 2; the ten unique entries, float64
//   eval      per edge slot, one thread: placement (the minimiser of Q_a + Q_b by explicit cofactors when it is well conditioned and
//             near the edge, else the cheapest of a, b, midpoint; a locked end keeps its position), rounded to fp32 once; the cost at
//             the rounded point; the topological rejections of remesh.hip's collapse; per rewritten face no zero area, no normal
//             turned by 90 degrees or more, no shape quality both below min_quality and below the face's old one.  Writes the cost,
//             the position and the query-point count (7 per rewritten face; 0 = rejected)
//   points    (surface bound only) the query points of the candidates -- every rewritten face's three vertices, centroid and edge
//             midpoints -- for the caller's bounded nu_lbvh_closest, and per point the squared distance it may have:
//             (bound - rho)^2, rho = longest edge / sqrt(12).  The midpoints cut a face into four half-size triangles whose corners
//             are all query points, and no point of a triangle is farther than its longest edge / sqrt(3) from a corner, so every
//             point of the face is within rho of a query point and hence within the bound of the input.  A face with rho >= bound
//             cannot be certified and rejects its candidate: under a bound, faces stay shorter than sqrt(12) x bound
//   keys      ((bits(float32(cost + floor)) >> 12) << 32) | mix32(edge id): cost quantised to 20 bits, ties broken by a bijective
//             hash of the edge id so that equal costs (flat regions) do not order the candidates along the edge table
//   claim     candidates at or below the budget threshold atomicMin their key onto every vertex of every face of a and b (the closed
//             neighbourhood of the edge); a winner holds the minimum at a, b and the two opposite vertices c, d.  Narrower than
//             remesh.hip's hold-everything rule and as safe: two winners have no end in each other's neighbourhood
//             -- each wrote onto the other's end, and both cannot hold a minimum there -- and share no opposite vertex
//   apply     winners in place: the kept vertex takes the position, the removed vertex's faces are rewritten, two faces die
// A minimum does not depend on arrival order and there is no float atomic, so two runs give the same bits.  All arithmetic is
// float64 with one rounding per operation, in the order of the port in tests/decimate_oracle.py; sqrt and divide are the IEEE
// correctly rounded ones.
#include "nu_common.h"
#include "remesh_common.h"

#pragma clang fp contract(off)

#define DM_NO_KEY 0x7fffffffffffffffull       // above every key (the high half of a key is below 2^20); sorts last as int64 too

static __device__ inline void dm_ld(const float* V, int v, double* p) {
    for (int k = 0; k < 3; ++k) p[k] = (double)V[3LL * v + k];
}
static __device__ inline double dm_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static __device__ inline double dm_dist2(const double* a, const double* b) {
    const double e[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    return dm_dot(e, e);
}
// unnormalised normal (b - a) x (c - a)
static __device__ inline void dm_normal(const double* a, const double* b, const double* c, double* n) {
    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}
// a bijection on 32-bit integers (the finaliser of MurmurHash3: xor-shifts and odd multipliers are each invertible)
static __device__ inline unsigned dm_mix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------------------------------------ vertex quadrics
// entries k = 0..9: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3) of the symmetric 4 x 4
__global__ __launch_bounds__(256) void dm_quadric_kernel(RmMesh m, double* __restrict__ Q) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.nv) return;
    double q[10];
    for (int k = 0; k < 10; ++k) q[k] = 0.0;
    for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
        const int g = m.vc_corner[c] / 3;
        double p0[3], p1[3], p2[3], n[3];
        dm_ld(m.V, m.F[3 * g], p0);
        dm_ld(m.V, m.F[3 * g + 1], p1);
        dm_ld(m.V, m.F[3 * g + 2], p2);
        dm_normal(p0, p1, p2, n);
        const double nn = dm_dot(n, n);
        if (!(nn > 0.0)) continue;
        const double len = __dsqrt_rn(nn);
        double pl[4];
        for (int k = 0; k < 3; ++k) pl[k] = __ddiv_rn(n[k], len);
        pl[3] = -dm_dot(pl, p0);
        const double w = len * 0.5;
        int k = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = i; j < 4; ++j, ++k) q[k] = q[k] + w * (pl[i] * pl[j]);
    }
    for (int k = 0; k < 10; ++k) Q[10LL * v + k] = q[k];
}

// ------------------------------------------------------------------------------------------------ edge evaluation
struct DmQuadric {
    double a00, a01, a02, a11, a12, a22, b0, b1, b2, c;
};
// x^T A x + 2 b^T x + c
static __device__ inline double dm_cost(const DmQuadric& s, const double* x) {
    const double ax0 = (s.a00 * x[0] + s.a01 * x[1]) + s.a02 * x[2];
    const double ax1 = (s.a01 * x[0] + s.a11 * x[1]) + s.a12 * x[2];
    const double ax2 = (s.a02 * x[0] + s.a12 * x[1]) + s.a22 * x[2];
    const double xax = (x[0] * ax0 + x[1] * ax1) + x[2] * ax2;
    const double bx = (s.b0 * x[0] + s.b1 * x[1]) + s.b2 * x[2];
    return (xax + 2.0 * bx) + s.c;
}

// Returns the query-point count of edge slot e (7 per rewritten face; 0 = rejected), its cost and its fp32 position.
static __device__ int dm_eval(const RmMesh& m, int e, const double* __restrict__ Q, double min_q2, double* cost, float* pos) {
    RmQuad q;
    if (!rm_quad(m, e, q) || q.c == q.d) return 0;
    const int a = q.a, b = q.b;
    const bool la = m.vlock[a], lb = m.vlock[b];
    if (la && lb) return 0;
    if (rm_deg(m, q.c) <= 3 || rm_deg(m, q.d) <= 3) return 0;
    const double* qa = Q + 10LL * a;
    const double* qb = Q + 10LL * b;
    DmQuadric s;
    s.a00 = qa[0] + qb[0]; s.a01 = qa[1] + qb[1]; s.a02 = qa[2] + qb[2]; s.b0 = qa[3] + qb[3];
    s.a11 = qa[4] + qb[4]; s.a12 = qa[5] + qb[5]; s.b1 = qa[6] + qb[6];
    s.a22 = qa[7] + qb[7]; s.b2 = qa[8] + qb[8];
    s.c = qa[9] + qb[9];
    double pa[3], pb[3], x[3];
    dm_ld(m.V, a, pa);
    dm_ld(m.V, b, pb);
    if (la || lb) {
        for (int k = 0; k < 3; ++k) x[k] = la ? pa[k] : pb[k];
    } else {
        double mid[3];
        for (int k = 0; k < 3; ++k) mid[k] = (pa[k] + pb[k]) * 0.5;
        const double c00 = s.a11 * s.a22 - s.a12 * s.a12;
        const double c01 = s.a02 * s.a12 - s.a01 * s.a22;
        const double c02 = s.a01 * s.a12 - s.a02 * s.a11;
        const double det = (s.a00 * c00 + s.a01 * c01) + s.a02 * c02;
        const double tr = fabs((s.a00 + s.a11) + s.a22);
        bool ok = fabs(det) > 1e-9 * ((tr * tr) * tr);
        if (ok) {
            const double c11 = s.a00 * s.a22 - s.a02 * s.a02;
            const double c12 = s.a01 * s.a02 - s.a00 * s.a12;
            const double c22 = s.a00 * s.a11 - s.a01 * s.a01;
            const double r0 = -s.b0, r1 = -s.b1, r2 = -s.b2;
            x[0] = __ddiv_rn((c00 * r0 + c01 * r1) + c02 * r2, det);
            x[1] = __ddiv_rn((c01 * r0 + c11 * r1) + c12 * r2, det);
            x[2] = __ddiv_rn((c02 * r0 + c12 * r1) + c22 * r2, det);
            ok = dm_dist2(x, mid) <= dm_dist2(pa, pb);
        }
        if (!ok) {                                   // the cheapest of a, b, midpoint; ties in that order
            double best = dm_cost(s, pa);
            const double cb = dm_cost(s, pb), cm = dm_cost(s, mid);
            for (int k = 0; k < 3; ++k) x[k] = pa[k];
            if (cb < best) {
                best = cb;
                for (int k = 0; k < 3; ++k) x[k] = pb[k];
            }
            if (cm < best)
                for (int k = 0; k < 3; ++k) x[k] = mid[k];
        }
    }
    float p[3];
    double xd[3];
    for (int k = 0; k < 3; ++k) {
        p[k] = (float)x[k];
        xd[k] = (double)p[k];
    }
    double cst = dm_cost(s, xd);
    if (!isfinite(cst)) return 0;
    cst = cst > 0.0 ? cst : 0.0;
    // link condition: a and b share no neighbour but c and d
    for (int c = m.vc_off[a]; c < m.vc_off[a + 1]; ++c) {
        const int g = m.vc_corner[c] / 3;
        for (int t = 0; t < 3; ++t) {
            const int u = m.F[3 * g + t];
            if (u == a || u == b || u == q.c || u == q.d) continue;
            if (rm_adjacent(m, b, u)) return 0;
        }
    }
    int n = 0;
    for (int side = 0; side < 2; ++side) {
        const int v = side ? b : a, o = side ? a : b;
        for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
            const int g = m.vc_corner[c] / 3;
            if (rm_face_has(m.F, g, o)) continue;
            double xo[3][3], y[3][3];
            for (int t = 0; t < 3; ++t) {
                const int u = m.F[3 * g + t];
                dm_ld(m.V, u, xo[t]);
                for (int k = 0; k < 3; ++k) y[t][k] = u == v ? xd[k] : xo[t][k];
            }
            double no[3], nw[3];
            dm_normal(xo[0], xo[1], xo[2], no);
            dm_normal(y[0], y[1], y[2], nw);
            const double nn_new = dm_dot(nw, nw), nn_old = dm_dot(no, no);
            if (!(nn_new > 0.0)) return 0;
            if (nn_old > 0.0 && !(dm_dot(no, nw) > 0.0)) return 0;
            const double sn = (dm_dist2(y[0], y[1]) + dm_dist2(y[1], y[2])) + dm_dist2(y[2], y[0]);
            const double so = (dm_dist2(xo[0], xo[1]) + dm_dist2(xo[1], xo[2])) + dm_dist2(xo[2], xo[0]);
            // quality 12 |n|^2 / (sum l^2)^2 (1 for an equilateral face) below min_q2 AND below the old face's: no division
            if (12.0 * nn_new < min_q2 * (sn * sn) && nn_new * (so * so) < nn_old * (sn * sn)) return 0;
            if (n >= RM_MAX_RING) return 0;
            ++n;
        }
    }
    if (n == 0) return 0;
    *cost = cst;
    for (int k = 0; k < 3; ++k) pos[k] = p[k];
    return 7 * n;
}

__global__ __launch_bounds__(256) void dm_eval_kernel(RmMesh m, int nh, const double* __restrict__ Q, double min_q2,
                                                      double* __restrict__ cost, float* __restrict__ pos, int* __restrict__ npts) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    double c = 0.0;
    float p[3] = {0.f, 0.f, 0.f};
    const int n = dm_eval(m, e, Q, min_q2, &c, p);
    npts[e] = n;
    cost[e] = n ? c : 0.0;
    for (int k = 0; k < 3; ++k) pos[3LL * e + k] = n ? p[k] : 0.0f;
}

// the query points of candidate e: per rewritten face (fp32, the moved vertex at pos[e]) its three vertices, then remesh.hip's four
// (centroid, edge midpoints); lim = the squared distance each may have, negative where the face is too large to certify
__global__ __launch_bounds__(256) void dm_points_kernel(RmMesh m, int nh, const float* __restrict__ pos, const int* __restrict__ npts,
                                                        const long long* __restrict__ poff, float max_dist, float* __restrict__ pts,
                                                        float* __restrict__ lim) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || npts[e] == 0) return;
    RmQuad q;
    rm_quad(m, e, q);
    const float p[3] = {pos[3LL * e], pos[3LL * e + 1], pos[3LL * e + 2]};
    float* out = pts + 3 * poff[e];
    float* lout = lim + poff[e];
    int n = 0;
    for (int side = 0; side < 2; ++side) {
        const int v = side ? q.b : q.a, o = side ? q.a : q.b;
        for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
            const int g = m.vc_corner[c] / 3;
            if (rm_face_has(m.F, g, o)) continue;
            if (7 * n + 7 > npts[e]) return;              // never past the candidate's own segment
            float y[3][3];
            for (int t = 0; t < 3; ++t) {
                const int u = m.F[3 * g + t];
                for (int k = 0; k < 3; ++k) {
                    y[t][k] = u == v ? p[k] : m.V[3LL * u + k];
                    out[21LL * n + 3 * t + k] = y[t][k];
                }
            }
            rm_face_points(y[0], y[1], y[2], out + 21LL * n + 9);
            const float l2 = fmaxf(fmaxf(rm_dist2(y[0], y[1]), rm_dist2(y[1], y[2])), rm_dist2(y[2], y[0]));
            const float room = max_dist - sqrtf(l2 / 12.0f) * 1.0001f;      // rho rounded up
            for (int i = 0; i < 7; ++i) lout[7 * n + i] = room > 0.0f ? room * room : -1.0f;
            ++n;
        }
    }
}

// ------------------------------------------------------------------------------------------------ keys, claim, win, apply
__global__ __launch_bounds__(256) void dm_keys_kernel(const double* __restrict__ cost, const int* __restrict__ npts,
                                                      const long long* __restrict__ poff, const float* __restrict__ pd2,
                                                      const float* __restrict__ lim, int nh, double floor_,
                                                      unsigned long long* __restrict__ ckey) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    unsigned long long key = DM_NO_KEY;
    const int n = npts[e];
    bool ok = n > 0;
    if (ok && pd2 != nullptr)
        for (long long i = poff[e]; i < poff[e] + n; ++i)
            if (!(pd2[i] <= lim[i])) ok = false;          // a miss is +inf
    if (ok) {
        const unsigned hi = (unsigned)__float_as_int((float)(cost[e] + floor_)) >> 12;
        key = ((unsigned long long)hi << 32) | dm_mix32((unsigned)e);
    }
    ckey[e] = key;
}

__global__ __launch_bounds__(256) void dm_claim_kernel(RmMesh m, int nh, const unsigned long long* __restrict__ ckey,
                                                       const unsigned long long* __restrict__ thr, unsigned long long* __restrict__ claim) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    const unsigned long long key = ckey[e];
    if (key == DM_NO_KEY || key > thr[0]) return;
    RmQuad q;
    rm_quad(m, e, q);
    rm_for_collapse_ring(m, q, [&](int v) { atomicMin(claim + v, key); });
}

__global__ __launch_bounds__(256) void dm_win_kernel(RmMesh m, int nh, const unsigned long long* __restrict__ ckey,
                                                     const unsigned long long* __restrict__ thr,
                                                     const unsigned long long* __restrict__ claim, int* __restrict__ win) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    const unsigned long long key = ckey[e];
    int w = 0;
    if (key != DM_NO_KEY && key <= thr[0]) {
        RmQuad q;
        rm_quad(m, e, q);
        w = claim[q.a] == key && claim[q.b] == key && claim[q.c] == key && claim[q.d] == key ? 1 : 0;
    }
    win[e] = w;
}

// no winner has an end in another's neighbourhood, so the rows of F and V they write are disjoint and nothing one reads is written by
// another: they apply in place concurrently; V / F may be the tables' own arrays (no __restrict__)
__global__ __launch_bounds__(256) void dm_apply_kernel(RmMesh m, int nh, const int* __restrict__ win, const float* __restrict__ pos,
                                                       float* V, int* F) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || !win[e]) return;
    RmQuad q;
    rm_quad(m, e, q);
    const bool lb = m.vlock[q.b];
    const int keep = lb ? q.b : q.a, rem = lb ? q.a : q.b;
    for (int k = 0; k < 3; ++k) V[3LL * keep + k] = pos[3LL * e + k];
    for (int c = m.vc_off[rem]; c < m.vc_off[rem + 1]; ++c) {
        const int g = m.vc_corner[c] / 3;
        if (rm_face_has(F, g, keep)) {
            F[3 * g] = -1; F[3 * g + 1] = -1; F[3 * g + 2] = -1;
        } else {
            for (int t = 0; t < 3; ++t)
                if (F[3 * g + t] == rem) F[3 * g + t] = keep;
        }
    }
}

extern "C" int nu_dm_quadrics(RM_MESH_ARGS, double* Q, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !Q) return NU_ERR_ARG;
    hipLaunchKernelGGL(dm_quadric_kernel, dim3((unsigned)nu_cdiv(nv, 256)), dim3(256), 0, stream, m, Q);
    return nu_launch_status();
}

extern "C" int nu_dm_eval(RM_MESH_ARGS, const double* Q, double min_quality2, double* cost, float* pos, int* npts, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !Q || !cost || !pos || !npts || !(min_quality2 >= 0.0)) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(dm_eval_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, Q, min_quality2, cost, pos, npts);
    return nu_launch_status();
}

extern "C" int nu_dm_points(RM_MESH_ARGS, const float* pos, const int* npts, const long long* poff, float max_dist, float* pts, float* lim,
                            hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !pos || !npts || !poff || !pts || !lim || !(max_dist >= 0.0f)) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(dm_points_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, pos, npts, poff, max_dist, pts, lim);
    return nu_launch_status();
}

extern "C" int nu_dm_keys(const double* cost, const int* npts, const long long* poff, const float* pd2, const float* lim, int nh,
                          double cost_floor, unsigned long long* ckey, hipStream_t stream) {
    if (nh <= 0 || !cost || !npts || !ckey || (pd2 != nullptr && (!poff || !lim)) || !(cost_floor >= 0.0)) return NU_ERR_ARG;
    hipLaunchKernelGGL(dm_keys_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, cost, npts, poff, pd2, lim, nh, cost_floor, ckey);
    return nu_launch_status();
}

extern "C" int nu_dm_claim(RM_MESH_ARGS, const unsigned long long* ckey, const unsigned long long* threshold, unsigned long long* claim,
                           int* win, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !ckey || !threshold || !claim || !win) return NU_ERR_ARG;
    const int nh = 3 * nf;
    if (hipMemsetAsync(claim, 0xff, 8LL * nv, stream) != hipSuccess) return NU_ERR_LAUNCH;
    const dim3 grid((unsigned)nu_cdiv(nh, 256));
    hipLaunchKernelGGL(dm_claim_kernel, grid, dim3(256), 0, stream, m, nh, ckey, threshold, claim);
    hipLaunchKernelGGL(dm_win_kernel, grid, dim3(256), 0, stream, m, nh, ckey, threshold, claim, win);
    return nu_launch_status();
}

extern "C" int nu_dm_apply(RM_MESH_ARGS, const int* win, const float* pos, float* V_io, int* F_io, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !win || !pos || !V_io || !F_io) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(dm_apply_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, win, pos, V_io, F_io);
    return nu_launch_status();
}
