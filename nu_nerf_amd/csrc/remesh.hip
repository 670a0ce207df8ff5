// remesh.hip -- isotropic explicit remeshing of a triangle mesh on the device (Botsch & Kobbelt 2004; the reference runs pymeshlab's
// meshing_isotropic_explicit_remeshing on the raw marching-cubes mesh, extract_mesh_stage1.py:44-50).  The driver, the sorts and
// the scans are in nu_nerf_amd/remesh.py; every geometric decision is made here.
//
// Mesh: V fp32 [nv,3], F int32 [nf,3]; a dead face (after a collapse) is the row (-1, -1, -1).  Half-edge h = 3 f + s runs from
// F[f][s] to F[f][(s+1) % 3].  Tables, rebuilt from F before every pass or round:
//   keys        64-bit (min, max) vertex pair per half-edge (dead: RM_SENTINEL), stably sorted by the caller -> skeys, perm
//   E [nh,4]    per SORTED slot i: (h0, h1, half-edge count, locked) at the first slot of a run of equal keys (that slot is the
//               edge's id), count 0 elsewhere.  An edge with a count other than 2, or whose two half-edges run the same way, is
//               locked and so are its vertices (vlock); a one-face edge makes its vertices boundary vertices (vbound)
//   he_edge     edge id of every half-edge (-1: dead face)
//   vc_off / vc_corner   vertex -> corner CSR (corners 3 f + s in ascending order): the caller's stable sort of F
// Passes: split (count -> caller's scans -> write, by edge id and (face, template slot)); collapse and flip rounds (count ->
// caller's scan -> query points -> caller's bounded nu_lbvh_closest -> claim -> apply); tangential relaxation; projection.
// A round's winners are an independent set chosen by a 64-bit atomicMin of (priority << 32 | edge id) over the vertices a
// candidate touches: a minimum does not depend on arrival order, so the set -- and everything else here -- is deterministic.
// No float atomics; every per-vertex sum walks the CSR in corner order.  fp32 with one rounding per operation, in the order of the
// numpy ports in tests/remesh_oracle.py.
#include "nu_common.h"
#include "remesh_common.h"        // RmMesh, the rm_* helpers and RM_MESH_ARGS (shared with decimate.hip)

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ edge table
__global__ __launch_bounds__(256) void rm_keys_kernel(const int* __restrict__ F, int nf, long long* __restrict__ keys) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= 3LL * nf) return;
    const long long f = h / 3;
    const int s = (int)(h - 3 * f);
    const int a = F[h], b = F[3 * f + (s + 1) % 3];
    if (F[3 * f] < 0) {
        keys[h] = RM_SENTINEL;
        return;
    }
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    keys[h] = ((long long)lo << 32) | (long long)(unsigned)hi;
}

__global__ __launch_bounds__(256) void rm_edges_kernel(const int* __restrict__ F, const long long* __restrict__ skeys,
                                                       const long long* __restrict__ perm, int nh, int* __restrict__ E,
                                                       int* __restrict__ he_edge, unsigned char* __restrict__ vlock,
                                                       unsigned char* __restrict__ vbound) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nh) return;
    const long long k = skeys[i];
    int* r = E + 4LL * i;
    r[0] = -1; r[1] = -1; r[2] = 0; r[3] = 1;
    if (k == RM_SENTINEL) {
        he_edge[perm[i]] = -1;
        return;
    }
    int j = i;
    while (j > 0 && skeys[j - 1] == k) --j;
    he_edge[perm[i]] = j;
    if (j != i) return;
    int n = 1;
    while (i + n < nh && skeys[i + n] == k) ++n;
    const int a = (int)(k >> 32), b = (int)(k & 0xffffffffLL);
    const int h0 = (int)perm[i], h1 = n >= 2 ? (int)perm[i + 1] : -1;
    bool lock = n != 2;
    if (n == 2 && F[h0] == F[h1]) lock = true;          // both half-edges run the same way: not an oriented 2-manifold edge
    r[0] = h0; r[1] = h1; r[2] = n; r[3] = lock ? 1 : 0;
    if (lock) { vlock[a] = 1; vlock[b] = 1; }
    if (n == 1) { vbound[a] = 1; vbound[b] = 1; }
}

extern "C" int nu_rm_edge_keys(const int* F, int nf, long long* keys, hipStream_t stream) {
    if (nf < 0 || (nf > 0 && (F == nullptr || keys == nullptr)) || 3LL * nf >= (1LL << 31)) return NU_ERR_ARG;
    if (nf == 0) return NU_OK;
    hipLaunchKernelGGL(rm_keys_kernel, dim3((unsigned)nu_cdivl(3LL * nf, 256)), dim3(256), 0, stream, F, nf, keys);
    return nu_launch_status();
}

extern "C" int nu_rm_edges(const int* F, int nf, int nv, const long long* skeys, const long long* perm, int* E, int* he_edge,
                           unsigned char* vlock, unsigned char* vbound, hipStream_t stream) {
    if (nf <= 0 || nv <= 0 || 3LL * nf >= (1LL << 31) || !F || !skeys || !perm || !E || !he_edge || !vlock || !vbound) return NU_ERR_ARG;
    if (hipMemsetAsync(vlock, 0, nv, stream) != hipSuccess || hipMemsetAsync(vbound, 0, nv, stream) != hipSuccess) return NU_ERR_LAUNCH;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(rm_edges_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, F, skeys, perm, nh, E, he_edge, vlock,
                       vbound);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ split
// eflag[e] = 1 when edge e is unlocked and |a - b|^2 > max_len2 (0 on the other slots)
__global__ __launch_bounds__(256) void rm_split_mark_kernel(const float* __restrict__ V, const int* __restrict__ F,
                                                            const int* __restrict__ E, int nh, float max_len2, int* __restrict__ eflag) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    const int* r = E + 4LL * e;
    int flag = 0;
    if (r[2] > 0 && !r[3]) {
        const int h = r[0], f = h / 3, s = h - 3 * f;
        float a[3], b[3];
        rm_ld(V, F[h], a);
        rm_ld(V, F[3 * f + (s + 1) % 3], b);
        flag = rm_dist2(a, b) > max_len2 ? 1 : 0;
    }
    eflag[e] = flag;
}

__global__ __launch_bounds__(256) void rm_split_count_kernel(const int* __restrict__ F, int nf, const int* __restrict__ he_edge,
                                                             const int* __restrict__ eflag, int* __restrict__ fcnt) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int n = 0;
    if (F[3 * f] >= 0) {
        n = 1;
        for (int s = 0; s < 3; ++s) n += eflag[he_edge[3 * f + s]];
    }
    fcnt[f] = n;                                 // output faces: 1 + split edges (0 for a dead face)
}

__global__ __launch_bounds__(256) void rm_split_vertex_kernel(const float* __restrict__ V, int nv, const int* __restrict__ F,
                                                              const int* __restrict__ E, int nh, const int* __restrict__ eflag,
                                                              const long long* __restrict__ voff, float* __restrict__ Vout) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || !eflag[e]) return;
    const int h = E[4LL * e], f = h / 3, s = h - 3 * f;
    float a[3], b[3];
    rm_ld(V, F[h], a);
    rm_ld(V, F[3 * f + (s + 1) % 3], b);
    const long long v = nv + voff[e];
    for (int k = 0; k < 3; ++k) Vout[3 * v + k] = (a[k] + b[k]) * 0.5f;
}

// templates (v0 v1 v2 the face, m_s the new vertex of edge s = (v_s, v_s+1)), rotated so that the pattern starts at slot r:
//   one split edge r:             (a, m, c) (m, b, c)                        a b c = v_r v_r+1 v_r+2
//   two, edge r not split:        (a, b, mbc) (a, mbc, mca) (mbc, c, mca)   a b c = v_r v_r+1 v_r+2
//   three:                        (v0, m0, m2) (m0, v1, m1) (m2, m1, v2) (m0, m1, m2)
__global__ __launch_bounds__(256) void rm_split_face_kernel(const int* __restrict__ F, int nf, int nv, const int* __restrict__ he_edge,
                                                            const int* __restrict__ eflag, const long long* __restrict__ voff,
                                                            const long long* __restrict__ foff, int* __restrict__ Fout) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || F[3 * f] < 0) return;
    int v[3], mid[3], mask = 0;
    for (int s = 0; s < 3; ++s) {
        v[s] = F[3 * f + s];
        const int e = he_edge[3 * f + s];
        mid[s] = eflag[e] ? (int)(nv + voff[e]) : -1;
        mask |= eflag[e] << s;
    }
    int* o = Fout + 3 * foff[f];
    auto put = [&](int t, int x, int y, int z) { o[3 * t] = x; o[3 * t + 1] = y; o[3 * t + 2] = z; };
    const int n = __popc(mask);
    if (n == 0) {
        put(0, v[0], v[1], v[2]);
    } else if (n == 1) {
        const int r = mask == 1 ? 0 : mask == 2 ? 1 : 2;
        const int a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3], m = mid[r];
        put(0, a, m, c);
        put(1, m, b, c);
    } else if (n == 2) {
        const int r = (~mask & 7) == 1 ? 0 : (~mask & 7) == 2 ? 1 : 2;
        const int a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3], mbc = mid[(r + 1) % 3], mca = mid[(r + 2) % 3];
        put(0, a, b, mbc);
        put(1, a, mbc, mca);
        put(2, mbc, c, mca);
    } else {
        put(0, v[0], mid[0], mid[2]);
        put(1, mid[0], v[1], mid[1]);
        put(2, mid[2], mid[1], v[2]);
        put(3, mid[0], mid[1], mid[2]);
    }
}

extern "C" int nu_rm_split_count(const float* V, const int* F, int nf, const int* E, const int* he_edge, float max_len2, int* eflag,
                                 int* fcnt, hipStream_t stream) {
    if (nf <= 0 || 3LL * nf >= (1LL << 31) || !V || !F || !E || !he_edge || !eflag || !fcnt) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(rm_split_mark_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, V, F, E, nh, max_len2, eflag);
    hipLaunchKernelGGL(rm_split_count_kernel, dim3((unsigned)nu_cdiv(nf, 256)), dim3(256), 0, stream, F, nf, he_edge, eflag, fcnt);
    return nu_launch_status();
}

extern "C" int nu_rm_split_write(const float* V, int nv, const int* F, int nf, const int* E, const int* he_edge, const int* eflag,
                                 const long long* voff, const long long* foff, float* Vout, int* Fout, hipStream_t stream) {
    if (nf <= 0 || nv <= 0 || 3LL * nf >= (1LL << 31) || !V || !F || !E || !he_edge || !eflag || !voff || !foff || !Vout || !Fout)
        return NU_ERR_ARG;
    const int nh = 3 * nf;
    if (hipMemcpyAsync(Vout, V, 12LL * nv, hipMemcpyDeviceToDevice, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(rm_split_vertex_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, V, nv, F, E, nh, eflag, voff, Vout);
    hipLaunchKernelGGL(rm_split_face_kernel, dim3((unsigned)nu_cdiv(nf, 256)), dim3(256), 0, stream, F, nf, nv, he_edge, eflag, voff, foff,
                       Fout);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ collapse
// Edge (a, b) of f0 = (a, b, c), f1 = (b, a, d), shorter than min_len2, not both endpoints locked.  `rem` merges into `keep` (b into a,
// or a into a locked b) at p = the locked endpoint, or (a + b) * 0.5.  Rejected when: c == d or c / d has <= 3 faces; a and b have
// a common neighbour other than c and d (link condition); a rewritten face (every face of a or b but f0, f1) would have zero area,
// turn its normal by more than 90 degrees, or have an edge to p longer than max_len2; or more than RM_MAX_RING faces are rewritten.
// Returns the number of query points (4 per rewritten face; 0 = rejected); PTS: writes them to pts.
template <bool PTS>
static __device__ int rm_collapse_eval(const RmMesh& m, int e, float min_len2, float max_len2, float* __restrict__ pts) {
    RmQuad q;
    if (!rm_quad(m, e, q) || q.c == q.d) return 0;
    const int a = q.a, b = q.b;
    const bool la = m.vlock[a], lb = m.vlock[b];
    if (la && lb) return 0;
    float pa[3], pb[3], p[3];
    rm_ld(m.V, a, pa);
    rm_ld(m.V, b, pb);
    if (!(rm_dist2(pa, pb) < min_len2)) return 0;
    if (rm_deg(m, q.c) <= 3 || rm_deg(m, q.d) <= 3) return 0;
    for (int k = 0; k < 3; ++k) p[k] = la ? pa[k] : lb ? pb[k] : (pa[k] + pb[k]) * 0.5f;
    for (int c = m.vc_off[a]; c < m.vc_off[a + 1]; ++c) {
        const int g = m.vc_corner[c] / 3;
        for (int t = 0; t < 3; ++t) {
            const int x = m.F[3 * g + t];
            if (x == a || x == b || x == q.c || x == q.d) continue;
            if (rm_adjacent(m, b, x)) return 0;
        }
    }
    int n = 0;
    for (int side = 0; side < 2; ++side) {
        const int v = side ? b : a, o = side ? a : b;
        for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
            const int g = m.vc_corner[c] / 3;
            if (rm_face_has(m.F, g, o)) continue;
            float x[3][3], y[3][3];
            for (int t = 0; t < 3; ++t) {
                const int u = m.F[3 * g + t];
                rm_ld(m.V, u, x[t]);
                const bool moved = u == v;
                for (int k = 0; k < 3; ++k) y[t][k] = moved ? p[k] : x[t][k];
                if (!moved && rm_dist2(p, x[t]) > max_len2) return 0;
            }
            float no[3], nn[3];
            rm_normal(x[0], x[1], x[2], no);
            rm_normal(y[0], y[1], y[2], nn);
            if (!(rm_dot(nn, nn) > 0.0f)) return 0;
            if (rm_dot(no, no) > 0.0f && !(rm_dot(no, nn) > 0.0f)) return 0;
            if (n >= RM_MAX_RING) return 0;
            if (PTS) rm_face_points(y[0], y[1], y[2], pts + 12LL * n);
            ++n;
        }
    }
    return 4 * n;
}

// ------------------------------------------------------------------------------------------------ flip
// Edge (a, b) -> (c, d): f0 = (a, b, c), f1 = (b, a, d) become (a, d, c), (d, b, c).  Valence = faces + 1 on a boundary vertex,
// target 6 (4 on a boundary); the flip must lower sum |valence - target| over a, b, c, d.  Rejected when c == d, a or b has
// valence <= 3, c and d are already adjacent, or a new face has zero area or makes an angle above the limit (cos2_max = its
// cos^2; compared as dot >= 0 and dot^2 >= cos2 |m|^2 |n|^2) with either replaced face of non-zero area.
// Returns 8 (query points of the two new faces) or 0; *gain = the decrease of the valence sum.
template <bool PTS>
static __device__ int rm_flip_eval(const RmMesh& m, int e, float cos2_max, int* gain, float* __restrict__ pts) {
    RmQuad q;
    if (!rm_quad(m, e, q) || q.c == q.d) return 0;
    const int vs[4] = {q.a, q.b, q.c, q.d};
    const int dv[4] = {-1, -1, 1, 1};
    int before = 0, after = 0;
    for (int i = 0; i < 4; ++i) {
        const int val = rm_deg(m, vs[i]) + (m.vbound[vs[i]] ? 1 : 0);
        const int tgt = m.vbound[vs[i]] ? 4 : 6;
        if (i < 2 && val <= 3) return 0;
        before += abs(val - tgt);
        after += abs(val + dv[i] - tgt);
    }
    if (after >= before) return 0;
    if (rm_adjacent(m, q.c, q.d)) return 0;
    float pa[3], pb[3], pc[3], pd[3];
    rm_ld(m.V, q.a, pa);
    rm_ld(m.V, q.b, pb);
    rm_ld(m.V, q.c, pc);
    rm_ld(m.V, q.d, pd);
    float n0[3], n1[3], m0[3], m1[3];
    rm_normal(pa, pb, pc, n0);
    rm_normal(pb, pa, pd, n1);
    rm_normal(pa, pd, pc, m0);
    rm_normal(pd, pb, pc, m1);
    const float* ms[2] = {m0, m1};
    const float* ns[2] = {n0, n1};
    for (int i = 0; i < 2; ++i) {
        const float mm = rm_dot(ms[i], ms[i]);
        if (!(mm > 0.0f)) return 0;
        for (int j = 0; j < 2; ++j) {
            const float nn = rm_dot(ns[j], ns[j]);
            if (!(nn > 0.0f)) continue;
            const float dn = rm_dot(ms[i], ns[j]);
            if (!(dn > 0.0f) || dn * dn < cos2_max * (mm * nn)) return 0;
        }
    }
    if (PTS) {
        rm_face_points(pa, pd, pc, pts);
        rm_face_points(pd, pb, pc, pts + 12);
    }
    *gain = before - after;
    return 8;
}

// ------------------------------------------------------------------------------------------------ rounds (collapse: mode 0, flip: 1)
template <int MODE>
__global__ __launch_bounds__(256) void rm_count_kernel(RmMesh m, int nh, float p0, float p1, int* __restrict__ npts) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    int g;
    npts[e] = MODE == 0 ? rm_collapse_eval<false>(m, e, p0, p1, nullptr) : rm_flip_eval<false>(m, e, p0, &g, nullptr);
}

template <int MODE>
__global__ __launch_bounds__(256) void rm_points_kernel(RmMesh m, int nh, float p0, float p1, const int* __restrict__ npts,
                                                        const long long* __restrict__ poff, float* __restrict__ pts) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || npts[e] == 0) return;
    int g;
    float* out = pts + 3 * poff[e];
    if (MODE == 0) rm_collapse_eval<true>(m, e, p0, p1, out);
    else rm_flip_eval<true>(m, e, p0, &g, out);
}

// the vertices a winner must hold: collapse -- every vertex of every face of a and b; flip -- a, b, c, d.  f(v) per vertex.
template <int MODE, typename Fn>
static __device__ inline void rm_for_ring(const RmMesh& m, const RmQuad& q, Fn f) {
    if (MODE == 0) {
        rm_for_collapse_ring(m, q, f);
    } else {
        f(q.a); f(q.b); f(q.c); f(q.d);
    }
}

// a candidate whose query points all found the input surface within the bound claims its vertices with its key:
// collapse (bits of |a - b|^2 << 32 | e), flip ((16 - gain) << 32 | e)
template <int MODE>
__global__ __launch_bounds__(256) void rm_claim_kernel(RmMesh m, int nh, float p0, const int* __restrict__ npts,
                                                       const long long* __restrict__ poff, const int* __restrict__ pidx,
                                                       unsigned long long* __restrict__ ckey, unsigned long long* __restrict__ claim) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    ckey[e] = RM_NO_KEY;
    const int n = npts[e];
    if (n == 0) return;
    for (long long i = poff[e]; i < poff[e] + n; ++i)
        if (pidx[i] == RM_MISS) return;
    RmQuad q;
    rm_quad(m, e, q);
    unsigned hi;
    if (MODE == 0) {
        float pa[3], pb[3];
        rm_ld(m.V, q.a, pa);
        rm_ld(m.V, q.b, pb);
        hi = (unsigned)__float_as_int(rm_dist2(pa, pb));
    } else {
        int gain = 0;
        rm_flip_eval<false>(m, e, p0, &gain, nullptr);
        hi = 16u - (unsigned)gain;
    }
    const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned)e;
    ckey[e] = key;
    rm_for_ring<MODE>(m, q, [&](int v) { atomicMin(claim + v, key); });
}

template <int MODE>
__global__ __launch_bounds__(256) void rm_win_kernel(RmMesh m, int nh, const unsigned long long* __restrict__ ckey,
                                                     const unsigned long long* __restrict__ claim, int* __restrict__ win) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh) return;
    const unsigned long long key = ckey[e];
    int w = 0;
    if (key != RM_NO_KEY) {
        RmQuad q;
        rm_quad(m, e, q);
        bool all = true;
        rm_for_ring<MODE>(m, q, [&](int v) { all = all && claim[v] == key; });
        w = all ? 1 : 0;
    }
    win[e] = w;
}

// winners touch disjoint faces and vertices (their claimed sets are disjoint), so they apply in place concurrently; V / F may be
// the tables' own arrays (no __restrict__)
__global__ __launch_bounds__(256) void rm_collapse_apply_kernel(RmMesh m, int nh, const int* __restrict__ win, float* V, int* F) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || !win[e]) return;
    RmQuad q;
    rm_quad(m, e, q);
    const bool lb = m.vlock[q.b], la = m.vlock[q.a];
    const int keep = lb ? q.b : q.a, rem = lb ? q.a : q.b;
    float pa[3], pb[3];
    rm_ld(V, q.a, pa);
    rm_ld(V, q.b, pb);
    for (int k = 0; k < 3; ++k) V[3LL * keep + k] = la ? pa[k] : lb ? pb[k] : (pa[k] + pb[k]) * 0.5f;
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

__global__ __launch_bounds__(256) void rm_flip_apply_kernel(RmMesh m, int nh, const int* __restrict__ win, int* F) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nh || !win[e]) return;
    RmQuad q;
    rm_quad(m, e, q);
    F[3 * q.f0] = q.a; F[3 * q.f0 + 1] = q.d; F[3 * q.f0 + 2] = q.c;
    F[3 * q.f1] = q.d; F[3 * q.f1 + 1] = q.b; F[3 * q.f1 + 2] = q.c;
}

static int rm_count(int mode, RmMesh m, float p0, float p1, int* npts, hipStream_t stream) {
    if (!rm_mesh_ok(m) || !npts) return NU_ERR_ARG;
    const int nh = 3 * m.nf;
    if (mode == 0) hipLaunchKernelGGL(rm_count_kernel<0>, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, p0, p1, npts);
    else hipLaunchKernelGGL(rm_count_kernel<1>, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, p0, p1, npts);
    return nu_launch_status();
}

static int rm_points(int mode, RmMesh m, float p0, float p1, const int* npts, const long long* poff, float* pts, hipStream_t stream) {
    if (!rm_mesh_ok(m) || !npts || !poff || !pts) return NU_ERR_ARG;
    const int nh = 3 * m.nf;
    if (mode == 0)
        hipLaunchKernelGGL(rm_points_kernel<0>, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, p0, p1, npts, poff, pts);
    else
        hipLaunchKernelGGL(rm_points_kernel<1>, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, p0, p1, npts, poff, pts);
    return nu_launch_status();
}

static int rm_claim(int mode, RmMesh m, float p0, const int* npts, const long long* poff, const int* pidx, unsigned long long* ckey,
                    unsigned long long* claim, int* win, hipStream_t stream) {
    if (!rm_mesh_ok(m) || !npts || !poff || !pidx || !ckey || !claim || !win) return NU_ERR_ARG;
    const int nh = 3 * m.nf;
    if (hipMemsetAsync(claim, 0xff, 8LL * m.nv, stream) != hipSuccess) return NU_ERR_LAUNCH;
    const dim3 grid((unsigned)nu_cdiv(nh, 256));
    if (mode == 0) {
        hipLaunchKernelGGL(rm_claim_kernel<0>, grid, dim3(256), 0, stream, m, nh, p0, npts, poff, pidx, ckey, claim);
        hipLaunchKernelGGL(rm_win_kernel<0>, grid, dim3(256), 0, stream, m, nh, ckey, claim, win);
    } else {
        hipLaunchKernelGGL(rm_claim_kernel<1>, grid, dim3(256), 0, stream, m, nh, p0, npts, poff, pidx, ckey, claim);
        hipLaunchKernelGGL(rm_win_kernel<1>, grid, dim3(256), 0, stream, m, nh, ckey, claim, win);
    }
    return nu_launch_status();
}

extern "C" int nu_rm_collapse_count(RM_MESH_ARGS, float min_len2, float max_len2, int* npts, hipStream_t stream) {
    return rm_count(0, RM_MESH, min_len2, max_len2, npts, stream);
}
extern "C" int nu_rm_collapse_points(RM_MESH_ARGS, float min_len2, float max_len2, const int* npts, const long long* poff, float* pts,
                                     hipStream_t stream) {
    return rm_points(0, RM_MESH, min_len2, max_len2, npts, poff, pts, stream);
}
extern "C" int nu_rm_collapse_claim(RM_MESH_ARGS, const int* npts, const long long* poff, const int* pidx, unsigned long long* ckey,
                                    unsigned long long* claim, int* win, hipStream_t stream) {
    return rm_claim(0, RM_MESH, 0.0f, npts, poff, pidx, ckey, claim, win, stream);
}
extern "C" int nu_rm_collapse_apply(RM_MESH_ARGS, const int* win, float* V_io, int* F_io, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !win || !V_io || !F_io) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(rm_collapse_apply_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, win, V_io, F_io);
    return nu_launch_status();
}
extern "C" int nu_rm_flip_count(RM_MESH_ARGS, float cos2_max, int* npts, hipStream_t stream) {
    return rm_count(1, RM_MESH, cos2_max, 0.0f, npts, stream);
}
extern "C" int nu_rm_flip_points(RM_MESH_ARGS, float cos2_max, const int* npts, const long long* poff, float* pts, hipStream_t stream) {
    return rm_points(1, RM_MESH, cos2_max, 0.0f, npts, poff, pts, stream);
}
extern "C" int nu_rm_flip_claim(RM_MESH_ARGS, float cos2_max, const int* npts, const long long* poff, const int* pidx,
                                unsigned long long* ckey, unsigned long long* claim, int* win, hipStream_t stream) {
    return rm_claim(1, RM_MESH, cos2_max, npts, poff, pidx, ckey, claim, win, stream);
}
extern "C" int nu_rm_flip_apply(RM_MESH_ARGS, const int* win, int* F_io, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !win || !F_io) return NU_ERR_ARG;
    const int nh = 3 * nf;
    hipLaunchKernelGGL(rm_flip_apply_kernel, dim3((unsigned)nu_cdiv(nh, 256)), dim3(256), 0, stream, m, nh, win, F_io);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ relaxation + projection
// unlocked vertex with faces: p + (c - p) minus its component along N, where c = sum_g w_g cen_g / sum_g w_g over the incident faces
// in corner order (w_g = |n_g| = twice the area, cen_g = ((x + y) + z) / 3, n_g = (y - x) x (z - x)) and N = sum_g n_g (the
// area-weighted normal: no transcendental, so the numpy port matches bit for bit).  Jacobi: reads V, writes Vout.
__global__ __launch_bounds__(256) void rm_relax_kernel(RmMesh m, float* __restrict__ Vout) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.nv) return;
    float p[3];
    rm_ld(m.V, v, p);
    float out[3] = {p[0], p[1], p[2]};
    if (!m.vlock[v] && rm_deg(m, v) > 0) {
        float sc[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f}, sw = 0.f;
        for (int c = m.vc_off[v]; c < m.vc_off[v + 1]; ++c) {
            const int g = m.vc_corner[c] / 3;
            float x[3], y[3], z[3], n[3];
            rm_ld(m.V, m.F[3 * g], x);
            rm_ld(m.V, m.F[3 * g + 1], y);
            rm_ld(m.V, m.F[3 * g + 2], z);
            rm_normal(x, y, z, n);
            const float w = sqrtf(rm_dot(n, n));
            for (int k = 0; k < 3; ++k) {
                sc[k] = sc[k] + (((x[k] + y[k]) + z[k]) / 3.0f) * w;
                N[k] = N[k] + n[k];
            }
            sw = sw + w;
        }
        if (sw > 0.0f) {
            float d[3];
            for (int k = 0; k < 3; ++k) d[k] = sc[k] / sw - p[k];
            const float nn = rm_dot(N, N);
            if (nn > 0.0f) {
                const float t = rm_dot(N, d) / nn;
                for (int k = 0; k < 3; ++k) d[k] = d[k] - N[k] * t;
            }
            for (int k = 0; k < 3; ++k) out[k] = p[k] + d[k];
        }
    }
    for (int k = 0; k < 3; ++k) Vout[3LL * v + k] = out[k];
}

__global__ __launch_bounds__(256) void rm_project_kernel(const float* __restrict__ V, int nv, const unsigned char* __restrict__ vlock,
                                                         const float* __restrict__ Q, float* __restrict__ Vout) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3LL * nv) return;
    Vout[i] = vlock[i / 3] ? V[i] : Q[i];
}

extern "C" int nu_rm_relax(RM_MESH_ARGS, float* Vout, hipStream_t stream) {
    const RmMesh m = RM_MESH;
    if (!rm_mesh_ok(m) || !Vout) return NU_ERR_ARG;
    hipLaunchKernelGGL(rm_relax_kernel, dim3((unsigned)nu_cdiv(nv, 256)), dim3(256), 0, stream, m, Vout);
    return nu_launch_status();
}

extern "C" int nu_rm_project(const float* V, int nv, const unsigned char* vlock, const float* closest, float* Vout, hipStream_t stream) {
    if (nv <= 0 || !V || !vlock || !closest || !Vout) return NU_ERR_ARG;
    hipLaunchKernelGGL(rm_project_kernel, dim3((unsigned)nu_cdivl(3LL * nv, 256)), dim3(256), 0, stream, V, nv, vlock, closest, Vout);
    return nu_launch_status();
}
