// components.hip -- connected components of a triangle mesh on the device: labelling, per-component statistics and compaction
// (the floater / bubble removal the reference's authors did by hand: their scripts read *_fixed.ply meshes).  The driver, the sorts
// and the scans are in nu_nerf_amd/components.py; DESIGN.md 23.
//
// Labelling: hook-and-compress over a link list links[nl,2] (node pairs) on parent[n].  The same kernels serve both connectivities:
//   vertex   nodes = vertices, links = (v0, v1) and (v1, v2) of every face
//   edge     nodes = faces, links = the faces of consecutive equal keys in the stably sorted half-edge keys of nu_rm_edge_keys
// One round is three launches: hook (per link, the larger root's parent = atomicMin with the smaller root), compress (every node
// points at its root), check (one flag: some link still joins two roots).  The driver reads the flag once per round.
// Invariants the code has by construction:
//   parent[x] <= x   parent starts as the identity and is only ever lowered (atomicMin with a smaller id, or a store of an
//                    ancestor), so every walk x -> parent[x] is a strictly decreasing integer and ends; no workgroup waits on another
//                    and nothing spins on a flag
//   staleness        a load of parent in the hook kernel may be an older value; every value parent[x] ever held is an ancestor of x
//                    in the same component, so the walk still ends at a node of that component.  A hook made from a stale root, or
//                    an atomicMin that replaces another link's hook, can leave a link unjoined: the check pass (its own launch,
//                    behind the kernel boundary) sees it and the driver runs another round.  Stale costs rounds, never correctness
// At the fixed point every link has both nodes under one root, a root is the smallest id of its tree, so the labels are the smallest
// node id of each component whatever the arrival order: bit-reproducible.  Integer atomics only.
//
// Statistics: counts by integer atomicAdd (exact in any order; one add per wave and component); area and signed volume in float64
// by a fixed-order segmented reduction over the faces sorted stably by label (a segment cut into NU_CC_PARTS slices, a slice summed
// by one workgroup: thread-strided partial sums, then a fixed LDS tree; the slices summed in slice order).
#include "nu_common.h"

#pragma clang fp contract(off)

#define CC_SENTINEL 0x7fffffffffffffffLL

static __device__ inline int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x: parent[x] <= x, so x strictly decreases until parent[x] == x
static __device__ inline int cc_root(const int* parent, int x) {
    int p;
    while ((p = cc_load(parent + x)) < x && p >= 0) x = p;
    return x;
}

// ------------------------------------------------------------------------------------------------ links
__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n) parent[x] = x;
}

__global__ __launch_bounds__(256) void cc_vertex_links_kernel(const int* __restrict__ F, int nf, int* __restrict__ links) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int a = F[3LL * f], b = F[3LL * f + 1], c = F[3LL * f + 2];
    int* l = links + 4LL * f;
    l[0] = a; l[1] = b; l[2] = b; l[3] = c;
}

__global__ __launch_bounds__(256) void cc_edge_links_kernel(const long long* __restrict__ skeys, const long long* __restrict__ perm,
                                                            int nh, int* __restrict__ links) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nh) return;
    const long long k = skeys[i];
    const int f = (int)(perm[i] / 3);
    int g = f;
    if (i > 0 && k != CC_SENTINEL && skeys[i - 1] == k) g = (int)(perm[i - 1] / 3);
    links[2LL * i] = g;
    links[2LL * i + 1] = f;
}

// ------------------------------------------------------------------------------------------------ one round
__global__ __launch_bounds__(256) void cc_hook_kernel(int* __restrict__ parent, int n, const int* __restrict__ links, int nl) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const int a = links[2LL * l], b = links[2LL * l + 1];
    if (a == b || (unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n) return;
    const int ra = cc_root(parent, a), rb = cc_root(parent, b);
    if (ra == rb) return;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    atomicMin(parent + hi, lo);
}

__global__ __launch_bounds__(256) void cc_compress_kernel(int* __restrict__ parent, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int p = parent[x];
    const int r = cc_root(parent, p < x && p >= 0 ? p : x);
    if (r != p) parent[x] = r;        // x's only writer in this launch; r is an ancestor of x, so parent[x] <= x stays
}

__global__ __launch_bounds__(256) void cc_check_kernel(const int* __restrict__ parent, int n, const int* __restrict__ links, int nl,
                                                       int* __restrict__ flag) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    bool open = false;
    if (l < nl) {
        const int a = links[2LL * l], b = links[2LL * l + 1];
        if (a != b && (unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n) open = parent[a] != parent[b];
    }
    if (__any(open) && (threadIdx.x & (NU_WAVE - 1)) == 0) atomicOr(flag, 1);
}

// ------------------------------------------------------------------------------------------------ labels
__global__ __launch_bounds__(256) void cc_mark_used_kernel(const int* __restrict__ F, int nh, int nv, int* __restrict__ used) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    const int v = F[h];
    if ((unsigned)v < (unsigned)nv) used[v] = 1;
}

__global__ __launch_bounds__(256) void cc_root_flags_kernel(const int* __restrict__ parent, const int* __restrict__ used, int n,
                                                            int* __restrict__ isroot) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    isroot[x] = (parent[x] == x && (used == nullptr || used[x])) ? 1 : 0;
}

__global__ __launch_bounds__(256) void cc_labels_kernel(const int* __restrict__ parent, const int* __restrict__ used,
                                                        const long long* __restrict__ rinc, int n, int* __restrict__ label) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int r = parent[x];
    label[x] = (used != nullptr && !used[x]) || (unsigned)r >= (unsigned)n ? -1 : (int)(rinc[r] - 1);
}

__global__ __launch_bounds__(256) void cc_face_labels_kernel(const int* __restrict__ F, int nf, const int* __restrict__ vlabel,
                                                             int* __restrict__ flabel) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < nf) flabel[f] = vlabel[F[3LL * f]];
}

// ------------------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(256) void cc_keep_flags_kernel(const int* __restrict__ F, int nf, int nv, const int* __restrict__ flabel,
                                                            const int* __restrict__ keep_comp, int C, int* __restrict__ fkeep,
                                                            int* __restrict__ vkeep) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int c = flabel[f];
    const int k = (unsigned)c < (unsigned)C && keep_comp[c] ? 1 : 0;
    fkeep[f] = k;
    if (!k) return;
    for (int s = 0; s < 3; ++s) {
        const int v = F[3LL * f + s];
        if ((unsigned)v < (unsigned)nv) vkeep[v] = 1;
    }
}

__global__ __launch_bounds__(256) void cc_compact_vertices_kernel(const float* __restrict__ V, int nv, const int* __restrict__ vkeep,
                                                                  const long long* __restrict__ vinc, float* __restrict__ Vout) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || !vkeep[v]) return;
    const long long o = vinc[v] - 1;
    for (int k = 0; k < 3; ++k) Vout[3 * o + k] = V[3LL * v + k];
}

__global__ __launch_bounds__(256) void cc_compact_faces_kernel(const int* __restrict__ F, int nf, int nv, const int* __restrict__ fkeep,
                                                               const long long* __restrict__ finc, const long long* __restrict__ vinc,
                                                               int* __restrict__ Fout) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || !fkeep[f]) return;
    const long long o = finc[f] - 1;
    for (int s = 0; s < 3; ++s) {
        const int v = F[3LL * f + s];
        Fout[3 * o + s] = (unsigned)v < (unsigned)nv ? (int)(vinc[v] - 1) : -1;
    }
}

// ------------------------------------------------------------------------------------------------ statistics
// slice p of component c: thread t sums its faces s0 + t, s0 + t + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void cc_face_parts_kernel(const float* __restrict__ V, const int* __restrict__ F,
                                                            const long long* __restrict__ order, const long long* __restrict__ foff,
                                                            int C, double* __restrict__ part, float* __restrict__ pbox) {
    __shared__ double sa[256], sv[256];
    __shared__ float sb[6][256];
    const int t = threadIdx.x, p = blockIdx.x;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const long long s = foff[c], e = foff[c + 1];
        const long long per = (e - s + NU_CC_PARTS - 1) / NU_CC_PARTS;
        const long long s0 = s + p * per, e0 = s0 + per < e ? s0 + per : e;
        double area = 0.0, vol = 0.0;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long long i = s0 + t; i < e0; i += 256) {
            const long long f = order[i];
            double q[3][3];
            for (int j = 0; j < 3; ++j) {
                const long long v = F[3 * f + j];
                for (int k = 0; k < 3; ++k) {
                    const float x = V[3 * v + k];
                    lo[k] = fminf(lo[k], x);
                    hi[k] = fmaxf(hi[k], x);
                    q[j][k] = (double)x;
                }
            }
            const double* a = q[0];
            const double* b = q[1];
            const double* d = q[2];
            const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
            const double n0 = u[1] * w[2] - u[2] * w[1], n1 = u[2] * w[0] - u[0] * w[2], n2 = u[0] * w[1] - u[1] * w[0];
            area += 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            const double c0 = b[1] * d[2] - b[2] * d[1], c1 = b[2] * d[0] - b[0] * d[2], c2 = b[0] * d[1] - b[1] * d[0];
            vol += ((a[0] * c0 + a[1] * c1) + a[2] * c2) / 6.0;
        }
        sa[t] = area;
        sv[t] = vol;
        for (int k = 0; k < 3; ++k) {
            sb[k][t] = lo[k];
            sb[3 + k][t] = hi[k];
        }
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) {
                sa[t] += sa[t + o];
                sv[t] += sv[t + o];
                for (int k = 0; k < 3; ++k) {
                    sb[k][t] = fminf(sb[k][t], sb[k][t + o]);
                    sb[3 + k][t] = fmaxf(sb[3 + k][t], sb[3 + k][t + o]);
                }
            }
            __syncthreads();
        }
        if (t == 0) {
            const long long r = (long long)c * NU_CC_PARTS + p;
            part[2 * r] = sa[0];
            part[2 * r + 1] = sv[0];
            for (int k = 0; k < 6; ++k) pbox[6 * r + k] = sb[k][0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cc_face_final_kernel(const double* __restrict__ part, const float* __restrict__ pbox, int C,
                                                            double* __restrict__ area, double* __restrict__ volume,
                                                            float* __restrict__ aabb) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, v = 0.0;
    float box[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int p = 0; p < NU_CC_PARTS; ++p) {
        const long long r = (long long)c * NU_CC_PARTS + p;
        a += part[2 * r];
        v += part[2 * r + 1];
        for (int k = 0; k < 3; ++k) {
            box[k] = fminf(box[k], pbox[6 * r + k]);
            box[3 + k] = fmaxf(box[3 + k], pbox[6 * r + 3 + k]);
        }
    }
    area[c] = a;
    volume[c] = v;
    for (int k = 0; k < 6; ++k) aabb[6LL * c + k] = box[k];
}

// counts[stride * c + k] += number of lanes with `on`, component c and flag[k] set: the lanes of a wave that share a component add
// once, through their first lane (almost every lane of a wave lies in the one large component, and a per-lane atomicAdd would queue
// millions of adds on one address).  Every lane of the wave must call it; at most 64 turns, one per distinct component.
template <int K>
static __device__ inline void cc_wave_count(int* counts, int c, bool on, const bool (&flag)[K]) {
    const int lane = threadIdx.x & (NU_WAVE - 1);
    unsigned long long todo = __ballot(on);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(c, leader, NU_WAVE);
        const bool mine = on && c == lc;
        int n[K];
        for (int k = 0; k < K; ++k) n[k] = __popcll(__ballot(mine && flag[k]));
        if (lane == leader)
            for (int k = 0; k < K; ++k)
                if (n[k]) atomicAdd(counts + (long long)K * lc + k, n[k]);
        todo &= ~__ballot(mine);
    }
}

// per run of equal keys (at its first slot): one unique edge of the component of its first face; 1 face: boundary, >= 3: non-manifold
__global__ __launch_bounds__(256) void cc_edge_counts_kernel(const long long* __restrict__ skeys, const long long* __restrict__ perm,
                                                             int nh, const int* __restrict__ flabel, int C, int* __restrict__ ecount) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    int c = 0, n = 0;
    if (i < nh) {
        const long long k = skeys[i];
        if (k != CC_SENTINEL && !(i > 0 && skeys[i - 1] == k)) {
            n = 1;
            while (i + n < nh && n < 3 && skeys[i + n] == k) ++n;
            c = flabel[perm[i] / 3];
            on = (unsigned)c < (unsigned)C;
        }
    }
    const bool flag[3] = {true, n == 1, n >= 3};
    cc_wave_count<3>(ecount, c, on, flag);
}

__global__ __launch_bounds__(256) void cc_corner_keys_kernel(const int* __restrict__ F, int nh, const int* __restrict__ flabel,
                                                             long long* __restrict__ keys) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    keys[h] = ((long long)flabel[h / 3] << 32) | (long long)(unsigned)F[h];
}

__global__ __launch_bounds__(256) void cc_vertex_counts_kernel(const long long* __restrict__ skeys, int nh, int C,
                                                               int* __restrict__ vcount) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    int c = 0;
    if (i < nh) {
        const long long k = skeys[i];
        c = (int)(k >> 32);
        on = !(i > 0 && skeys[i - 1] == k) && (unsigned)c < (unsigned)C;
    }
    const bool flag[1] = {true};
    cc_wave_count<1>(vcount, c, on, flag);
}

// ------------------------------------------------------------------------------------------------ entries
#define CC_GRID(n) dim3((unsigned)nu_cdiv((n), 256)), dim3(256), 0, stream

static inline bool cc_bad_faces(int nf) { return nf <= 0 || 3LL * nf >= (1LL << 31); }

extern "C" int nu_cc_init(int* parent, int n, hipStream_t stream) {
    if (n <= 0 || !parent) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_init_kernel, CC_GRID(n), parent, n);
    return nu_launch_status();
}

extern "C" int nu_cc_vertex_links(const int* F, int nf, int* links, hipStream_t stream) {
    if (cc_bad_faces(nf) || !F || !links) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_vertex_links_kernel, CC_GRID(nf), F, nf, links);
    return nu_launch_status();
}

extern "C" int nu_cc_edge_links(const long long* skeys, const long long* perm, int nh, int* links, hipStream_t stream) {
    if (nh <= 0 || !skeys || !perm || !links) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_edge_links_kernel, CC_GRID(nh), skeys, perm, nh, links);
    return nu_launch_status();
}

extern "C" int nu_cc_hook(int* parent, int n, const int* links, int nl, hipStream_t stream) {
    if (n <= 0 || nl <= 0 || !parent || !links) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_hook_kernel, CC_GRID(nl), parent, n, links, nl);
    return nu_launch_status();
}

extern "C" int nu_cc_compress(int* parent, int n, hipStream_t stream) {
    if (n <= 0 || !parent) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_compress_kernel, CC_GRID(n), parent, n);
    return nu_launch_status();
}

extern "C" int nu_cc_check(const int* parent, int n, const int* links, int nl, int* flag, hipStream_t stream) {
    if (n <= 0 || nl <= 0 || !parent || !links || !flag) return NU_ERR_ARG;
    if (hipMemsetAsync(flag, 0, sizeof(int), stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_check_kernel, CC_GRID(nl), parent, n, links, nl, flag);
    return nu_launch_status();
}

extern "C" int nu_cc_mark_used(const int* F, int nf, int nv, int* used, hipStream_t stream) {
    if (cc_bad_faces(nf) || nv <= 0 || !F || !used) return NU_ERR_ARG;
    if (hipMemsetAsync(used, 0, sizeof(int) * (size_t)nv, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_mark_used_kernel, CC_GRID(3 * nf), F, 3 * nf, nv, used);
    return nu_launch_status();
}

extern "C" int nu_cc_root_flags(const int* parent, const int* used, int n, int* isroot, hipStream_t stream) {
    if (n <= 0 || !parent || !isroot) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_root_flags_kernel, CC_GRID(n), parent, used, n, isroot);
    return nu_launch_status();
}

extern "C" int nu_cc_labels(const int* parent, const int* used, const long long* rinc, int n, int* label, hipStream_t stream) {
    if (n <= 0 || !parent || !rinc || !label) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_labels_kernel, CC_GRID(n), parent, used, rinc, n, label);
    return nu_launch_status();
}

extern "C" int nu_cc_face_labels(const int* F, int nf, const int* vlabel, int* flabel, hipStream_t stream) {
    if (cc_bad_faces(nf) || !F || !vlabel || !flabel) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_face_labels_kernel, CC_GRID(nf), F, nf, vlabel, flabel);
    return nu_launch_status();
}

extern "C" int nu_cc_keep_flags(const int* F, int nf, int nv, const int* flabel, const int* keep_comp, int C, int* fkeep, int* vkeep,
                                hipStream_t stream) {
    if (cc_bad_faces(nf) || nv <= 0 || C <= 0 || !F || !flabel || !keep_comp || !fkeep || !vkeep) return NU_ERR_ARG;
    if (hipMemsetAsync(vkeep, 0, sizeof(int) * (size_t)nv, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_keep_flags_kernel, CC_GRID(nf), F, nf, nv, flabel, keep_comp, C, fkeep, vkeep);
    return nu_launch_status();
}

extern "C" int nu_cc_compact(const float* V, int nv, const int* F, int nf, const int* fkeep, const long long* finc, const int* vkeep,
                             const long long* vinc, float* Vout, int* Fout, hipStream_t stream) {
    if (cc_bad_faces(nf) || nv <= 0 || !V || !F || !fkeep || !finc || !vkeep || !vinc || !Vout || !Fout) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_compact_vertices_kernel, CC_GRID(nv), V, nv, vkeep, vinc, Vout);
    hipLaunchKernelGGL(cc_compact_faces_kernel, CC_GRID(nf), F, nf, nv, fkeep, finc, vinc, Fout);
    return nu_launch_status();
}

extern "C" int nu_cc_face_stats(const float* V, const int* F, int nf, const long long* order, const long long* foff, int C,
                                double* part, float* pbox, double* area, double* volume, float* aabb, hipStream_t stream) {
    if (cc_bad_faces(nf) || C <= 0 || !V || !F || !order || !foff || !part || !pbox || !area || !volume || !aabb) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_face_parts_kernel, dim3(NU_CC_PARTS, (unsigned)(C < 65535 ? C : 65535)), dim3(256), 0, stream, V, F, order,
                       foff, C, part, pbox);
    hipLaunchKernelGGL(cc_face_final_kernel, CC_GRID(C), part, pbox, C, area, volume, aabb);
    return nu_launch_status();
}

extern "C" int nu_cc_edge_counts(const long long* skeys, const long long* perm, int nh, const int* flabel, int C, int* ecount,
                                 hipStream_t stream) {
    if (nh <= 0 || C <= 0 || !skeys || !perm || !flabel || !ecount) return NU_ERR_ARG;
    if (hipMemsetAsync(ecount, 0, sizeof(int) * 3 * (size_t)C, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_edge_counts_kernel, CC_GRID(nh), skeys, perm, nh, flabel, C, ecount);
    return nu_launch_status();
}

extern "C" int nu_cc_corner_keys(const int* F, int nf, const int* flabel, long long* keys, hipStream_t stream) {
    if (cc_bad_faces(nf) || !F || !flabel || !keys) return NU_ERR_ARG;
    hipLaunchKernelGGL(cc_corner_keys_kernel, CC_GRID(3 * nf), F, 3 * nf, flabel, keys);
    return nu_launch_status();
}

extern "C" int nu_cc_vertex_counts(const long long* skeys, int nh, int C, int* vcount, hipStream_t stream) {
    if (nh <= 0 || C <= 0 || !skeys || !vcount) return NU_ERR_ARG;
    if (hipMemsetAsync(vcount, 0, sizeof(int) * (size_t)C, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_vertex_counts_kernel, CC_GRID(nh), skeys, nh, C, vcount);
    return nu_launch_status();
}
