// lbvh.hip -- linear BVH build + closest-hit traversal over a triangle mesh (gfx950).
//
// Replaces the reference's OptiX path: GAS build (network/tracing_optix.py:20-23, :142-146), the
// 1xN launch (:74-117, :154-158) and the three device programs of cuda/triangle.cu:48-99
//   raygen: one closest-hit trace per ray, tmin = 0, tmax = 1e16, no face culling
//   miss  : (hit, index) = (0.0, 10000000)      closesthit: (1.0, primitive index)
// Build = Morton codes of triangle centroids -> sort -> Karras 2012 radix-tree hierarchy -> bottom-up
// AABB refit -> 4-wide records (each node's grandchildren).  Traversal = four lanes per ray over the 4-wide records, one
// stack per ray in LDS, nearest entry first (lbvh_trace_quad_kernel).
//
// Hit indices are defined bit-exactly against the brute-force oracle (oracle/lbvh_oracle.py): the
// ray/triangle test below is written with explicit single-rounding fp32 operations in a fixed order, ties in t go
// to the lowest face id, and boxes are padded so that traversal never culls a triangle the test would accept.
#include "nu_common.h"
#include "relight.h"
#include <stdlib.h>

// Bit-exact parity with the oracle needs one rounding per operation.  HIP's __fmul_rn/__fadd_rn are header-defined
// plain operators that still carry the 'contract' flag, so the arithmetic is written with ordinary operators and FMA
// contraction is switched off for this whole file.
#pragma clang fp contract(off)

#define NU_MISS_INDEX 10000000
#define NU_STACK 64

struct NuBvhNode {           // 64 bytes: both child boxes inline
    float lmin[3], lmax[3];
    float rmin[3], rmax[3];
    int left, right;         // >= 0: internal node index; < 0: leaf, sorted position = -1 - value
    int parent, pad;
};

struct NuBvhHeader {
    int n_faces, n_pad, n_verts, pad;
    float bmin[3], bmax[3], eps, pad2;
};

// ---- memory layout inside the caller's buffer -------------------------------------------------
static __host__ __device__ inline long long nu_align256(long long x) { return (x + 255) / 256 * 256; }
// 4-wide view of the same tree (one record per binary internal node: its grandchildren, or a child that is a leaf), traversed
// by the small-batch kernel with four lanes per ray.  Entry = 32 bytes: box, child reference.
#define NU_WIDE_EMPTY ((int)0x80000000)
struct NuBvhWideEntry {
    float bmin[3], bmax[3];
    int ref;                 // >= 0: internal node index (its wide record); < 0: leaf, sorted position = -1 - value; NU_WIDE_EMPTY: unused
    int pad;
};
struct NuBvhLayout {
    long long header, keys, nodes, leaf_parent, counters, tris, ids, bounds_i, wide, total;
};
static __host__ __device__ inline NuBvhLayout nu_bvh_layout(int n) {
    int npad = 1;
    while (npad < n) npad <<= 1;
    NuBvhLayout L;
    long long o = 0;
    L.header = o; o = nu_align256(o + sizeof(NuBvhHeader));
    L.keys = o; o = nu_align256(o + (long long)npad * 8);
    L.nodes = o; o = nu_align256(o + (long long)(n > 1 ? n - 1 : 1) * sizeof(NuBvhNode));
    L.leaf_parent = o; o = nu_align256(o + (long long)n * 4);
    L.counters = o; o = nu_align256(o + (long long)n * 4);
    L.tris = o; o = nu_align256(o + (long long)n * 48);      // 3 vertices x (x,y,z,pad)
    L.ids = o; o = nu_align256(o + (long long)n * 4);
    L.bounds_i = o; o = nu_align256(o + 32);
    L.wide = o; o = nu_align256(o + (long long)(n > 1 ? n - 1 : 1) * 4 * sizeof(NuBvhWideEntry));
    L.total = o;
    return L;
}
extern "C" long long nu_lbvh_bytes(int n_faces) { return nu_bvh_layout(n_faces).total; }

// order-preserving float <-> int maps for atomicMin/Max
static __device__ inline int nu_f2ord(float f) { int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
static __device__ inline float nu_ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void lbvh_init_kernel(char* buf, NuBvhLayout L, int n, int npad, int nv) {
    NuBvhHeader* h = (NuBvhHeader*)(buf + L.header);
    int* b = (int*)(buf + L.bounds_i);
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        h->n_faces = n; h->n_pad = npad; h->n_verts = nv;
        for (int c = 0; c < 3; ++c) { b[c] = 0x7fffffff; b[3 + c] = (int)0x80000000; }
    }
    int* cnt = (int*)(buf + L.counters);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) cnt[i] = 0;
}

__global__ void lbvh_bounds_kernel(const float* __restrict__ V, const int* __restrict__ F, int n, char* buf, NuBvhLayout L) {
    int* b = (int*)(buf + L.bounds_i);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c[3];
    for (int k = 0; k < 3; ++k)
        c[k] = (V[F[i * 3] * 3LL + k] + V[F[i * 3 + 1] * 3LL + k] + V[F[i * 3 + 2] * 3LL + k]) * (1.0f / 3.0f);
    for (int k = 0; k < 3; ++k) { atomicMin(&b[k], nu_f2ord(c[k])); atomicMax(&b[3 + k], nu_f2ord(c[k])); }
}

static __device__ inline unsigned nu_expand10(unsigned v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__global__ void lbvh_morton_kernel(const float* __restrict__ V, const int* __restrict__ F, int n, int npad, char* buf,
                                   NuBvhLayout L) {
    const int* b = (const int*)(buf + L.bounds_i);
    unsigned long long* keys = (unsigned long long*)(buf + L.keys);
    NuBvhHeader* h = (NuBvhHeader*)(buf + L.header);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = nu_ord2f(b[k]); hi[k] = nu_ord2f(b[3 + k]); }
    if (i == 0) {
        float diag = 0.f;
        for (int k = 0; k < 3; ++k) { h->bmin[k] = lo[k]; h->bmax[k] = hi[k]; diag += (hi[k] - lo[k]) * (hi[k] - lo[k]); }
        h->eps = 1e-5f * fmaxf(sqrtf(diag), 1e-3f);
    }
    if (i >= npad) return;
    if (i >= n) { keys[i] = ~0ull; return; }
    unsigned code = 0;
    for (int k = 0; k < 3; ++k) {
        const float c = (V[F[i * 3] * 3LL + k] + V[F[i * 3 + 1] * 3LL + k] + V[F[i * 3 + 2] * 3LL + k]) * (1.0f / 3.0f);
        const float ext = fmaxf(hi[k] - lo[k], 1e-20f);
        float u = (c - lo[k]) / ext;
        u = fminf(fmaxf(u * 1024.0f, 0.0f), 1023.0f);
        code |= nu_expand10((unsigned)u) << (2 - k);
    }
    keys[i] = ((unsigned long long)code << 32) | (unsigned)i;
}

__global__ void lbvh_bitonic_kernel(unsigned long long* keys, int npad, int j, int k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    const int l = i ^ j;
    if (l > i) {
        const unsigned long long a = keys[i], b = keys[l];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { keys[i] = b; keys[l] = a; }
    }
}

// gather triangles in sorted order (+ ids)
__global__ void lbvh_gather_kernel(const float* __restrict__ V, const int* __restrict__ F, int n, char* buf, NuBvhLayout L) {
    const unsigned long long* keys = (const unsigned long long*)(buf + L.keys);
    float* tris = (float*)(buf + L.tris);
    int* ids = (int*)(buf + L.ids);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int f = (int)(keys[p] & 0xffffffffu);
    ids[p] = f;
    for (int v = 0; v < 3; ++v) {
        const int vi = F[f * 3 + v];
        for (int k = 0; k < 3; ++k) tris[p * 12LL + v * 4 + k] = V[vi * 3LL + k];
        tris[p * 12LL + v * 4 + 3] = 0.f;
    }
}

static __device__ inline int nu_delta(const unsigned long long* __restrict__ keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return __clzll(keys[i] ^ keys[j]);
}

// Karras 2012: one thread per internal node
__global__ void lbvh_hierarchy_kernel(int n, char* buf, NuBvhLayout L) {
    const unsigned long long* keys = (const unsigned long long*)(buf + L.keys);
    NuBvhNode* nodes = (NuBvhNode*)(buf + L.nodes);
    int* leaf_parent = (int*)(buf + L.leaf_parent);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (nu_delta(keys, n, i, i + 1) - nu_delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = nu_delta(keys, n, i, i - d);
    int lmax = 2;
    while (nu_delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (nu_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = nu_delta(keys, n, i, j);
    int s = 0;
    for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (nu_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t == 1) break;
    }
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int left = (lo == gamma) ? -1 - gamma : gamma;
    const int right = (hi == gamma + 1) ? -1 - (gamma + 1) : gamma + 1;
    nodes[i].left = left;
    nodes[i].right = right;
    if (i == 0) nodes[i].parent = -1;
    if (left >= 0) nodes[left].parent = i; else leaf_parent[gamma] = i;
    if (right >= 0) nodes[right].parent = i; else leaf_parent[gamma + 1] = i;
}

// bottom-up refit: leaf threads climb; the second arriver at a node owns it
__global__ void lbvh_refit_kernel(int n, char* buf, NuBvhLayout L) {
    NuBvhNode* nodes = (NuBvhNode*)(buf + L.nodes);
    const int* leaf_parent = (const int*)(buf + L.leaf_parent);
    int* counters = (int*)(buf + L.counters);
    const float* tris = (const float*)(buf + L.tris);
    const NuBvhHeader* h = (const NuBvhHeader*)(buf + L.header);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float eps = h->eps;
    float bmin[3], bmax[3];
    for (int k = 0; k < 3; ++k) {
        const float a = tris[p * 12LL + k], b = tris[p * 12LL + 4 + k], c = tris[p * 12LL + 8 + k];
        bmin[k] = fminf(a, fminf(b, c)) - eps;
        bmax[k] = fmaxf(a, fmaxf(b, c)) + eps;
    }
    int child = -1 - p;
    int node = leaf_parent[p];
    while (node >= 0) {
        NuBvhNode* nd = &nodes[node];
        volatile float* dmin = (nd->left == child) ? nd->lmin : nd->rmin;
        volatile float* dmax = (nd->left == child) ? nd->lmax : nd->rmax;
        for (int k = 0; k < 3; ++k) { dmin[k] = bmin[k]; dmax[k] = bmax[k]; }
        __threadfence();
        const int prev = atomicAdd(&counters[node], 1);
        if (prev == 0) return;      // sibling subtree not finished: its thread continues upwards
        __threadfence();
        volatile NuBvhNode* vn = nd;
        for (int k = 0; k < 3; ++k) {
            bmin[k] = fminf(vn->lmin[k], vn->rmin[k]);
            bmax[k] = fmaxf(vn->lmax[k], vn->rmax[k]);
        }
        child = node;
        node = nd->parent;
    }
}

// Every (j, k) step of the sorting network whose partner distance j fits inside one NU_SORT_TILE-key tile is executed from
// LDS: one launch covers k = 2 .. NU_SORT_TILE completely, and for each larger k the tail j = NU_SORT_TILE/2 .. 1.  Same
// comparators as lbvh_bitonic_kernel in the same order, hence the same permutation; 10 launches instead of 120 at 32768 keys.
#define NU_SORT_TILE 4096
__global__ __launch_bounds__(256) void lbvh_bitonic_local_kernel(unsigned long long* keys, int npad, int k_first, int k_last) {
    __shared__ unsigned long long sk[NU_SORT_TILE];
    const int base = blockIdx.x * NU_SORT_TILE;
    const int tile = npad < NU_SORT_TILE ? npad : NU_SORT_TILE;
    for (int t = threadIdx.x; t < tile; t += 256) sk[t] = keys[base + t];
    __syncthreads();
    for (int k = k_first; k <= k_last; k <<= 1) {
        for (int j = (k >> 1) < (tile >> 1) ? (k >> 1) : (tile >> 1); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < tile; t += 256) {
                const int l = t ^ j;
                if (l > t) {
                    const unsigned long long a = sk[t], b = sk[l];
                    const bool up = ((base + t) & k) == 0;
                    if ((a > b) == up) { sk[t] = b; sk[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < tile; t += 256) keys[base + t] = sk[t];
}

// 4-wide records: node i -> the children of its two children (a child that is a leaf stands for itself); after the refit
__global__ void lbvh_widen_kernel(int n, char* buf, NuBvhLayout L) {
    const NuBvhNode* nodes = (const NuBvhNode*)(buf + L.nodes);
    NuBvhWideEntry* wide = (NuBvhWideEntry*)(buf + L.wide);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const NuBvhNode nd = nodes[i];
    NuBvhWideEntry e[4];
    int ne = 0;
    auto put = [&](const float* bmin, const float* bmax, int ref) {
        for (int k = 0; k < 3; ++k) { e[ne].bmin[k] = bmin[k]; e[ne].bmax[k] = bmax[k]; }
        e[ne].ref = ref; e[ne].pad = 0;
        ++ne;
    };
    for (int side = 0; side < 2; ++side) {
        const int c = side ? nd.right : nd.left;
        if (c < 0) {
            put(side ? nd.rmin : nd.lmin, side ? nd.rmax : nd.lmax, c);
        } else {
            const NuBvhNode nc = nodes[c];
            put(nc.lmin, nc.lmax, nc.left);
            put(nc.rmin, nc.rmax, nc.right);
        }
    }
    for (; ne < 4; ) {
        const float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        put(lo, hi, NU_WIDE_EMPTY);
    }
    for (int k = 0; k < 4; ++k) wide[i * 4LL + k] = e[k];
}

extern "C" int nu_lbvh_build(const float* V, int n_verts, const int* F, int n_faces, void* bvh, long long bvh_bytes,
                             hipStream_t stream) {
    if (n_faces <= 0 || n_verts <= 0) return NU_ERR_ARG;
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    if (bvh_bytes < L.total) return NU_ERR_WORKSPACE;
    int npad = 1;
    while (npad < n_faces) npad <<= 1;
    char* buf = (char*)bvh;
    const int T = 256;
    hipLaunchKernelGGL(lbvh_init_kernel, dim3(nu_cdiv(n_faces, T) < 1024 ? nu_cdiv(n_faces, T) : 1024), dim3(T), 0, stream, buf, L,
                       n_faces, npad, n_verts);
    hipLaunchKernelGGL(lbvh_bounds_kernel, dim3(nu_cdiv(n_faces, T)), dim3(T), 0, stream, V, F, n_faces, buf, L);
    hipLaunchKernelGGL(lbvh_morton_kernel, dim3(nu_cdiv(npad, T)), dim3(T), 0, stream, V, F, n_faces, npad, buf, L);
    unsigned long long* keys = (unsigned long long*)(buf + L.keys);
    {
        const int tile = npad < NU_SORT_TILE ? npad : NU_SORT_TILE;
        const int nblk = npad / tile;
        hipLaunchKernelGGL(lbvh_bitonic_local_kernel, dim3(nblk), dim3(256), 0, stream, keys, npad, 2, tile);
        for (int k = tile << 1; k <= npad; k <<= 1) {
            for (int j = k >> 1; j >= tile; j >>= 1)
                hipLaunchKernelGGL(lbvh_bitonic_kernel, dim3(nu_cdiv(npad, T)), dim3(T), 0, stream, keys, npad, j, k);
            hipLaunchKernelGGL(lbvh_bitonic_local_kernel, dim3(nblk), dim3(256), 0, stream, keys, npad, k, k);
        }
    }
    hipLaunchKernelGGL(lbvh_gather_kernel, dim3(nu_cdiv(n_faces, T)), dim3(T), 0, stream, V, F, n_faces, buf, L);
    if (n_faces > 1) {
        hipLaunchKernelGGL(lbvh_hierarchy_kernel, dim3(nu_cdiv(n_faces - 1, T)), dim3(T), 0, stream, n_faces, buf, L);
        hipLaunchKernelGGL(lbvh_refit_kernel, dim3(nu_cdiv(n_faces, T)), dim3(T), 0, stream, n_faces, buf, L);
        hipLaunchKernelGGL(lbvh_widen_kernel, dim3(nu_cdiv(n_faces - 1, T)), dim3(T), 0, stream, n_faces, buf, L);
    }
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// ray / triangle (Moeller-Trumbore, both facings), single-rounding fp32 ops in a fixed order
// ------------------------------------------------------------------------------------------------
static __device__ inline float nu_dot3_rn(const float* a, const float* b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];     // contraction is off in this file: one rounding per op
}
static __device__ inline void nu_cross_rn(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// returns true and t when the ray hits the triangle with tmin < t < tmax
static __device__ inline bool nu_ray_tri(const float* o, const float* d, const float* v0, const float* v1, const float* v2,
                                         float tmin, float tmax, float& t) {
    float e1[3], e2[3], pv[3], tv[3], qv[3];
    for (int k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; }
    nu_cross_rn(d, e2, pv);
    const float det = nu_dot3_rn(e1, pv);
    if (det == 0.0f) return false;
    const float inv = 1.0f / det;
    for (int k = 0; k < 3; ++k) tv[k] = o[k] - v0[k];
    const float u = nu_dot3_rn(tv, pv) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    nu_cross_rn(tv, e1, qv);
    const float v = nu_dot3_rn(d, qv) * inv;
    if (!(v >= 0.0f && (u + v) <= 1.0f)) return false;
    t = nu_dot3_rn(e2, qv) * inv;
    return t > tmin && t < tmax;
}

static __device__ inline bool nu_ray_box(const float* o, const float* invd, const float* bmin, const float* bmax, float tmin,
                                         float tbest, float& tnear) {
    float t0 = tmin, t1 = tbest;
    for (int k = 0; k < 3; ++k) {
        const float a = (bmin[k] - o[k]) * invd[k], b = (bmax[k] - o[k]) * invd[k];
        t0 = fmaxf(t0, fminf(a, b));      // fminf/fmaxf drop the NaN of 0 * inf
        t1 = fminf(t1, fmaxf(a, b));
    }
    tnear = t0;
    return t0 <= t1 * 1.0000005f;
}

// ------------------------------------------------------------------------------------------------
// FOUR lanes per ray over the 4-wide records (16 rays per single-wave workgroup).  A traversal is a chain of dependent fetches --
// a launch of 4 096 rays lasts as long as its longest chain (56 records at ~0.7 us; the average ray visits 13) -- so the lever
// is fewer and shorter links: the four lanes of a ray test the four entries of a wide record at once
// (two binary levels per fetch), leaf entries are intersected by the lanes that hold them, the hits are ordered inside the
// quad with DPP quad permutes and the ray's stack (one per quad, in LDS) takes the farther ones.  Closest hit, ties in t to the
// lowest face id, the box and triangle tests of this file: identical (hit, index, t) to the brute-force sweep.
// ------------------------------------------------------------------------------------------------
#define NU_WSTACK 96            // <= 3 pushes per wide level, <= 31 wide levels (a Morton tree over 62-bit keys)
template <int CTRL> static __device__ __forceinline__ int nu_quad_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL> static __device__ __forceinline__ float nu_quad_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
#define NU_QP_XOR1 0xB1         // quad_perm:[1,0,3,2]
#define NU_QP_XOR2 0x4E         // quad_perm:[2,3,0,1]
#define NU_QP_XOR3 0x1B         // quad_perm:[3,2,1,0]

// Ray sources of the traversal kernel.  begin() fetches (or computes) the ray of quad q of block blk and returns false when the quad
// has no ray; end() stores the verdict.  Every lane of a quad calls begin(); only lane 0 of the quad calls end().
struct NuRayBuffer {                       // rays [N,6] from memory -> (hit, idx, t) per ray: nu_lbvh_trace
    const float* __restrict__ rays;
    int N;
    float* __restrict__ hit;
    int* __restrict__ idx;
    float* __restrict__ tout;
    int r;
    __device__ __forceinline__ bool begin(int blk, int q, float* o, float* d) {
        r = blk * 16 + q;
        if (r >= N) return false;
        for (int k = 0; k < 3; ++k) { o[k] = rays[r * 6LL + k]; d[k] = rays[r * 6LL + 3 + k]; }
        return true;
    }
    __device__ __forceinline__ void end(int found, int best_id, float best_t) {
        hit[r] = found ? 1.0f : 0.0f;
        idx[r] = best_id;
        if (tout) tout[r] = found ? best_t : 0.0f;
    }
};

// The camera ray of pixel (x, y) in the real-capture convention (utils/render_mask_real.py:52-67, the ray store of
// renderer._construct_ray_batch): c = (x + 0.5, y + 0.5, 1), d = normalize(R^T (Kinv c)), o = -R^T t.  cam = Kinv [3x3] then the
// world -> camera [R|t] [3x4], both row-major.  Single-rounding fp32 operations in a fixed order (contraction is off in this file): the
// one definition nu_mask_pinhole_rays and nu_mask_pinhole_trace share, so the two are bit-identical.
#define NU_CAM_FLOATS 21
static __device__ inline void nu_pinhole_ray(const float* __restrict__ cam, int x, int y, float* o, float* d) {
    const float* Ki = cam;
    const float* P = cam + 9;
    const float c0 = (float)x + 0.5f, c1 = (float)y + 0.5f;
    float kc[3];
    for (int i = 0; i < 3; ++i) kc[i] = (Ki[i * 3] * c0 + Ki[i * 3 + 1] * c1) + Ki[i * 3 + 2];
    float v[3];
    for (int j = 0; j < 3; ++j) {
        v[j] = (P[j] * kc[0] + P[4 + j] * kc[1]) + P[8 + j] * kc[2];                       // (R^T kc)_j
        o[j] = -((P[j] * P[3] + P[4 + j] * P[7]) + P[8 + j] * P[11]);                      // -(R^T t)_j
    }
    const float n = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int j = 0; j < 3; ++j) d[j] = v[j] / n;
}

struct NuPinholeMask {                     // every pixel of n images -> uint8 0 / 255 per pixel: nu_mask_pinhole_trace
    const float* __restrict__ cams;        // [n, NU_CAM_FLOATS]
    int h, w, tiles_x, tiles;              // 4 x 4 pixel tiles per image, one tile per 16-ray wave
    unsigned char* __restrict__ out;       // [n, h, w]
    long long p;
    __device__ __forceinline__ bool begin(int blk, int q, float* o, float* d) {
        const int img = blk / tiles, t = blk - img * tiles;
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * 4 + (q & 3), y = ty * 4 + (q >> 2);
        if (x >= w || y >= h) return false;
        p = ((long long)img * h + y) * w + x;
        nu_pinhole_ray(cams + (long long)img * NU_CAM_FLOATS, x, y, o, d);
        return true;
    }
    __device__ __forceinline__ void end(int found, int, float) { out[p] = found ? 255 : 0; }
};

// (nu_walk_quad further down is this walk a second time, as a device function for the kernels that trace several dependent rays per
// quad: a change to the walk is made in both.  Calling it from here, with ANY_HIT passed as a constant, was tried and changes the
// compiler's figures of all four instantiations below -- VGPR 66 / 63 / 68 / 61 -> 72 / 59 / 72 / 59, SGPR 42 / 46 / 58 / 47 ->
// 42 / 44 / 52 / 41 (scripts/kernel_regs.py; LDS and scratch stay) -- so they keep their own code)
// ANY_HIT = false: closest hit (nu_lbvh_trace).  ANY_HIT = true: the ray ends as soon as a lane of its quad accepts a triangle; until
// then the running best is tmax, so the walk is step for step the closest-hit walk and `found` is the same predicate (the boxes are
// padded so that no accepted triangle is ever culled) -- only the (t, face id) of an any-hit are not the closest ones.
template <class RaySrc, bool ANY_HIT>
__global__ __launch_bounds__(64) void lbvh_trace_quad_kernel(const char* __restrict__ buf, NuBvhLayout L, RaySrc src, float tmin,
                                                             float tmax) {
    __shared__ int stack[NU_WSTACK][16];
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    float o[3], d[3], invd[3];
    if (!src.begin(blockIdx.x, q, o, d)) return;           // whole quads leave together
    const NuBvhHeader* h = (const NuBvhHeader*)(buf + L.header);
    const NuBvhWideEntry* wide = (const NuBvhWideEntry*)(buf + L.wide);
    const float* tris = (const float*)(buf + L.tris);
    const int* ids = (const int*)(buf + L.ids);
    const int n = h->n_faces;
    for (int k = 0; k < 3; ++k) invd[k] = 1.0f / d[k];
    float best_t = tmax;
    int best_id = NU_MISS_INDEX;
    int found = 0;

    // candidate of this lane -> best of the quad -> the ray's running best (every lane of the quad holds the same triple)
    auto merge = [&](int cf, float ct, int ci) {
#define NU_BETTER(f2, t2, i2) ((f2) && (!cf || (t2) < ct || ((t2) == ct && (i2) < ci)))
        { const int f2 = nu_quad_i<NU_QP_XOR1>(cf); const float t2 = nu_quad_f<NU_QP_XOR1>(ct); const int i2 = nu_quad_i<NU_QP_XOR1>(ci);
          if (NU_BETTER(f2, t2, i2)) { cf = 1; ct = t2; ci = i2; } }
        { const int f2 = nu_quad_i<NU_QP_XOR2>(cf); const float t2 = nu_quad_f<NU_QP_XOR2>(ct); const int i2 = nu_quad_i<NU_QP_XOR2>(ci);
          if (NU_BETTER(f2, t2, i2)) { cf = 1; ct = t2; ci = i2; } }
#undef NU_BETTER
        if (cf && (!found || ct < best_t || (ct == best_t && ci < best_id))) { best_t = ct; best_id = ci; found = 1; }
    };
    auto test_leaf = [&](int pos, int& cf, float& ct, int& ci) {
        const float* tp = tris + pos * 12LL;
        float t;
        if (nu_ray_tri(o, d, tp, tp + 4, tp + 8, tmin, tmax, t)) { cf = 1; ct = t; ci = ids[pos]; }
    };

    if (n == 1) {
        int cf = 0, ci = NU_MISS_INDEX;
        float ct = 0.f;
        if (sub == 0) test_leaf(0, cf, ct, ci);
        merge(cf, ct, ci);
    } else {
        int sp = 0;
#ifdef NU_LBVH_STATS
        int steps = 0;
#endif
        // The loop is arranged so that the two fetches of a step -- the triangle of a leaf entry that was hit, the next record --
        // are in flight TOGETHER: the triangle is requested, the next record is chosen (that needs the box distances only) and
        // requested, and only then is the triangle intersected.  The running best it may improve prunes from the next record on.
        NuBvhWideEntry e = wide[sub];
        while (true) {
#ifdef NU_LBVH_STATS
            ++steps;
#endif
            float tn;
            // inclusive in best_t: an equal-t hit with a lower face id must still be found
            const bool hb = e.ref != NU_WIDE_EMPTY && nu_ray_box(o, invd, e.bmin, e.bmax, tmin, ANY_HIT ? tmax : best_t, tn);
            const bool leaf = hb && e.ref < 0;
            const int pos = leaf ? -1 - e.ref : 0;
            float tv[9];
            int tid = NU_MISS_INDEX;
            if (leaf) {
#pragma unroll
                for (int v = 0; v < 3; ++v)
#pragma unroll
                    for (int k = 0; k < 3; ++k) tv[v * 3 + k] = tris[pos * 12LL + v * 4 + k];
                tid = ids[pos];
            }
            // internal entries that were hit: nearest first, the others on the ray's stack (farthest deepest)
            const int want = (hb && e.ref >= 0) ? 1 : 0;
            int rank = 0, cnt = want;
            { const int w2 = nu_quad_i<NU_QP_XOR1>(want); const float t2 = nu_quad_f<NU_QP_XOR1>(tn); const int s2 = sub ^ 1;
              cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
            { const int w2 = nu_quad_i<NU_QP_XOR2>(want); const float t2 = nu_quad_f<NU_QP_XOR2>(tn); const int s2 = sub ^ 2;
              cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
            { const int w2 = nu_quad_i<NU_QP_XOR3>(want); const float t2 = nu_quad_f<NU_QP_XOR3>(tn); const int s2 = sub ^ 3;
              cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
            int next = (want && rank == 0) ? e.ref : -1;
            next = max(next, nu_quad_i<NU_QP_XOR1>(next));
            next = max(next, nu_quad_i<NU_QP_XOR2>(next));
            if (want && rank > 0) stack[sp + (cnt - 1 - rank)][q] = e.ref;
            sp += cnt > 0 ? cnt - 1 : 0;
            bool done = false;
            if (cnt == 0) {
                // (measured and dropped: keeping the box distance beside each stacked record and skipping, at the pop, what the
                // running best has overtaken -- 12.9 -> 11.2 records per ray on average, but the longest chain of a batch, which
                // is what a launch waits for, stays at 56 records and the pop loop costs more than it saves: 38.8 -> 44.1 us;
                // subtrees of up to four triangles as ONE entry whose triangles are fetched together -- longest chain 56 -> 42
                // records, but every step then carries four triangle fetches: 39 -> 44 us at 4 096 rays, 2.7 -> 1.0 G rays/s at 2^20;
                // eight lanes per ray over 8-wide records -- three binary levels per fetch, profiles/r03/lbvh_eight_lanes_per_ray.patch --
                // bit-exact too, 37 / 32 us against 42 / 31 at 4 096 rays and 1.65 against 2.67 G rays/s at 2^20: a link costs
                // ~0.55 us whatever the mesh size (320 .. 81 920 faces), and the longest chain shrinks less than the fan-out grows)
                if (sp == 0) done = true;
                else next = stack[--sp][q];
            }
            NuBvhWideEntry e2 = e;
            if (!done) e2 = wide[next * 4LL + sub];
            // the leaf entries of THIS record
            int cf = 0, ci = NU_MISS_INDEX;
            float ct = 0.f;
            if (leaf) {
                float t;
                if (nu_ray_tri(o, d, tv, tv + 3, tv + 6, tmin, tmax, t)) { cf = 1; ct = t; ci = tid; }
            }
            merge(cf, ct, ci);
            if (done || (ANY_HIT && found)) break;
            e = e2;
        }
#ifdef NU_LBVH_STATS
        best_t = (float)steps; found = 1;                  // development build: t_out reports the number of records visited
#endif
    }
    if (sub == 0) src.end(found, best_id, best_t);
}

extern "C" int nu_lbvh_trace(const void* bvh, int n_faces, const float* rays, int N, float tmin, float tmax, float* hit,
                             int* idx, float* t_out, hipStream_t stream) {
    if (N <= 0) return NU_OK;
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    // four lanes per ray at every batch size: against the one-lane-per-ray kernel (since removed) 4 096 rays took 75 -> 39 us
    // object-aimed, 49 -> 32 us camera rays; 2^20 rays 1.82 -> 2.67 and 4.22 -> 4.96 G rays/s (profiles/r03/lbvh_bench.txt)
    const NuRayBuffer src = {rays, N, hit, idx, t_out, 0};
    hipLaunchKernelGGL((lbvh_trace_quad_kernel<NuRayBuffer, false>), dim3(nu_cdiv(N, 16)), dim3(64), 0, stream, (const char*)bvh, L, src,
                       tmin, tmax);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// object masks of real captures (utils/render_mask_real.py): one any-hit trace per pixel, rays made in registers
// ------------------------------------------------------------------------------------------------
extern "C" int nu_mask_pinhole_trace(const void* bvh, int n_faces, const float* cams, int n_img, int h, int w, unsigned char* out,
                                     hipStream_t stream) {
    if (n_img < 0 || h <= 0 || w <= 0 || n_faces <= 0 || !bvh || !cams || !out) return NU_ERR_ARG;
    if (n_img == 0) return NU_OK;
    const int tiles_x = nu_cdiv(w, 4), tiles_y = nu_cdiv(h, 4);
    const long long blocks = (long long)n_img * tiles_x * tiles_y;
    if (blocks > 0x7fffffffLL) return NU_ERR_ARG;         // the caller chunks over images
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    const NuPinholeMask src = {cams, h, w, tiles_x, tiles_x * tiles_y, out, 0};
    // tmin = 0, tmax = 1e16: the raygen program of cuda/triangle.cu
    hipLaunchKernelGGL((lbvh_trace_quad_kernel<NuPinholeMask, true>), dim3((unsigned)blocks), dim3(64), 0, stream, (const char*)bvh, L,
                       src, 0.0f, 1e16f);
    return nu_launch_status();
}

__global__ __launch_bounds__(256) void mask_pinhole_rays_kernel(const float* __restrict__ cams, int n_img, int h, int w,
                                                                float* __restrict__ rays) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long hw = (long long)h * w;
    if (p >= hw * n_img) return;
    const int img = (int)(p / hw);
    const int rem = (int)(p - img * hw), y = rem / w, x = rem - y * w;
    float o[3], d[3];
    nu_pinhole_ray(cams + (long long)img * NU_CAM_FLOATS, x, y, o, d);
    for (int k = 0; k < 3; ++k) { rays[p * 6 + k] = o[k]; rays[p * 6 + 3 + k] = d[k]; }
}
extern "C" int nu_mask_pinhole_rays(const float* cams, int n_img, int h, int w, float* rays, hipStream_t stream) {
    if (n_img < 0 || h <= 0 || w <= 0 || !cams || !rays) return NU_ERR_ARG;
    const long long N = (long long)n_img * h * w;
    if (N == 0) return NU_OK;
    if (nu_cdivl(N, 256) > 0x7fffffffLL) return NU_ERR_ARG;
    hipLaunchKernelGGL(mask_pinhole_rays_kernel, dim3((unsigned)nu_cdivl(N, 256)), dim3(256), 0, stream, cams, n_img, h, w, rays);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// relighting: the two traced passes.  Their ray sources instantiate the traversal template, so they live in this file;
// the sample sequence, the shadow ray and the shading are relight.h, the resolve pass and the debug entries relight.hip.
// ------------------------------------------------------------------------------------------------
struct NuRelightPrimary {                  // pixel centres of rows [y0, y0 + rows) of n images -> face id + G-buffer row: nu_relight_gbuffer
    const float* __restrict__ cams;        // [n, NU_CAM_FLOATS]
    int img0, h, w, y0, rows, tiles_x, tiles;
    const float* __restrict__ V;
    const int* __restrict__ F;
    const float* __restrict__ VN;          // [V,3] unit vertex normals
    const float* __restrict__ mat;         // [V,5] albedo, metallic, roughness
    int* __restrict__ face;                // [n, rows, w]
    float* __restrict__ gbuf;              // [n, rows, w, NU_RL_ROW]
    long long p;
    int img, pixel;
    float ro[3], rd[3];
    __device__ __forceinline__ bool begin(int blk, int q, float* o, float* d) {
        img = blk / tiles;
        const int t = blk - img * tiles;
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * 4 + (q & 3), yl = ty * 4 + (q >> 2);
        if (x >= w || yl >= rows) return false;
        p = ((long long)img * rows + yl) * w + x;
        pixel = (y0 + yl) * w + x;
        nu_pinhole_ray(cams + (long long)img * NU_CAM_FLOATS, x, y0 + yl, o, d);
        for (int k = 0; k < 3; ++k) { ro[k] = o[k]; rd[k] = d[k]; }
        return true;
    }
    __device__ __forceinline__ void end(int found, int id, float t) {
        float* g = gbuf + p * NU_RL_ROW;
        face[p] = found ? id : NU_RL_MISS;
        if (!found) {
            for (int k = 0; k < NU_RL_ROW; ++k) g[k] = 0.0f;
            return;
        }
        const int i0 = F[id * 3LL], i1 = F[id * 3LL + 1], i2 = F[id * 3LL + 2];
        float v0[3], e1[3], e2[3], pv[3], tv[3], qv[3], view[3];
        for (int k = 0; k < 3; ++k) {
            v0[k] = V[i0 * 3LL + k];
            e1[k] = V[i1 * 3LL + k] - v0[k];
            e2[k] = V[i2 * 3LL + k] - v0[k];
            view[k] = -rd[k];
        }
        // the barycentrics of the accepted hit: the operations of nu_ray_tri in its order
        nu_cross_rn(rd, e2, pv);
        const float inv = 1.0f / nu_dot3_rn(e1, pv);
        for (int k = 0; k < 3; ++k) tv[k] = ro[k] - v0[k];
        const float u = nu_dot3_rn(tv, pv) * inv;
        nu_cross_rn(tv, e1, qv);
        const float v = nu_dot3_rn(rd, qv) * inv;
        const float w0 = (1.0f - u) - v;
        float ng[3], ns[3];
        nu_cross_rn(e1, e2, ng);
        float len = sqrtf(nu_dot3_rn(ng, ng));
        if (len > 0.0f) { for (int k = 0; k < 3; ++k) ng[k] = ng[k] / len; }
        else { for (int k = 0; k < 3; ++k) ng[k] = view[k]; }
        if (nu_dot3_rn(ng, view) < 0.0f) { for (int k = 0; k < 3; ++k) ng[k] = -ng[k]; }
        for (int k = 0; k < 3; ++k) ns[k] = (w0 * VN[i0 * 3LL + k] + u * VN[i1 * 3LL + k]) + v * VN[i2 * 3LL + k];
        len = sqrtf(nu_dot3_rn(ns, ns));
        if (len > 0.0f && len < 1e30f) { for (int k = 0; k < 3; ++k) ns[k] = ns[k] / len; }      // false for NaN normals too
        else { for (int k = 0; k < 3; ++k) ns[k] = ng[k]; }
        if (nu_dot3_rn(ns, ng) < 0.0f) { for (int k = 0; k < 3; ++k) ns[k] = -ns[k]; }
        g[0] = t;
        for (int k = 0; k < 3; ++k) {
            g[1 + k] = ro[k] + t * rd[k];
            g[4 + k] = ng[k];
            g[7 + k] = ns[k];
            g[15 + k] = view[k];
        }
        for (int k = 0; k < 5; ++k) g[10 + k] = (w0 * mat[i0 * 5LL + k] + u * mat[i1 * 5LL + k]) + v * mat[i2 * 5LL + k];
        g[18] = __int_as_float(img0 + img);
        g[19] = __int_as_float(pixel);
    }
};

extern "C" int nu_relight_gbuffer(const void* bvh, int n_faces, const float* V, const int* F, const float* vnormals, const float* materials,
                                  const float* cams, int n_img, int img0, int h, int w, int y0, int rows, int* face, float* gbuf,
                                  hipStream_t stream) {
    if (n_img < 0 || h <= 0 || w <= 0 || n_faces <= 0 || y0 < 0 || rows < 0 || y0 + rows > h || img0 < 0) return NU_ERR_ARG;
    if (!bvh || !V || !F || !vnormals || !materials || !cams || !face || !gbuf) return NU_ERR_ARG;
    if (n_img == 0 || rows == 0) return NU_OK;
    const int tiles_x = nu_cdiv(w, 4), tiles_y = nu_cdiv(rows, 4);
    const long long blocks = (long long)n_img * tiles_x * tiles_y;
    if (blocks > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL) return NU_ERR_ARG;       // the caller chunks over images / rows
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    NuRelightPrimary src = {};
    src.cams = cams; src.img0 = img0; src.h = h; src.w = w; src.y0 = y0; src.rows = rows; src.tiles_x = tiles_x; src.tiles = tiles_x * tiles_y;
    src.V = V; src.F = F; src.VN = vnormals; src.mat = materials; src.face = face; src.gbuf = gbuf;
    hipLaunchKernelGGL((lbvh_trace_quad_kernel<NuRelightPrimary, false>), dim3((unsigned)blocks), dim3(64), 0, stream, (const char*)bvh, L,
                       src, 0.0f, 1e16f);
    return nu_launch_status();
}

struct NuRelightShadow {                   // samples [s0, s0 + s_count) of the listed pixels -> one byte each (1 = lit): nu_relight_visibility
    const float* __restrict__ gbuf;
    const int* __restrict__ pix;           // [n_pix] G-buffer rows of hit pixels
    int S, s0, s_count, bpp;               // bpp = 16-sample blocks per pixel
    unsigned seed;
    float eps;
    unsigned char* __restrict__ vis;       // [n_pix, s_count]
    long long slot;
    __device__ __forceinline__ bool begin(int blk, int q, float* o, float* d) {
        const int i = blk / bpp;
        const int c = (blk - i * bpp) * 16 + q;
        if (c >= s_count) return false;
        slot = (long long)i * s_count + c;
        unsigned bits[2];
        if (!nu_relight_shadow_ray(gbuf + (long long)pix[i] * NU_RL_ROW, S, s0 + c, seed, eps, o, d, bits)) {
            if ((threadIdx.x & 3) == 0) vis[slot] = 0;         // below a horizon: not traced, dark
            return false;
        }
        return true;
    }
    __device__ __forceinline__ void end(int found, int, float) { vis[slot] = found ? 0 : 1; }
};

extern "C" int nu_relight_visibility(const void* bvh, int n_faces, const float* gbuf, const int* pix, int n_pix, int samples, int s0,
                                     int s_count, int seed, float eps, unsigned char* vis, hipStream_t stream) {
    if (n_pix < 0 || n_faces <= 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples) return NU_ERR_ARG;
    if (!bvh || !gbuf || !pix || !vis) return NU_ERR_ARG;
    if (n_pix == 0 || s_count == 0) return NU_OK;
    const int bpp = nu_cdiv(s_count, 16);
    const long long blocks = (long long)n_pix * bpp;
    if (blocks > 0x7fffffffLL) return NU_ERR_ARG;         // the caller chunks over pixels / samples
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    NuRelightShadow src = {gbuf, pix, samples, s0, s_count, bpp, (unsigned)seed, eps, vis, 0};
    // tmin = 0, tmax = 1e16 as every trace of this file; any hit: `found` is the closest-hit predicate (see the kernel)
    hipLaunchKernelGGL((lbvh_trace_quad_kernel<NuRelightShadow, true>), dim3((unsigned)blocks), dim3(64), 0, stream, (const char*)bvh, L,
                       src, 0.0f, 1e16f);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// relighting of the nested object: several DEPENDENT walks per quad, through two trees, in one launch.
//
// nu_walk_quad is the walk of lbvh_trace_quad_kernel written a second time as a device function (that kernel is left as it is: its
// instantiations keep their register figures and their bits): the same records, the same box and triangle tests in the same order,
// the same ordering inside the quad, the same stack discipline -- so (found, face id, t) of a closest-hit walk and `found` of an
// any-hit walk are those of nu_lbvh_trace on the same ray, bit for bit.  any_hit is a run-time flag here, and the walk may be
// called again and again by a quad: the stack column of the quad is empty whenever a walk ends (an any-hit walk that leaves early
// simply starts the next one at sp = 0).  The kernels below call it from ONE site inside a per-quad state machine, so the quads of a
// wave that are at different steps of their paths still share the loop.
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ void nu_walk_quad(int (*stack)[16], int q, int sub, const char* __restrict__ buf, const NuBvhLayout L,
                                                    const float* o, const float* d, float tmin, float tmax, bool any_hit, int& found,
                                                    int& best_id, float& best_t) {
    const NuBvhHeader* h = (const NuBvhHeader*)(buf + L.header);
    const NuBvhWideEntry* wide = (const NuBvhWideEntry*)(buf + L.wide);
    const float* tris = (const float*)(buf + L.tris);
    const int* ids = (const int*)(buf + L.ids);
    const int n = h->n_faces;
    float invd[3];
    for (int k = 0; k < 3; ++k) invd[k] = 1.0f / d[k];
    best_t = tmax;
    best_id = NU_MISS_INDEX;
    found = 0;
    auto merge = [&](int cf, float ct, int ci) {
#define NU_BETTER(f2, t2, i2) ((f2) && (!cf || (t2) < ct || ((t2) == ct && (i2) < ci)))
        { const int f2 = nu_quad_i<NU_QP_XOR1>(cf); const float t2 = nu_quad_f<NU_QP_XOR1>(ct); const int i2 = nu_quad_i<NU_QP_XOR1>(ci);
          if (NU_BETTER(f2, t2, i2)) { cf = 1; ct = t2; ci = i2; } }
        { const int f2 = nu_quad_i<NU_QP_XOR2>(cf); const float t2 = nu_quad_f<NU_QP_XOR2>(ct); const int i2 = nu_quad_i<NU_QP_XOR2>(ci);
          if (NU_BETTER(f2, t2, i2)) { cf = 1; ct = t2; ci = i2; } }
#undef NU_BETTER
        if (cf && (!found || ct < best_t || (ct == best_t && ci < best_id))) { best_t = ct; best_id = ci; found = 1; }
    };
    if (n == 1) {
        int cf = 0, ci = NU_MISS_INDEX;
        float ct = 0.f, t;
        if (sub == 0 && nu_ray_tri(o, d, tris, tris + 4, tris + 8, tmin, tmax, t)) { cf = 1; ct = t; ci = ids[0]; }
        merge(cf, ct, ci);
        return;
    }
    int sp = 0;
    NuBvhWideEntry e = wide[sub];
    while (true) {
        float tn;
        const bool hb = e.ref != NU_WIDE_EMPTY && nu_ray_box(o, invd, e.bmin, e.bmax, tmin, any_hit ? tmax : best_t, tn);
        const bool leaf = hb && e.ref < 0;
        const int pos = leaf ? -1 - e.ref : 0;
        float tv[9];
        int tid = NU_MISS_INDEX;
        if (leaf) {
#pragma unroll
            for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int k = 0; k < 3; ++k) tv[v * 3 + k] = tris[pos * 12LL + v * 4 + k];
            tid = ids[pos];
        }
        const int want = (hb && e.ref >= 0) ? 1 : 0;
        int rank = 0, cnt = want;
        { const int w2 = nu_quad_i<NU_QP_XOR1>(want); const float t2 = nu_quad_f<NU_QP_XOR1>(tn); const int s2 = sub ^ 1;
          cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
        { const int w2 = nu_quad_i<NU_QP_XOR2>(want); const float t2 = nu_quad_f<NU_QP_XOR2>(tn); const int s2 = sub ^ 2;
          cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
        { const int w2 = nu_quad_i<NU_QP_XOR3>(want); const float t2 = nu_quad_f<NU_QP_XOR3>(tn); const int s2 = sub ^ 3;
          cnt += w2; rank += (w2 && (t2 < tn || (t2 == tn && s2 < sub))) ? 1 : 0; }
        int next = (want && rank == 0) ? e.ref : -1;
        next = max(next, nu_quad_i<NU_QP_XOR1>(next));
        next = max(next, nu_quad_i<NU_QP_XOR2>(next));
        if (want && rank > 0) stack[sp + (cnt - 1 - rank)][q] = e.ref;
        sp += cnt > 0 ? cnt - 1 : 0;
        bool done = false;
        if (cnt == 0) {
            if (sp == 0) done = true;
            else next = stack[--sp][q];
        }
        NuBvhWideEntry e2 = e;
        if (!done) e2 = wide[next * 4LL + sub];
        int cf = 0, ci = NU_MISS_INDEX;
        float ct = 0.f;
        if (leaf) {
            float t;
            if (nu_ray_tri(o, d, tv, tv + 3, tv + 6, tmin, tmax, t)) { cf = 1; ct = t; ci = tid; }
        }
        merge(cf, ct, ci);
        if (done || (any_hit && found)) break;
        e = e2;
    }
}

// The two meshes of a nested scene: as the entries take them, and as the kernels see them.
#define NU_NESTED_ARGS const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior, \
                       const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i
struct NuNestedMeshes {
    const char* __restrict__ bvh_o;        // outer shell: tree, vertices, faces, unit vertex normals, index of refraction per vertex
    NuBvhLayout Lo;
    const float* __restrict__ Vo;
    const int* __restrict__ Fo;
    const float* __restrict__ VNo;
    const float* __restrict__ ior;
    const char* __restrict__ bvh_i;        // inner object: tree, vertices, faces, unit vertex normals, materials [V,5]
    NuBvhLayout Li;
    const float* __restrict__ Vi;
    const int* __restrict__ Fi;
    const float* __restrict__ VNi;
    const float* __restrict__ mat;
};

// Interior chain of the listed hit pixels of the OUTER G-buffer (whose rows carry the interpolated index of refraction - 1 in [10]):
// one quad per pixel, 16 consecutive listed pixels per wave, every walk of a pixel's path in this one launch, state in registers.
// Steps of a path: the reflection ray (any hit, outer), then per segment the closest hit against the inner and against the outer
// tree, then the exit ray (any hit, outer).  DUMP writes every traced ray and what it met (tests).
#define NU_RLN_PH_REFL 0
#define NU_RLN_PH_INNER 1
#define NU_RLN_PH_OUTER 2
#define NU_RLN_PH_EXIT 3
#define NU_RLN_PH_DONE 4
template <bool DUMP>
__global__ __launch_bounds__(64) void relight_nested_chain_kernel(NuNestedMeshes m, const float* __restrict__ gbuf, const int* __restrict__ pix,
                                                                  int n_pix, float eps, int K, int* __restrict__ kind,
                                                                  float* __restrict__ chain, float* __restrict__ irow,
                                                                  float* __restrict__ seg, float* __restrict__ aux) {
    __shared__ int stack[NU_WSTACK][16];
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    const int i = blockIdx.x * 16 + q;
    if (i >= n_pix) return;                                 // whole quads leave together
    const float* g = gbuf + (long long)pix[i] * NU_RL_ROW;
    float d0[3], x0[3], ng0[3], n[3], cur_o[3], cur_d[3], rdir[3];
    for (int k = 0; k < 3; ++k) { d0[k] = -g[15 + k]; x0[k] = g[1 + k]; ng0[k] = g[4 + k]; }
    float f_entry;
    const bool enters = nu_rln_interface(d0, g + 7, 1.0f + g[10], true, n, cur_d, f_entry);
    if (enters) nu_rln_reflect(d0, n, rdir);
    else { for (int k = 0; k < 3; ++k) rdir[k] = cur_d[k]; }
    const bool refl_traced = f_entry > 0.0f && nu_rl_dot3(n, rdir) > 0.0f && nu_rl_dot3(ng0, rdir) > 0.0f;
    for (int k = 0; k < 3; ++k) cur_o[k] = x0[k] - eps * ng0[k];
    float T = enters ? 1.0f - f_entry : 0.0f;
    float refl_vis = 0.0f, exit_vis = 0.0f;
    float exit_o[3] = {0.f, 0.f, 0.f}, exit_d[3] = {0.f, 0.f, 0.f};
    int what = NU_RLN_DARK, k_seg = 0, n_walked = 0;
    int in_found = 0, in_id = NU_MISS_INDEX;
    float in_t = 0.0f;
    int phase = refl_traced ? NU_RLN_PH_REFL : (enters ? NU_RLN_PH_INNER : NU_RLN_PH_DONE);
    if (DUMP && sub == 0) {
        float* a = aux + (long long)i * 16;
        for (int k = 0; k < 3; ++k) { a[k] = x0[k] + eps * ng0[k]; a[3 + k] = rdir[k]; }
        a[6] = refl_traced ? 1.0f : 0.0f; a[7] = 0.0f;
        for (int k = 8; k < 16; ++k) a[k] = 0.0f;
        for (int k = 0; k < K * 16; ++k) seg[(long long)i * K * 16 + k] = 0.0f;
    }
    while (phase != NU_RLN_PH_DONE) {
        float o[3], d[3];
        const bool outer = phase != NU_RLN_PH_INNER;
        const bool any_hit = phase == NU_RLN_PH_REFL || phase == NU_RLN_PH_EXIT;
        for (int k = 0; k < 3; ++k) {
            o[k] = phase == NU_RLN_PH_REFL ? x0[k] + eps * ng0[k] : (phase == NU_RLN_PH_EXIT ? exit_o[k] : cur_o[k]);
            d[k] = phase == NU_RLN_PH_REFL ? rdir[k] : (phase == NU_RLN_PH_EXIT ? exit_d[k] : cur_d[k]);
        }
        int found, id;
        float t;
        nu_walk_quad(stack, q, sub, outer ? m.bvh_o : m.bvh_i, outer ? m.Lo : m.Li, o, d, 0.0f, 1e16f, any_hit, found, id, t);
        if (phase == NU_RLN_PH_REFL) {
            refl_vis = found ? 0.0f : 1.0f;
            if (DUMP && sub == 0) aux[(long long)i * 16 + 7] = found ? 1.0f : 0.0f;
            phase = enters ? NU_RLN_PH_INNER : NU_RLN_PH_DONE;
        } else if (phase == NU_RLN_PH_INNER) {
            in_found = found; in_id = id; in_t = t;
            phase = NU_RLN_PH_OUTER;
        } else if (phase == NU_RLN_PH_OUTER) {
            const bool ends_inner = in_found && (!found || in_t <= t);
            ++n_walked;
            float* sg = DUMP ? seg + ((long long)i * K + k_seg) * 16 : nullptr;
            if (DUMP && sub == 0) {
                for (int k = 0; k < 3; ++k) { sg[k] = cur_o[k]; sg[3 + k] = cur_d[k]; }
                sg[6] = __int_as_float(ends_inner ? 1 : (found ? 2 : 0));
                sg[7] = __int_as_float(ends_inner ? in_id : id);
                sg[8] = ends_inner ? in_t : (found ? t : 0.0f);
                sg[9] = __int_as_float(in_found); sg[10] = __int_as_float(in_id); sg[11] = in_found ? in_t : 0.0f;
                sg[12] = __int_as_float(found); sg[13] = __int_as_float(id); sg[14] = found ? t : 0.0f;
                sg[15] = __int_as_float(1);                                     // the segment was walked
            }
            if (ends_inner) {
                float x[3], ng[3], ns[3], bary[3];
                int vi[3];
                nu_rl_surface(m.Vi, m.Fi, m.VNi, cur_o, cur_d, in_id, in_t, x, ng, ns, vi, bary);
                if (sub == 0) {
                    float* r = irow + (long long)i * NU_RL_ROW;
                    r[0] = in_t;
                    for (int k = 0; k < 3; ++k) { r[1 + k] = x[k]; r[4 + k] = ng[k]; r[7 + k] = ns[k]; r[15 + k] = -cur_d[k]; }
                    for (int k = 0; k < 5; ++k)
                        r[10 + k] = (bary[0] * m.mat[vi[0] * 5LL + k] + bary[1] * m.mat[vi[1] * 5LL + k]) + bary[2] * m.mat[vi[2] * 5LL + k];
                    r[18] = g[18]; r[19] = g[19];
                }
                what = NU_RLN_INNER;
                phase = NU_RLN_PH_DONE;
            } else if (found) {
                float keep, o2[3], d2[3];
                const bool refr = nu_rln_leave(m.Vo, m.Fo, m.VNo, m.ior, cur_o, cur_d, id, t, eps, o2, d2, keep);
                if (refr) {
                    T = T * keep;
                    for (int k = 0; k < 3; ++k) { exit_o[k] = o2[k]; exit_d[k] = d2[k]; }
                    phase = NU_RLN_PH_EXIT;
                } else {
                    for (int k = 0; k < 3; ++k) { cur_o[k] = o2[k]; cur_d[k] = d2[k]; }     // total internal reflection: on, from eps inside
                    ++k_seg;
                    phase = k_seg < K ? NU_RLN_PH_INNER : NU_RLN_PH_DONE;
                    if (k_seg >= K) T = 0.0f;
                }
            } else {                                        // a leaky shell: the ray leaves as it is, and nothing can shadow it
                for (int k = 0; k < 3; ++k) { exit_o[k] = cur_o[k]; exit_d[k] = cur_d[k]; }
                exit_vis = 1.0f;
                what = NU_RLN_EXIT;
                phase = NU_RLN_PH_DONE;
            }
        } else {
            exit_vis = found ? 0.0f : 1.0f;
            if (DUMP && sub == 0) {
                float* a = aux + (long long)i * 16 + 8;
                for (int k = 0; k < 3; ++k) { a[k] = exit_o[k]; a[3 + k] = exit_d[k]; }
                a[6] = 1.0f; a[7] = found ? 1.0f : 0.0f;
            }
            what = NU_RLN_EXIT;
            phase = NU_RLN_PH_DONE;
        }
    }
    if (sub == 0) {
        kind[i] = what;
        float* c = chain + (long long)i * NU_RLN_CHAIN;
        c[0] = what == NU_RLN_DARK ? 0.0f : T;
        for (int k = 0; k < 3; ++k) { c[1 + k] = exit_d[k]; c[5 + k] = rdir[k]; }
        c[4] = exit_vis; c[8] = f_entry; c[9] = refl_vis;
        c[10] = __int_as_float(n_walked); c[11] = 0.0f;
        if (what != NU_RLN_INNER) { for (int k = 0; k < NU_RL_ROW; ++k) irow[(long long)i * NU_RL_ROW + k] = 0.0f; }
    }
}

// Light paths of the listed inner rows: blocks of 16 quads = 16 consecutive samples of one pixel (as NuRelightShadow), the three walks
// of a sample back to back on the one stack, no ray stored: (a) any hit against the inner tree, (b) closest hit against the outer
// tree along the same ray, the interface event going out, (c) any hit against the outer tree along the exit ray.  Per sample one
// 16-byte record: (exit direction, 1 - F_exit), or zero for a dark sample; nu_relight_nested_resolve taps the environment.
template <bool DUMP>
__global__ __launch_bounds__(64) void relight_nested_light_kernel(NuNestedMeshes m, const float* __restrict__ irow, const int* __restrict__ sel,
                                                                  int S, int s0, int s_count, int bpp, unsigned seed, float eps,
                                                                  float4* __restrict__ rec, float* __restrict__ dump) {
    __shared__ int stack[NU_WSTACK][16];
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    const int i = blockIdx.x / bpp;
    const int c = (blockIdx.x - i * bpp) * 16 + q;
    if (c >= s_count) return;                               // whole quads leave together
    const long long slot = (long long)i * s_count + c;
    float o[3], d[3];
    unsigned bits[2];
    const bool traced = nu_relight_shadow_ray(irow + (long long)sel[i] * NU_RL_ROW, S, s0 + c, seed, eps, o, d, bits);
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float keep = 1.0f;
    float* dp = DUMP ? dump + slot * NU_RLN_LIGHT_DUMP : nullptr;
    if (DUMP && sub == 0) {
        for (int k = 0; k < NU_RLN_LIGHT_DUMP; ++k) dp[k] = 0.0f;
        for (int k = 0; k < 3; ++k) { dp[k] = o[k]; dp[3 + k] = d[k]; }
        dp[6] = traced ? 1.0f : 0.0f;
    }
    int phase = traced ? 0 : 3;
    while (phase != 3) {
        int found, id;
        float t;
        nu_walk_quad(stack, q, sub, phase == 0 ? m.bvh_i : m.bvh_o, phase == 0 ? m.Li : m.Lo, o, d, 0.0f, 1e16f, phase != 1, found, id, t);
        if (phase == 0) {
            if (DUMP && sub == 0) dp[7] = found ? 1.0f : 0.0f;
            phase = found ? 3 : 1;
        } else if (phase == 1) {
            if (DUMP && sub == 0) { dp[8] = found ? 1.0f : 0.0f; dp[9] = __int_as_float(id); dp[10] = found ? t : 0.0f; }
            if (!found) {                                   // a leaky shell: the direction leaves unrefracted
                out = make_float4(d[0], d[1], d[2], 1.0f);
                phase = 3;
            } else {
                float o2[3], d2[3];
                const bool refr = nu_rln_leave(m.Vo, m.Fo, m.VNo, m.ior, o, d, id, t, eps, o2, d2, keep);
                if (DUMP && sub == 0) {
                    dp[11] = refr ? 1.0f : 0.0f;
                    for (int k = 0; k < 3; ++k) { dp[12 + k] = o2[k]; dp[15 + k] = d2[k]; }
                    dp[19] = keep;
                }
                for (int k = 0; k < 3; ++k) { o[k] = o2[k]; d[k] = d2[k]; }
                phase = refr ? 2 : 3;
            }
        } else {
            if (DUMP && sub == 0) dp[18] = found ? 1.0f : 0.0f;
            if (!found) out = make_float4(d[0], d[1], d[2], keep);
            phase = 3;
        }
    }
    if (sub == 0) rec[slot] = out;
}

static int nu_nested_meshes(NU_NESTED_ARGS, NuNestedMeshes& m) {
    if (n_faces_o <= 0 || n_faces_i <= 0) return NU_ERR_ARG;
    if (!bvh_o || !V_o || !F_o || !vnormals_o || !ior || !bvh_i || !V_i || !F_i || !vnormals_i || !materials_i) return NU_ERR_ARG;
    m.bvh_o = (const char*)bvh_o; m.Lo = nu_bvh_layout(n_faces_o); m.Vo = V_o; m.Fo = F_o; m.VNo = vnormals_o; m.ior = ior;
    m.bvh_i = (const char*)bvh_i; m.Li = nu_bvh_layout(n_faces_i); m.Vi = V_i; m.Fi = F_i; m.VNi = vnormals_i; m.mat = materials_i;
    return NU_OK;
}
#define NU_NESTED_PASS bvh_o, n_faces_o, V_o, F_o, vnormals_o, ior, bvh_i, n_faces_i, V_i, F_i, vnormals_i, materials_i

static int nu_nested_chain_launch(NU_NESTED_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int max_segments, int* kind,
                                  float* chain, float* inner_rows, float* seg, float* aux, bool dump, hipStream_t stream) {
    NuNestedMeshes m;
    if (n_pix < 0 || max_segments < 1 || max_segments > 64 || nu_nested_meshes(NU_NESTED_PASS, m) != NU_OK) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    if (!gbuf || !pix || !kind || !chain || !inner_rows || (dump && (!seg || !aux))) return NU_ERR_ARG;
    const dim3 grid(nu_cdiv(n_pix, 16));
    if (dump)
        hipLaunchKernelGGL((relight_nested_chain_kernel<true>), grid, dim3(64), 0, stream, m, gbuf, pix, n_pix, eps, max_segments, kind,
                           chain, inner_rows, seg, aux);
    else
        hipLaunchKernelGGL((relight_nested_chain_kernel<false>), grid, dim3(64), 0, stream, m, gbuf, pix, n_pix, eps, max_segments, kind,
                           chain, inner_rows, seg, aux);
    return nu_launch_status();
}
extern "C" int nu_relight_nested_chain(NU_NESTED_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int max_segments, int* kind,
                                       float* chain, float* inner_rows, hipStream_t stream) {
    return nu_nested_chain_launch(NU_NESTED_PASS, gbuf, pix, n_pix, eps, max_segments, kind, chain, inner_rows, nullptr, nullptr, false, stream);
}
extern "C" int nu_relight_nested_chain_dump(NU_NESTED_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int max_segments,
                                            int* kind, float* chain, float* inner_rows, float* seg, float* aux, hipStream_t stream) {
    return nu_nested_chain_launch(NU_NESTED_PASS, gbuf, pix, n_pix, eps, max_segments, kind, chain, inner_rows, seg, aux, true, stream);
}

static int nu_nested_light_launch(NU_NESTED_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                  int seed, float eps, float* rec, float* dump, bool dumping, hipStream_t stream) {
    NuNestedMeshes m;
    if (n_sel < 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples) return NU_ERR_ARG;
    if (nu_nested_meshes(NU_NESTED_PASS, m) != NU_OK) return NU_ERR_ARG;
    if (n_sel == 0 || s_count == 0) return NU_OK;
    if (!inner_rows || !sel || !rec || (dumping && !dump)) return NU_ERR_ARG;
    const int bpp = nu_cdiv(s_count, 16);
    const long long blocks = (long long)n_sel * bpp;
    if (blocks > 0x7fffffffLL) return NU_ERR_ARG;         // the caller chunks over pixels / samples
    if (dumping)
        hipLaunchKernelGGL((relight_nested_light_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, stream, m, inner_rows, sel, samples, s0,
                           s_count, bpp, (unsigned)seed, eps, (float4*)rec, dump);
    else
        hipLaunchKernelGGL((relight_nested_light_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, stream, m, inner_rows, sel, samples, s0,
                           s_count, bpp, (unsigned)seed, eps, (float4*)rec, dump);
    return nu_launch_status();
}
extern "C" int nu_relight_nested_light(NU_NESTED_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                       int seed, float eps, float* rec, hipStream_t stream) {
    return nu_nested_light_launch(NU_NESTED_PASS, inner_rows, sel, n_sel, samples, s0, s_count, seed, eps, rec, nullptr, false, stream);
}
extern "C" int nu_relight_nested_light_dump(NU_NESTED_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0,
                                            int s_count, int seed, float eps, float* rec, float* dump, hipStream_t stream) {
    return nu_nested_light_launch(NU_NESTED_PASS, inner_rows, sel, n_sel, samples, s0, s_count, seed, eps, rec, dump, true, stream);
}

// ------------------------------------------------------------------------------------------------
// relighting through the THIN shell: the nested kernels above with the wall crossing of the non-zero-thickness model
// (nu_rlt_cross) in place of the single interface.  New kernels -- the ones above keep their registers and their bits -- of the same
// build: one quad per pixel / sample, every walk from ONE call site of nu_walk_quad, the same stack.  A camera path has one cavity
// segment: a crossing that fails (total reflection at any face) ends it dark.
// ------------------------------------------------------------------------------------------------
struct NuThinMeshes {
    NuNestedMeshes m;
    const float* __restrict__ thick;       // wall thickness per vertex of the outer mesh
    const float* __restrict__ curv;        // Gaussian curvature per vertex of the outer mesh
};

// Outer G-buffer rows carry index - 1, thickness and curvature in [10], [11], [12].  Steps: the reflection ray (any hit, outer), the
// cavity segment (closest hit, inner then outer), the exit ray (any hit, outer).  Records as relight_nested_chain_kernel writes them.
template <bool DUMP>
__global__ __launch_bounds__(64) void relight_thin_chain_kernel(NuThinMeshes tm, const float* __restrict__ gbuf, const int* __restrict__ pix,
                                                                int n_pix, float eps, int* __restrict__ kind, float* __restrict__ chain,
                                                                float* __restrict__ irow, float* __restrict__ seg, float* __restrict__ aux) {
    __shared__ int stack[NU_WSTACK][16];
    const NuNestedMeshes& m = tm.m;
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    const int i = blockIdx.x * 16 + q;
    if (i >= n_pix) return;                                 // whole quads leave together
    const float* g = gbuf + (long long)pix[i] * NU_RL_ROW;
    float d0[3], x0[3], ng0[3], n[3], pend[3], cur_o[3], cur_d[3], rdir[3];
    for (int k = 0; k < 3; ++k) { d0[k] = -g[15 + k]; x0[k] = g[1 + k]; ng0[k] = g[4 + k]; }
    float f_entry, f_b;
    bool refr, ok;
    nu_rlt_cross(d0, x0, g + 7, 1.0f + g[10], g[11], g[12], false, refr, ok, n, pend, cur_o, cur_d, f_entry, f_b);
    const bool enters = refr && ok;
    nu_rln_reflect(d0, n, rdir);
    const bool refl_traced = f_entry > 0.0f && nu_rl_dot3(n, rdir) > 0.0f && nu_rl_dot3(ng0, rdir) > 0.0f;
    float T = enters ? (1.0f - f_entry) * (1.0f - f_b) : 0.0f;
    float refl_vis = 0.0f, exit_vis = 0.0f;
    float exit_o[3] = {0.f, 0.f, 0.f}, exit_d[3] = {0.f, 0.f, 0.f};
    int what = NU_RLN_DARK, n_walked = 0;
    int in_found = 0, in_id = NU_MISS_INDEX;
    float in_t = 0.0f;
    int phase = refl_traced ? NU_RLN_PH_REFL : (enters ? NU_RLN_PH_INNER : NU_RLN_PH_DONE);
    if (DUMP && sub == 0) {
        float* a = aux + (long long)i * 16;
        for (int k = 0; k < 3; ++k) { a[k] = x0[k] + eps * ng0[k]; a[3 + k] = rdir[k]; }
        a[6] = refl_traced ? 1.0f : 0.0f; a[7] = 0.0f;
        for (int k = 8; k < 16; ++k) a[k] = 0.0f;
        for (int k = 0; k < 16; ++k) seg[(long long)i * 16 + k] = 0.0f;
    }
    while (phase != NU_RLN_PH_DONE) {
        float o[3], d[3];
        const bool outer = phase != NU_RLN_PH_INNER;
        const bool any_hit = phase == NU_RLN_PH_REFL || phase == NU_RLN_PH_EXIT;
        for (int k = 0; k < 3; ++k) {
            o[k] = phase == NU_RLN_PH_REFL ? x0[k] + eps * ng0[k] : (phase == NU_RLN_PH_EXIT ? exit_o[k] : cur_o[k]);
            d[k] = phase == NU_RLN_PH_REFL ? rdir[k] : (phase == NU_RLN_PH_EXIT ? exit_d[k] : cur_d[k]);
        }
        int found, id;
        float t;
        nu_walk_quad(stack, q, sub, outer ? m.bvh_o : m.bvh_i, outer ? m.Lo : m.Li, o, d, 0.0f, 1e16f, any_hit, found, id, t);
        if (phase == NU_RLN_PH_REFL) {
            refl_vis = found ? 0.0f : 1.0f;
            if (DUMP && sub == 0) aux[(long long)i * 16 + 7] = found ? 1.0f : 0.0f;
            phase = enters ? NU_RLN_PH_INNER : NU_RLN_PH_DONE;
        } else if (phase == NU_RLN_PH_INNER) {
            in_found = found; in_id = id; in_t = t;
            phase = NU_RLN_PH_OUTER;
        } else if (phase == NU_RLN_PH_OUTER) {
            const bool ends_inner = in_found && (!found || in_t <= t);
            n_walked = 1;
            if (DUMP && sub == 0) {
                float* sg = seg + (long long)i * 16;
                for (int k = 0; k < 3; ++k) { sg[k] = cur_o[k]; sg[3 + k] = cur_d[k]; }
                sg[6] = __int_as_float(ends_inner ? 1 : (found ? 2 : 0));
                sg[7] = __int_as_float(ends_inner ? in_id : id);
                sg[8] = ends_inner ? in_t : (found ? t : 0.0f);
                sg[9] = __int_as_float(in_found); sg[10] = __int_as_float(in_id); sg[11] = in_found ? in_t : 0.0f;
                sg[12] = __int_as_float(found); sg[13] = __int_as_float(id); sg[14] = found ? t : 0.0f;
                sg[15] = __int_as_float(1);                                     // the segment was walked
            }
            if (ends_inner) {
                float x[3], ng[3], ns[3], bary[3];
                int vi[3];
                nu_rl_surface(m.Vi, m.Fi, m.VNi, cur_o, cur_d, in_id, in_t, x, ng, ns, vi, bary);
                if (sub == 0) {
                    float* r = irow + (long long)i * NU_RL_ROW;
                    r[0] = in_t;
                    for (int k = 0; k < 3; ++k) { r[1 + k] = x[k]; r[4 + k] = ng[k]; r[7 + k] = ns[k]; r[15 + k] = -cur_d[k]; }
                    for (int k = 0; k < 5; ++k)
                        r[10 + k] = (bary[0] * m.mat[vi[0] * 5LL + k] + bary[1] * m.mat[vi[1] * 5LL + k]) + bary[2] * m.mat[vi[2] * 5LL + k];
                    r[18] = g[18]; r[19] = g[19];
                }
                what = NU_RLN_INNER;
                phase = NU_RLN_PH_DONE;
            } else if (found) {
                float keep;
                const bool out = nu_rlt_leave(m.Vo, m.Fo, m.VNo, m.ior, tm.thick, tm.curv, cur_o, cur_d, id, t, eps, exit_o, exit_d, keep);
                T = out ? T * keep : 0.0f;
                phase = out ? NU_RLN_PH_EXIT : NU_RLN_PH_DONE;     // a crossing that fails ends the path dark
            } else {                                        // a leaky shell: the ray leaves as it is, and nothing can shadow it
                for (int k = 0; k < 3; ++k) { exit_o[k] = cur_o[k]; exit_d[k] = cur_d[k]; }
                exit_vis = 1.0f;
                what = NU_RLN_EXIT;
                phase = NU_RLN_PH_DONE;
            }
        } else {
            exit_vis = found ? 0.0f : 1.0f;
            if (DUMP && sub == 0) {
                float* a = aux + (long long)i * 16 + 8;
                for (int k = 0; k < 3; ++k) { a[k] = exit_o[k]; a[3 + k] = exit_d[k]; }
                a[6] = 1.0f; a[7] = found ? 1.0f : 0.0f;
            }
            what = NU_RLN_EXIT;
            phase = NU_RLN_PH_DONE;
        }
    }
    if (sub == 0) {
        kind[i] = what;
        float* c = chain + (long long)i * NU_RLN_CHAIN;
        c[0] = what == NU_RLN_DARK ? 0.0f : T;
        for (int k = 0; k < 3; ++k) { c[1 + k] = what == NU_RLN_EXIT ? exit_d[k] : 0.0f; c[5 + k] = rdir[k]; }
        c[4] = exit_vis; c[8] = f_entry; c[9] = refl_vis;
        c[10] = __int_as_float(n_walked); c[11] = 0.0f;
        if (what != NU_RLN_INNER) { for (int k = 0; k < NU_RL_ROW; ++k) irow[(long long)i * NU_RL_ROW + k] = 0.0f; }
    }
}

// Light paths of the listed inner rows, as relight_nested_light_kernel: (a) any hit against the inner tree, (b) closest hit against the
// outer tree along the same ray and the leaving crossing, (c) any hit against the outer tree along the ray behind the wall.  Per
// sample one 16-byte record (exit direction, keep = (1 - F_a)(1 - F_b)), or zero for a dark sample.
template <bool DUMP>
__global__ __launch_bounds__(64) void relight_thin_light_kernel(NuThinMeshes tm, const float* __restrict__ irow, const int* __restrict__ sel,
                                                                int S, int s0, int s_count, int bpp, unsigned seed, float eps,
                                                                float4* __restrict__ rec, float* __restrict__ dump) {
    __shared__ int stack[NU_WSTACK][16];
    const NuNestedMeshes& m = tm.m;
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    const int i = blockIdx.x / bpp;
    const int c = (blockIdx.x - i * bpp) * 16 + q;
    if (c >= s_count) return;                               // whole quads leave together
    const long long slot = (long long)i * s_count + c;
    float o[3], d[3];
    unsigned bits[2];
    const bool traced = nu_relight_shadow_ray(irow + (long long)sel[i] * NU_RL_ROW, S, s0 + c, seed, eps, o, d, bits);
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float keep = 1.0f;
    float* dp = DUMP ? dump + slot * NU_RLN_LIGHT_DUMP : nullptr;
    if (DUMP && sub == 0) {
        for (int k = 0; k < NU_RLN_LIGHT_DUMP; ++k) dp[k] = 0.0f;
        for (int k = 0; k < 3; ++k) { dp[k] = o[k]; dp[3 + k] = d[k]; }
        dp[6] = traced ? 1.0f : 0.0f;
    }
    int phase = traced ? 0 : 3;
    while (phase != 3) {
        int found, id;
        float t;
        nu_walk_quad(stack, q, sub, phase == 0 ? m.bvh_i : m.bvh_o, phase == 0 ? m.Li : m.Lo, o, d, 0.0f, 1e16f, phase != 1, found, id, t);
        if (phase == 0) {
            if (DUMP && sub == 0) dp[7] = found ? 1.0f : 0.0f;
            phase = found ? 3 : 1;
        } else if (phase == 1) {
            if (DUMP && sub == 0) { dp[8] = found ? 1.0f : 0.0f; dp[9] = __int_as_float(id); dp[10] = found ? t : 0.0f; }
            if (!found) {                                   // a leaky shell: the direction leaves unrefracted
                out = make_float4(d[0], d[1], d[2], 1.0f);
                phase = 3;
            } else {
                float o2[3], d2[3];
                const bool ok = nu_rlt_leave(m.Vo, m.Fo, m.VNo, m.ior, tm.thick, tm.curv, o, d, id, t, eps, o2, d2, keep);
                if (DUMP && sub == 0) {
                    dp[11] = ok ? 1.0f : 0.0f;
                    for (int k = 0; k < 3; ++k) { dp[12 + k] = o2[k]; dp[15 + k] = d2[k]; }
                    dp[19] = keep;
                }
                for (int k = 0; k < 3; ++k) { o[k] = o2[k]; d[k] = d2[k]; }
                phase = ok ? 2 : 3;
            }
        } else {
            if (DUMP && sub == 0) dp[18] = found ? 1.0f : 0.0f;
            if (!found) out = make_float4(d[0], d[1], d[2], keep);
            phase = 3;
        }
    }
    if (sub == 0) rec[slot] = out;
}

#define NU_THIN_ARGS NU_NESTED_ARGS, const float* thickness, const float* curvature
#define NU_THIN_PASS NU_NESTED_PASS, thickness, curvature
static int nu_thin_meshes(NU_THIN_ARGS, NuThinMeshes& tm) {
    if (!thickness || !curvature) return NU_ERR_ARG;
    tm.thick = thickness; tm.curv = curvature;
    return nu_nested_meshes(NU_NESTED_PASS, tm.m);
}

static int nu_thin_chain_launch(NU_THIN_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int* kind, float* chain,
                                float* inner_rows, float* seg, float* aux, bool dump, hipStream_t stream) {
    NuThinMeshes tm;
    if (n_pix < 0 || nu_thin_meshes(NU_THIN_PASS, tm) != NU_OK) return NU_ERR_ARG;
    if (n_pix == 0) return NU_OK;
    if (!gbuf || !pix || !kind || !chain || !inner_rows || (dump && (!seg || !aux))) return NU_ERR_ARG;
    const dim3 grid(nu_cdiv(n_pix, 16));
    if (dump)
        hipLaunchKernelGGL((relight_thin_chain_kernel<true>), grid, dim3(64), 0, stream, tm, gbuf, pix, n_pix, eps, kind, chain, inner_rows,
                           seg, aux);
    else
        hipLaunchKernelGGL((relight_thin_chain_kernel<false>), grid, dim3(64), 0, stream, tm, gbuf, pix, n_pix, eps, kind, chain, inner_rows,
                           seg, aux);
    return nu_launch_status();
}
extern "C" int nu_relight_thin_chain(NU_THIN_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int* kind, float* chain,
                                     float* inner_rows, hipStream_t stream) {
    return nu_thin_chain_launch(NU_THIN_PASS, gbuf, pix, n_pix, eps, kind, chain, inner_rows, nullptr, nullptr, false, stream);
}
extern "C" int nu_relight_thin_chain_dump(NU_THIN_ARGS, const float* gbuf, const int* pix, int n_pix, float eps, int* kind, float* chain,
                                          float* inner_rows, float* seg, float* aux, hipStream_t stream) {
    return nu_thin_chain_launch(NU_THIN_PASS, gbuf, pix, n_pix, eps, kind, chain, inner_rows, seg, aux, true, stream);
}

static int nu_thin_light_launch(NU_THIN_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                int seed, float eps, float* rec, float* dump, bool dumping, hipStream_t stream) {
    NuThinMeshes tm;
    if (n_sel < 0 || samples < 2 || (samples & 1) || s0 < 0 || s_count < 0 || s0 + s_count > samples) return NU_ERR_ARG;
    if (nu_thin_meshes(NU_THIN_PASS, tm) != NU_OK) return NU_ERR_ARG;
    if (n_sel == 0 || s_count == 0) return NU_OK;
    if (!inner_rows || !sel || !rec || (dumping && !dump)) return NU_ERR_ARG;
    const int bpp = nu_cdiv(s_count, 16);
    const long long blocks = (long long)n_sel * bpp;
    if (blocks > 0x7fffffffLL) return NU_ERR_ARG;         // the caller chunks over pixels / samples
    if (dumping)
        hipLaunchKernelGGL((relight_thin_light_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, stream, tm, inner_rows, sel, samples, s0,
                           s_count, bpp, (unsigned)seed, eps, (float4*)rec, dump);
    else
        hipLaunchKernelGGL((relight_thin_light_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, stream, tm, inner_rows, sel, samples, s0,
                           s_count, bpp, (unsigned)seed, eps, (float4*)rec, dump);
    return nu_launch_status();
}
extern "C" int nu_relight_thin_light(NU_THIN_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                     int seed, float eps, float* rec, hipStream_t stream) {
    return nu_thin_light_launch(NU_THIN_PASS, inner_rows, sel, n_sel, samples, s0, s_count, seed, eps, rec, nullptr, false, stream);
}
extern "C" int nu_relight_thin_light_dump(NU_THIN_ARGS, const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                          int seed, float eps, float* rec, float* dump, hipStream_t stream) {
    return nu_thin_light_launch(NU_THIN_PASS, inner_rows, sel, n_sel, samples, s0, s_count, seed, eps, rec, dump, true, stream);
}

// nu_rlt_cross row by row (tests): M rows in, the crossing's outputs out
__global__ __launch_bounds__(256) void relight_thin_cross_kernel(const float* __restrict__ d, const float* __restrict__ nraw,
                                                                 const float* __restrict__ x, const float* __restrict__ ior,
                                                                 const float* __restrict__ thick, const float* __restrict__ gk, int M,
                                                                 int inside, unsigned char* __restrict__ refracts,
                                                                 unsigned char* __restrict__ tir_ok, float* __restrict__ nrm,
                                                                 float* __restrict__ pend, float* __restrict__ ns, float* __restrict__ nd,
                                                                 float* __restrict__ fres) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    float dd[3], nn[3], xx[3], on[3], oe[3], os[3], od[3], f_a, f_b;
    for (int k = 0; k < 3; ++k) { dd[k] = d[r * 3LL + k]; nn[k] = nraw[r * 3LL + k]; xx[k] = x[r * 3LL + k]; }
    bool rf, ok;
    nu_rlt_cross(dd, xx, nn, ior[r], thick[r], gk[r], inside != 0, rf, ok, on, oe, os, od, f_a, f_b);
    refracts[r] = rf ? 1 : 0;
    tir_ok[r] = ok ? 1 : 0;
    for (int k = 0; k < 3; ++k) { nrm[r * 3LL + k] = on[k]; pend[r * 3LL + k] = oe[k]; ns[r * 3LL + k] = os[k]; nd[r * 3LL + k] = od[k]; }
    fres[r * 2LL] = f_a; fres[r * 2LL + 1] = f_b;
}
extern "C" int nu_relight_thin_cross(const float* d, const float* normal, const float* x, const float* ior, const float* thickness,
                                     const float* curvature, int M, int inside, unsigned char* refracts, unsigned char* tir_ok, float* nrm,
                                     float* pend, float* ns, float* nd, float* fres, hipStream_t stream) {
    if (M < 0) return NU_ERR_ARG;
    if (M == 0) return NU_OK;
    if (!d || !normal || !x || !ior || !thickness || !curvature || !refracts || !tir_ok || !nrm || !pend || !ns || !nd || !fres)
        return NU_ERR_ARG;
    hipLaunchKernelGGL(relight_thin_cross_kernel, dim3(nu_cdiv(M, 256)), dim3(256), 0, stream, d, normal, x, ior, thickness, curvature, M,
                       inside, refracts, tir_ok, nrm, pend, ns, nd, fres);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// visibility transfer: ONE surface point per single-wave block, all its hemisphere rays in this launch, reduced in the wave.
// A round is 16 quads = 16 consecutive samples: each quad makes its ray in registers (relight.h) and walks it any-hit on the one stack;
// lane 0 of the quad leaves the sample's NU_TR_LIVE contributions (zero when occluded) in `red`, and lanes 0 .. NU_TR_LIVE - 1, one per
// output column, add the round's 16 entries IN SAMPLE ORDER to a register.  No verdict, no ray and no partial sum goes to memory: the
// point's row is the only store, and its bits depend on nothing but the point, its id, the sample parameters and the mesh.
// ------------------------------------------------------------------------------------------------
template <bool DUMP>
__global__ __launch_bounds__(64) void transfer_bake_kernel(const char* __restrict__ buf, NuBvhLayout L, const float* __restrict__ points,
                                                           const float* __restrict__ normals, int id0, int S, unsigned seed, float eps,
                                                           float radius, float* __restrict__ out, unsigned char* __restrict__ vis) {
    __shared__ int stack[NU_WSTACK][16];
    __shared__ float red[16][NU_TR_ROW];
    const int lane = threadIdx.x & 63, sub = lane & 3, q = lane >> 2;
    const long long i = blockIdx.x;
    const int id = (int)((unsigned)id0 + (unsigned)blockIdx.x);
    float p[3], n[3];
    for (int k = 0; k < 3; ++k) { p[k] = points[i * 3 + k]; n[k] = normals[i * 3 + k]; }
    float acc = 0.0f;
    for (int s0 = 0; s0 < S; s0 += 16) {                    // every lane of the wave takes every round: the barriers are uniform
        const int s = s0 + q;
        unsigned bits[2];
        float o[3], d[3];
        nu_transfer_uniforms(id, seed, S, s, bits);
        nu_transfer_ray(p, n, eps, bits, o, d);
        int found, fid;
        float t;
        nu_walk_quad(stack, q, sub, buf, L, o, d, 0.0f, radius, true, found, fid, t);
        if (sub == 0) {
            float c[NU_TR_LIVE];
            nu_transfer_contrib(d, c);
#pragma unroll
            for (int k = 0; k < NU_TR_LIVE; ++k) red[q][k] = found ? 0.0f : c[k];
            if (DUMP) vis[i * S + s] = found ? 0 : 1;
        }
        __syncthreads();
        if (lane < NU_TR_LIVE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc = acc + red[r][lane];
        }
        __syncthreads();                                    // the next round overwrites red
    }
    if (lane < NU_TR_LIVE) red[0][lane] = acc;
    __syncthreads();
    if (lane < NU_TR_ROW) {
        float sum[NU_TR_LIVE];
#pragma unroll
        for (int k = 0; k < NU_TR_LIVE; ++k) sum[k] = red[0][k];
        out[i * NU_TR_ROW + lane] = nu_transfer_finish(sum, n, S, lane);       // one 64-byte row
    }
}

static int nu_transfer_launch(const void* bvh, int n_faces, const float* points, const float* normals, int n, int id0, int samples,
                              int seed, float eps, float radius, float* out, unsigned char* vis, bool dump, hipStream_t stream) {
    if (n < 0 || n_faces <= 0 || samples < 16 || (samples & 15)) return NU_ERR_ARG;
    if (!(eps > -3e38f && eps < 3e38f) || !(radius > 0.0f && radius < 3e38f)) return NU_ERR_ARG;
    if ((long long)n * samples > 0x7fffffffLL) return NU_ERR_ARG;          // the caller chunks over points (nu_transfer_rays' count)
    if (n == 0) return NU_OK;
    if (!bvh || !points || !normals || !out || (dump && !vis)) return NU_ERR_ARG;
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    if (dump)
        hipLaunchKernelGGL((transfer_bake_kernel<true>), dim3((unsigned)n), dim3(64), 0, stream, (const char*)bvh, L, points, normals, id0,
                           samples, (unsigned)seed, eps, radius, out, vis);
    else
        hipLaunchKernelGGL((transfer_bake_kernel<false>), dim3((unsigned)n), dim3(64), 0, stream, (const char*)bvh, L, points, normals, id0,
                           samples, (unsigned)seed, eps, radius, out, vis);
    return nu_launch_status();
}
extern "C" int nu_transfer_bake(const void* bvh, int n_faces, const float* points, const float* normals, int n, int id0, int samples,
                                int seed, float eps, float radius, float* out, hipStream_t stream) {
    return nu_transfer_launch(bvh, n_faces, points, normals, n, id0, samples, seed, eps, radius, out, nullptr, false, stream);
}
extern "C" int nu_transfer_bake_dump(const void* bvh, int n_faces, const float* points, const float* normals, int n, int id0, int samples,
                                     int seed, float eps, float radius, float* out, unsigned char* vis, hipStream_t stream) {
    return nu_transfer_launch(bvh, n_faces, points, normals, n, id0, samples, seed, eps, radius, out, vis, true, stream);
}

// brute-force closest hit on the device (same triangle test; O(N*F)): cross-check + tiny meshes
__global__ __launch_bounds__(256) void brute_trace_kernel(const float* __restrict__ V, const int* __restrict__ F, int nf,
                                                          const float* __restrict__ rays, int N, float tmin, float tmax,
                                                          float* __restrict__ hit, int* __restrict__ idx, float* __restrict__ tout) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) { o[k] = rays[r * 6LL + k]; d[k] = rays[r * 6LL + 3 + k]; }
    float best_t = tmax;
    int best_id = NU_MISS_INDEX;
    bool found = false;
    for (int f = 0; f < nf; ++f) {
        float v[3][3];
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 3; ++k) v[a][k] = V[F[f * 3 + a] * 3LL + k];
        float t;
        if (nu_ray_tri(o, d, v[0], v[1], v[2], tmin, tmax, t)) {
            if (!found || t < best_t) { best_t = t; best_id = f; found = true; }   // ascending f: ties keep the lowest id
        }
    }
    hit[r] = found ? 1.0f : 0.0f;
    idx[r] = best_id;
    if (tout) tout[r] = found ? best_t : 0.0f;
}
extern "C" int nu_brute_trace(const float* V, const int* F, int n_faces, const float* rays, int N, float tmin, float tmax,
                              float* hit, int* idx, float* t_out, hipStream_t stream) {
    if (N <= 0) return NU_OK;
    hipLaunchKernelGGL(brute_trace_kernel, dim3(nu_cdiv(N, 256)), dim3(256), 0, stream, V, F, n_faces, rays, N, tmin, tmax, hit,
                       idx, t_out);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------
// closest point on the mesh (postprocess of the stage-2 mesh, mesh distances).  Same tree, same file-wide single-rounding rule:
// the LBVH result is defined bit-exactly against the O(N*F) sweep below and tests/closest_point_oracle.py.
// ------------------------------------------------------------------------------------------------
// closest point on the segment [a, b] (Ericson, Real-Time Collision Detection 5.1.2); a zero-length segment gives a
static __device__ inline void nu_closest_seg(const float* p, const float* a, const float* b, float* q) {
    float ab[3], ap[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ap[k] = p[k] - a[k]; }
    const float t = nu_dot3_rn(ap, ab);
    if (t <= 0.0f) { for (int k = 0; k < 3; ++k) q[k] = a[k]; return; }
    const float den = nu_dot3_rn(ab, ab);
    if (t >= den) { for (int k = 0; k < 3; ++k) q[k] = b[k]; return; }
    const float s = t / den;
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * s;
}
static __device__ inline float nu_dist2(const float* p, const float* q) {
    float e[3];
    for (int k = 0; k < 3; ++k) e[k] = p[k] - q[k];
    return nu_dot3_rn(e, e);
}
// minimum over the three edges as segments, in the order ab, bc, ca (a later edge wins only when strictly nearer)
static __device__ inline float nu_closest_edges(const float* p, const float* a, const float* b, const float* c, float* q) {
    float q1[3];
    nu_closest_seg(p, a, b, q);
    float best = nu_dist2(p, q);
    nu_closest_seg(p, b, c, q1);
    float d = nu_dist2(p, q1);
    if (d < best) { best = d; for (int k = 0; k < 3; ++k) q[k] = q1[k]; }
    nu_closest_seg(p, c, a, q1);
    d = nu_dist2(p, q1);
    if (d < best) { best = d; for (int k = 0; k < 3; ++k) q[k] = q1[k]; }
    return best;
}
// closest point q on the triangle abc to p and d2 = |p - q|^2: the vertex / edge / face regions of Ericson 5.1.5.  A triangle
// with dot(n, n) == 0 (n = ab x ac: a zero-area sliver, as marching cubes emits) takes the minimum over its edges; so does a sliver
// whose rounded face-region weights va, vb, vc are not all >= 0 with a positive sum -- this keeps q on the triangle (inside its
// padded box, see nu_box_dist2) and finite.  No sqrt anywhere (hipcc's v_sqrt_f32 is not correctly rounded).
static __device__ inline float nu_closest_tri(const float* p, const float* a, const float* b, const float* c, float* q) {
    float ab[3], ac[3], n[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; }
    nu_cross_rn(ab, ac, n);
    if (nu_dot3_rn(n, n) == 0.0f) return nu_closest_edges(p, a, b, c, q);
    for (int k = 0; k < 3; ++k) ap[k] = p[k] - a[k];
    const float d1 = nu_dot3_rn(ab, ap), d2 = nu_dot3_rn(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) { for (int k = 0; k < 3; ++k) q[k] = a[k]; return nu_dist2(p, q); }
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const float d3 = nu_dot3_rn(ab, bp), d4 = nu_dot3_rn(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) { for (int k = 0; k < 3; ++k) q[k] = b[k]; return nu_dist2(p, q); }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float den = d1 - d3;                // >= 0; exactly 0 only where both dots round to 0 (a vanishing edge): take a
        const float v = den > 0.0f ? d1 / den : 0.0f;
        for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * v;
        return nu_dist2(p, q);
    }
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const float d5 = nu_dot3_rn(ab, cp), d6 = nu_dot3_rn(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) { for (int k = 0; k < 3; ++k) q[k] = c[k]; return nu_dist2(p, q); }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float den = d2 - d6;
        const float w = den > 0.0f ? d2 / den : 0.0f;
        for (int k = 0; k < 3; ++k) q[k] = a[k] + ac[k] * w;
        return nu_dist2(p, q);
    }
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        const float den = e43 + e56;
        const float w = den > 0.0f ? e43 / den : 0.0f;
        for (int k = 0; k < 3; ++k) q[k] = b[k] + (c[k] - b[k]) * w;
        return nu_dist2(p, q);
    }
    const float sum = (va + vb) + vc;
    if (!(va >= 0.0f && vb >= 0.0f && vc >= 0.0f && sum > 0.0f)) return nu_closest_edges(p, a, b, c, q);
    const float denom = 1.0f / sum;
    const float v = vb * denom, w = vc * denom;
    for (int k = 0; k < 3; ++k) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
    return nu_dist2(p, q);
}

// squared distance from p to the box (0 inside).  Conservative against nu_closest_tri: every q it returns lies on its triangle up to
// the rounding of one convex combination, far below the eps the refit pads each leaf box with (lbvh_refit_kernel), so q is inside
// every box that holds the triangle; per axis rn(p - q) is then at least rn(p - bmax) (or rn(bmin - p)) in magnitude, and
// round-to-nearest squares and sums are monotone, so the computed box distance never exceeds the triangle's computed d2.
static __device__ inline float nu_box_dist2(const float* p, const float* bmin, const float* bmax) {
    float e[3];
    for (int k = 0; k < 3; ++k) e[k] = fmaxf(fmaxf(bmin[k] - p[k], p[k] - bmax[k]), 0.0f);
    return nu_dot3_rn(e, e);
}

// One query per lane over the binary nodes: depth first, the nearer child (box distance) first, a box culled only when its
// distance is STRICTLY greater than the running best (an equal distance can still hold a lower face id), the best kept in
// lexicographic (d2, face id) order and started at max_d2.  The stack holds (node, box distance) per lane in LDS,
// wavefront-interleaved; a popped entry the running best has overtaken is skipped without its node being fetched.
// First pass (RETRACE = false): a SHORT ring of STACK entries.  While the walk starts unbounded (max_d2 = inf) every level pushes,
// so the ring drops its oldest entry instead of failing; a query that dropped one writes its best so far, marked
// (idx = -1 - face id).  The second pass re-walks exactly the marked queries with the full NU_STACK (a Morton tree over 62-bit keys
// is at most 62 deep) and starts from that best, which is a real candidate, so its bound is tight from the root on.
template <int STACK, bool RETRACE, int WPB>
__global__ __launch_bounds__(64 * WPB) void lbvh_closest_kernel(const char* __restrict__ buf, NuBvhLayout L, const float* __restrict__ pts,
                                                                int N, float max_d2, float* __restrict__ d2out, int* __restrict__ idx,
                                                                float* __restrict__ qout) {
    static_assert((STACK & (STACK - 1)) == 0, "ring indexing needs a power of two");
    __shared__ int snode[WPB][STACK][64];
    __shared__ float sdist[WPB][STACK][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float best = max_d2;
    int best_id = NU_MISS_INDEX;
    if (RETRACE) {
        const int m = idx[r];
        if (m >= 0) return;
        best_id = -1 - m;
        if (best_id != NU_MISS_INDEX) best = d2out[r];
    }
    const NuBvhHeader* h = (const NuBvhHeader*)(buf + L.header);
    const NuBvhNode* nodes = (const NuBvhNode*)(buf + L.nodes);
    const float* tris = (const float*)(buf + L.tris);
    const int* ids = (const int*)(buf + L.ids);
    const int n = h->n_faces;
    float p[3];
    for (int k = 0; k < 3; ++k) p[k] = pts[r * 3LL + k];
    float bq[3] = {0.f, 0.f, 0.f};
    bool improved = false;

    auto test_leaf = [&](int pos) {
        const float4* tp = (const float4*)(tris + pos * 12LL);
        const float4 A = tp[0], B = tp[1], C = tp[2];
        const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
        float q[3];
        const float d = nu_closest_tri(p, a, b, c, q);
        const int id = ids[pos];
        if (d < best || (d == best && id < best_id)) {
            best = d; best_id = id; improved = true;
            for (int k = 0; k < 3; ++k) bq[k] = q[k];
        }
    };

    bool dropped = false;
    if (n == 1) {
        test_leaf(0);
    } else {
        int top = 0, cnt = 0;            // ring: entries top - cnt .. top - 1 (mod STACK), the newest at top - 1
        int node = 0;
        while (true) {
            const NuBvhNode nd = nodes[node];
            const float dl = nu_box_dist2(p, nd.lmin, nd.lmax), dr = nu_box_dist2(p, nd.rmin, nd.rmax);
            if (nd.left < 0 && dl <= best) test_leaf(-1 - nd.left);
            if (nd.right < 0 && dr <= best) test_leaf(-1 - nd.right);
            const bool il = nd.left >= 0 && dl <= best, ir = nd.right >= 0 && dr <= best;
            int next = -1;
            if (il && ir) {
                const bool left_first = dl <= dr;
                next = left_first ? nd.left : nd.right;
                snode[w][top][lane] = left_first ? nd.right : nd.left;
                sdist[w][top][lane] = left_first ? dr : dl;
                top = (top + 1) & (STACK - 1);
                if (cnt < STACK) ++cnt;
                else dropped = true;     // the oldest entry was overwritten (never in the full-stack pass: depth <= 62)
            } else if (il) {
                next = nd.left;
            } else if (ir) {
                next = nd.right;
            }
            while (next < 0 && cnt > 0) {
                top = (top - 1) & (STACK - 1);
                --cnt;
                if (sdist[w][top][lane] <= best) next = snode[w][top][lane];
            }
            if (next < 0) break;
            node = next;
        }
    }
    if (!RETRACE && dropped) {           // incomplete: the second pass finishes this query from its best so far
        idx[r] = -1 - best_id;
        if (best_id != NU_MISS_INDEX) {
            d2out[r] = best;
            if (qout) for (int k = 0; k < 3; ++k) qout[r * 3LL + k] = bq[k];
        }
        return;
    }
    if (RETRACE && !improved) {          // the first pass's candidate stands (its d2 and point are already written)
        idx[r] = best_id;
        if (best_id != NU_MISS_INDEX) return;
    }
    const bool hit = best_id != NU_MISS_INDEX;
    d2out[r] = hit ? best : __int_as_float(0x7f800000);
    idx[r] = best_id;
    if (qout) for (int k = 0; k < 3; ++k) qout[r * 3LL + k] = hit ? bq[k] : 0.0f;
}

#define NU_CLOSEST_SHORT 16
extern "C" int nu_lbvh_closest(const void* bvh, int n_faces, const float* pts, int N, float max_d2, float* d2, int* idx, float* closest,
                               hipStream_t stream) {
    if (N <= 0) return NU_OK;
    if (n_faces <= 0 || !bvh || !pts || !d2 || !idx) return NU_ERR_ARG;
    const NuBvhLayout L = nu_bvh_layout(n_faces);
    // both passes on the caller's stream, in order: the second reads the marks the first wrote
    hipLaunchKernelGGL((lbvh_closest_kernel<NU_CLOSEST_SHORT, false, 4>), dim3(nu_cdiv(N, 256)), dim3(256), 0, stream, (const char*)bvh, L,
                       pts, N, max_d2, d2, idx, closest);
    hipLaunchKernelGGL((lbvh_closest_kernel<NU_STACK, true, 1>), dim3(nu_cdiv(N, 64)), dim3(64), 0, stream, (const char*)bvh, L, pts, N,
                       max_d2, d2, idx, closest);
    return nu_launch_status();
}

// brute-force closest point on the device (same point/triangle routine; O(N*F)): cross-check + small meshes
__global__ __launch_bounds__(256) void brute_closest_kernel(const float* __restrict__ V, const int* __restrict__ F, int nf,
                                                            const float* __restrict__ pts, int N, float max_d2, float* __restrict__ d2out,
                                                            int* __restrict__ idx, float* __restrict__ qout) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float p[3];
    for (int k = 0; k < 3; ++k) p[k] = pts[r * 3LL + k];
    float best = max_d2, bq[3] = {0.f, 0.f, 0.f};
    int best_id = NU_MISS_INDEX;
    for (int f = 0; f < nf; ++f) {
        float v[3][3], q[3];
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 3; ++k) v[a][k] = V[F[f * 3 + a] * 3LL + k];
        const float d = nu_closest_tri(p, v[0], v[1], v[2], q);
        if (d < best || (d == best && best_id == NU_MISS_INDEX)) {      // ascending f: ties keep the lowest id
            best = d; best_id = f;
            for (int k = 0; k < 3; ++k) bq[k] = q[k];
        }
    }
    const bool hit = best_id != NU_MISS_INDEX;
    d2out[r] = hit ? best : __int_as_float(0x7f800000);
    idx[r] = best_id;
    if (qout) for (int k = 0; k < 3; ++k) qout[r * 3LL + k] = hit ? bq[k] : 0.0f;
}
extern "C" int nu_brute_closest(const float* V, const int* F, int n_faces, const float* pts, int N, float max_d2, float* d2, int* idx,
                                float* closest, hipStream_t stream) {
    if (N <= 0) return NU_OK;
    if (n_faces <= 0 || !V || !F || !pts || !d2 || !idx) return NU_ERR_ARG;
    hipLaunchKernelGGL(brute_closest_kernel, dim3(nu_cdiv(N, 256)), dim3(256), 0, stream, V, F, n_faces, pts, N, max_d2, d2, idx,
                       closest);
    return nu_launch_status();
}
