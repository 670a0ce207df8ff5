// mcubes.hip -- mesh extraction from a dense SDF grid (reference: extract_mesh_stage1.py, network/field.py:1286-1317, which run
// PyMCubes on a host numpy grid): marching cubes on a device grid, and the compaction / scatter that evaluates the grid's
// inside-the-unit-sphere points through the SDF MLP without a host copy.
//
// Grid: u[nx][ny][nz], fp32, C order, point p = (i ny + j) nz + k, addressed in 64-bit (1024^3 x 3 overflows int32).
// Work unit: a BRICK of 256 consecutive points (one 256-thread workgroup, thread = point).  Every pass below is a count or a
// write over bricks; the per-brick counts go through one reduce-then-scan (no workgroup ever waits on another), and the write
// passes recompute their brick and place its items by an in-brick prefix.  Output positions therefore follow the linear point
// order: no atomics decide where anything lands, and two runs give the same bits.
//
// Marching cubes (tables: mc_tables.h; a corner is INSIDE when u < iso):
//   vertices   point p owns the edges +x, +y, +z from p; a straddling edge gives ONE vertex, shared by every triangle on it.
//              Order: (owner p, axis).  Position in index space: p + t e_axis, t = (iso - u_p) / (u_{p+e} - u_p)
//   triangles  cell = its first corner p (i < nx-1, j < ny-1, k < nz-1).  Order: (cell, table slot)
//   passes     nu_mc_count (brick totals) -> nu_mc_scan (exclusive offsets, grand totals) -> [host reads the totals once] ->
//              nu_mc_write_vertices (V, and first_vid[p] at every owner) -> nu_mc_write_triangles (reads first_vid)
// Grid compaction (sdf evaluation of the points with |x| < 1):
//   nu_grid_inside_count (brick counts + the same scan + row offsets of the chunks) -> per chunk: nu_grid_compact (x rows) ->
//   SDF MLP -> nu_grid_scatter (u = sdf inside, outside_val elsewhere)
#include "nu_common.h"
#include "mc_tables.h"

#define MC_BRICK 256
#define MC_SCAN_PER_THREAD 16
#define MC_SCAN_CHUNK (MC_BRICK * MC_SCAN_PER_THREAD)      // bricks per workgroup of the scan's reduce / downsweep passes

// ------------------------------------------------------------------------------------------------ workspace
// [cnt: int2 per brick][off: long long2 per brick + 1 (exclusive; off[nb] = totals)][bsum: long long2 per scan chunk]
struct McWs {
    int* cnt;
    long long* off;
    long long* bsum;
    long long nb, nchunk;
};

static __host__ __device__ inline long long mc_align(long long b) { return (b + 255) / 256 * 256; }

static inline bool mc_ws(void* ws, long long ws_bytes, long long npts, McWs& w) {
    w.nb = (npts + MC_BRICK - 1) / MC_BRICK;
    w.nchunk = (w.nb + MC_SCAN_CHUNK - 1) / MC_SCAN_CHUNK;
    const long long b_cnt = mc_align(w.nb * 2 * 4), b_off = mc_align((w.nb + 1) * 2 * 8), b_bsum = mc_align(w.nchunk * 2 * 8);
    if (ws == nullptr || ws_bytes < b_cnt + b_off + b_bsum) return false;
    char* p = static_cast<char*>(ws);
    w.cnt = reinterpret_cast<int*>(p);
    w.off = reinterpret_cast<long long*>(p + b_cnt);
    w.bsum = reinterpret_cast<long long*>(p + b_cnt + b_off);
    return true;
}

static inline bool mc_dims_ok(int nx, int ny, int nz) { return nx >= 2 && ny >= 2 && nz >= 2; }

extern "C" long long nu_mc_workspace_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return NU_ERR_ARG;
    const long long nb = ((long long)nx * ny * nz + MC_BRICK - 1) / MC_BRICK;
    const long long nchunk = (nb + MC_SCAN_CHUNK - 1) / MC_SCAN_CHUNK;
    return mc_align(nb * 2 * 4) + mc_align((nb + 1) * 2 * 8) + mc_align(nchunk * 2 * 8);
}

// ------------------------------------------------------------------------------------------------ block prefix helpers
// exclusive prefix of v over the 256 threads of a workgroup (4 waves: shuffle scan inside a wave, wave totals through LDS);
// *total gets the workgroup's sum
template <typename T>
static __device__ inline T mc_block_excl(T v, T* lds4, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds4[wv] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const T s = lds4[w];
        base += w < wv ? s : T(0);
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return base + inc - v;
}

// exclusive prefix of a 0/1 flag over the workgroup: wave64 ballot + popcount, wave totals through LDS
static __device__ inline int mc_block_excl_bit(bool f, int* lds4) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    if (lane == 0) lds4[wv] = __popcll(m);
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) base += w < wv ? lds4[w] : 0;
    __syncthreads();
    return base + __popcll(m & below);
}

// ------------------------------------------------------------------------------------------------ reduce-then-scan
// pass 1: per scan chunk (MC_SCAN_CHUNK bricks) the sums of both components
__global__ __launch_bounds__(256) void mc_scan_reduce_kernel(const int* __restrict__ cnt, long long nb, long long* __restrict__ bsum) {
    __shared__ long long lds[8];
    const long long b0 = blockIdx.x * (long long)MC_SCAN_CHUNK + threadIdx.x * (long long)MC_SCAN_PER_THREAD;
    long long s0 = 0, s1 = 0;
    for (int e = 0; e < MC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < nb) { s0 += cnt[2 * b]; s1 += cnt[2 * b + 1]; }
    }
    long long t0, t1;
    mc_block_excl<long long>(s0, lds, &t0);
    mc_block_excl<long long>(s1, lds + 4, &t1);
    if (threadIdx.x == 0) { bsum[2 * blockIdx.x] = t0; bsum[2 * blockIdx.x + 1] = t1; }
}

// pass 2: one workgroup scans the chunk sums in place (exclusive) and writes the grand totals to off[2 nb .. 2 nb + 1]
__global__ __launch_bounds__(256) void mc_scan_top_kernel(long long* __restrict__ bsum, long long nchunk, long long* __restrict__ off,
                                                         long long nb) {
    __shared__ long long lds[8];
    long long run0 = 0, run1 = 0;
    for (long long c0 = 0; c0 < nchunk; c0 += 256) {
        const long long c = c0 + threadIdx.x;
        const long long v0 = c < nchunk ? bsum[2 * c] : 0, v1 = c < nchunk ? bsum[2 * c + 1] : 0;
        long long t0, t1;
        const long long e0 = mc_block_excl<long long>(v0, lds, &t0);
        const long long e1 = mc_block_excl<long long>(v1, lds + 4, &t1);
        if (c < nchunk) { bsum[2 * c] = run0 + e0; bsum[2 * c + 1] = run1 + e1; }
        run0 += t0;
        run1 += t1;
    }
    if (threadIdx.x == 0) { off[2 * nb] = run0; off[2 * nb + 1] = run1; }
}

// pass 3: every chunk rescans its bricks from its base offset
__global__ __launch_bounds__(256) void mc_scan_down_kernel(const int* __restrict__ cnt, long long nb, const long long* __restrict__ bsum,
                                                          long long* __restrict__ off) {
    __shared__ long long lds[8];
    const long long b0 = blockIdx.x * (long long)MC_SCAN_CHUNK + threadIdx.x * (long long)MC_SCAN_PER_THREAD;
    long long s0 = 0, s1 = 0;
    for (int e = 0; e < MC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < nb) { s0 += cnt[2 * b]; s1 += cnt[2 * b + 1]; }
    }
    long long t0, t1;
    long long r0 = bsum[2 * blockIdx.x] + mc_block_excl<long long>(s0, lds, &t0);
    long long r1 = bsum[2 * blockIdx.x + 1] + mc_block_excl<long long>(s1, lds + 4, &t1);
    for (int e = 0; e < MC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < nb) {
            off[2 * b] = r0;
            off[2 * b + 1] = r1;
            r0 += cnt[2 * b];
            r1 += cnt[2 * b + 1];
        }
    }
}

static int mc_scan_launch(const McWs& w, hipStream_t stream) {
    hipLaunchKernelGGL(mc_scan_reduce_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, stream, w.cnt, w.nb, w.bsum);
    hipLaunchKernelGGL(mc_scan_top_kernel, dim3(1), dim3(256), 0, stream, w.bsum, w.nchunk, w.off, w.nb);
    hipLaunchKernelGGL(mc_scan_down_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, stream, w.cnt, w.nb, w.bsum, w.off);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ marching cubes
struct McPoint {
    long long p;
    int i, j, k;
};

static __device__ inline McPoint mc_point(long long p, int ny, int nz) {
    McPoint q;
    q.p = p;
    const long long plane = (long long)ny * nz;
    q.i = (int)(p / plane);
    const long long r = p - (long long)q.i * plane;
    q.j = (int)(r / nz);
    q.k = (int)(r - (long long)q.j * nz);
    return q;
}

// bits 0..2: the +x / +y / +z edges of q straddle iso (and exist)
static __device__ inline int mc_owned(const float* __restrict__ u, const McPoint& q, int nx, int ny, int nz, float iso) {
    const long long sx = (long long)ny * nz;
    const bool in0 = u[q.p] < iso;
    int m = 0;
    if (q.i + 1 < nx && ((u[q.p + sx] < iso) != in0)) m |= 1;
    if (q.j + 1 < ny && ((u[q.p + nz] < iso) != in0)) m |= 2;
    if (q.k + 1 < nz && ((u[q.p + 1] < iso) != in0)) m |= 4;
    return m;
}

// cube index of the cell whose first corner is q (corner numbering: mc_tables.h), -1 when q opens no cell
static __device__ inline int mc_cube(const float* __restrict__ u, const McPoint& q, int nx, int ny, int nz, float iso) {
    if (q.i + 1 >= nx || q.j + 1 >= ny || q.k + 1 >= nz) return -1;
    const long long sx = (long long)ny * nz, sy = nz;
    const long long p = q.p;
    int c = 0;
    c |= (u[p] < iso) ? 1 : 0;
    c |= (u[p + sx] < iso) ? 2 : 0;
    c |= (u[p + sx + sy] < iso) ? 4 : 0;
    c |= (u[p + sy] < iso) ? 8 : 0;
    c |= (u[p + 1] < iso) ? 16 : 0;
    c |= (u[p + sx + 1] < iso) ? 32 : 0;
    c |= (u[p + sx + sy + 1] < iso) ? 64 : 0;
    c |= (u[p + sy + 1] < iso) ? 128 : 0;
    return c;
}

// owner corner offset (bits 0/1/2: +1 in i/j/k) and axis of each of the 12 cube edges
__constant__ unsigned char mc_edge_owner[12] = {0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 3, 2};
__constant__ unsigned char mc_edge_axis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

static __device__ inline int mc_ntri_of(const signed char* row) {
    int n = 0;
    while (n < 5 && row[3 * n] >= 0) ++n;
    return n;
}

__global__ __launch_bounds__(256) void mc_count_kernel(const float* __restrict__ u, int nx, int ny, int nz, float iso,
                                                      int* __restrict__ cnt) {
    __shared__ unsigned char ntri[256];
    __shared__ int lds[8];
    ntri[threadIdx.x] = (unsigned char)mc_ntri_of(nu_mc_tri_table[threadIdx.x]);
    __syncthreads();
    const long long npts = (long long)nx * ny * nz;
    const long long p = (long long)blockIdx.x * MC_BRICK + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < npts) {
        const McPoint q = mc_point(p, ny, nz);
        nv = __popc(mc_owned(u, q, nx, ny, nz, iso));
        const int c = mc_cube(u, q, nx, ny, nz, iso);
        nt = c >= 0 ? ntri[c] : 0;
    }
    int tv, tt;
    mc_block_excl<int>(nv, lds, &tv);
    mc_block_excl<int>(nt, lds + 4, &tt);
    if (threadIdx.x == 0) { cnt[2 * blockIdx.x] = tv; cnt[2 * blockIdx.x + 1] = tt; }
}

__global__ __launch_bounds__(256) void mc_vertex_kernel(const float* __restrict__ u, int nx, int ny, int nz, float iso,
                                                       const int* __restrict__ cnt, const long long* __restrict__ off,
                                                       float* __restrict__ V, int* __restrict__ first_vid) {
#pragma clang fp contract(off)
    __shared__ int lds[4];
    if (cnt[2 * blockIdx.x] == 0) return;                         // workgroup-uniform: most bricks hold no surface
    const long long npts = (long long)nx * ny * nz;
    const long long p = (long long)blockIdx.x * MC_BRICK + threadIdx.x;
    McPoint q = {};
    int m = 0;
    if (p < npts) {
        q = mc_point(p, ny, nz);
        m = mc_owned(u, q, nx, ny, nz, iso);
    }
    int tot;
    const long long base = off[2 * blockIdx.x] + mc_block_excl<int>(__popc(m), lds, &tot);
    if (m == 0) return;
    first_vid[p] = (int)base;
    const long long sx = (long long)ny * nz;
    const long long step[3] = {sx, (long long)nz, 1};
    const float ua = u[p];
    long long v = base;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1 << a))) continue;
        const float ub = u[p + step[a]];
        const float t = (iso - ua) / (ub - ua);
        float x = (float)q.i, y = (float)q.j, z = (float)q.k;
        if (a == 0) x = x + t;
        else if (a == 1) y = y + t;
        else z = z + t;
        V[3 * v + 0] = x;
        V[3 * v + 1] = y;
        V[3 * v + 2] = z;
        ++v;
    }
}

__global__ __launch_bounds__(256) void mc_triangle_kernel(const float* __restrict__ u, int nx, int ny, int nz, float iso,
                                                         const int* __restrict__ cnt, const long long* __restrict__ off,
                                                         const int* __restrict__ first_vid, int* __restrict__ F) {
    __shared__ signed char tri[256 * 16];
    __shared__ int lds[4];
    if (cnt[2 * blockIdx.x + 1] == 0) return;                     // workgroup-uniform
    for (int e = threadIdx.x; e < 256 * 16; e += 256) tri[e] = nu_mc_tri_table[e >> 4][e & 15];
    __syncthreads();
    const long long npts = (long long)nx * ny * nz;
    const long long p = (long long)blockIdx.x * MC_BRICK + threadIdx.x;
    int c = -1;
    McPoint q = {};
    if (p < npts) {
        q = mc_point(p, ny, nz);
        c = mc_cube(u, q, nx, ny, nz, iso);
    }
    const int nt = c >= 0 ? mc_ntri_of(tri + 16 * c) : 0;
    int tot;
    const long long base = off[2 * blockIdx.x + 1] + mc_block_excl<int>(nt, lds, &tot);
    const long long sx = (long long)ny * nz;
    for (int s = 0; s < 3 * nt; ++s) {
        const int e = tri[16 * c + s];
        const int ow = mc_edge_owner[e], ax = mc_edge_axis[e];
        McPoint o;
        o.i = q.i + (ow & 1);
        o.j = q.j + ((ow >> 1) & 1);
        o.k = q.k + ((ow >> 2) & 1);
        o.p = p + (ow & 1) * sx + ((ow >> 1) & 1) * (long long)nz + ((ow >> 2) & 1);
        // rank of this axis among the edges the owner holds: its straddling edges of lower axis come first
        const int m = ax ? mc_owned(u, o, nx, ny, nz, iso) : 0;
        const int rank = __popc(m & ((1 << ax) - 1));
        F[3 * base + s] = first_vid[o.p] + rank;
    }
}

extern "C" int nu_mc_count(const float* u, int nx, int ny, int nz, float iso, void* workspace, long long workspace_bytes,
                           hipStream_t stream) {
    if (u == nullptr || !mc_dims_ok(nx, ny, nz)) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(workspace, workspace_bytes, (long long)nx * ny * nz, w)) return NU_ERR_WORKSPACE;
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)w.nb), dim3(256), 0, stream, u, nx, ny, nz, iso, w.cnt);
    return nu_launch_status();
}

extern "C" int nu_mc_scan(int nx, int ny, int nz, void* workspace, long long workspace_bytes, long long* totals, hipStream_t stream) {
    if (!mc_dims_ok(nx, ny, nz)) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(workspace, workspace_bytes, (long long)nx * ny * nz, w)) return NU_ERR_WORKSPACE;
    const int rc = mc_scan_launch(w, stream);
    if (rc != NU_OK) return rc;
    if (totals != nullptr && hipMemcpyAsync(totals, w.off + 2 * w.nb, 2 * sizeof(long long), hipMemcpyDeviceToDevice, stream) != hipSuccess)
        return NU_ERR_LAUNCH;
    return NU_OK;
}

extern "C" int nu_mc_write_vertices(const float* u, int nx, int ny, int nz, float iso, const void* workspace, long long workspace_bytes,
                                    float* V, int* first_vid, hipStream_t stream) {
    if (u == nullptr || V == nullptr || first_vid == nullptr || !mc_dims_ok(nx, ny, nz)) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(const_cast<void*>(workspace), workspace_bytes, (long long)nx * ny * nz, w)) return NU_ERR_WORKSPACE;
    hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)w.nb), dim3(256), 0, stream, u, nx, ny, nz, iso, w.cnt, w.off, V, first_vid);
    return nu_launch_status();
}

extern "C" int nu_mc_write_triangles(const float* u, int nx, int ny, int nz, float iso, const void* workspace, long long workspace_bytes,
                                     const int* first_vid, int* F, hipStream_t stream) {
    if (u == nullptr || F == nullptr || first_vid == nullptr || !mc_dims_ok(nx, ny, nz)) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(const_cast<void*>(workspace), workspace_bytes, (long long)nx * ny * nz, w)) return NU_ERR_WORKSPACE;
    hipLaunchKernelGGL(mc_triangle_kernel, dim3((unsigned)w.nb), dim3(256), 0, stream, u, nx, ny, nz, iso, w.cnt, w.off, first_vid, F);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ grid compaction
// inside <=> NOT (torch.norm(x, dim=-1) >= 1), with torch's own arithmetic for a 3-element row: its reduction splits the row over
// two lanes (x^2 + z^2 on one, y^2 on the other, each square rounded), adds the partials, then a correctly rounded sqrt.  Measured
// on the MI355X against torch.norm on 4M points within 3e-7 of the sphere: that order gives 0 mask and 0 norm-bit differences, the
// left-to-right sum differs on 1.2 % of the masks, an fma-contracted sum on 1.6 %.
static __device__ inline bool mc_inside(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                        const McPoint& q, float* xyz) {
#pragma clang fp contract(off)
    // no fma: every square and every sum is rounded on its own (hipcc contracts x x + z z into an fma otherwise, even through
    // __fmul_rn / __fadd_rn, which are plain operators here)
    const float x = X[q.i], y = Y[q.j], z = Z[q.k];
    xyz[0] = x; xyz[1] = y; xyz[2] = z;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = (xx + zz) + yy;
    // sqrt(s) >= 1 <=> s >= 1 for a correctly rounded sqrt (torch's; sqrt(1 - 2^-24) rounds down to 1 - 2^-24), and the compare
    // needs no sqrt here (hipcc's v_sqrt_f32 is 1 ulp)
    return !(s >= 1.0f);
}

__global__ __launch_bounds__(256) void grid_count_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                                        int nx, int ny, int nz, int* __restrict__ cnt) {
    __shared__ int lds[4];
    const long long npts = (long long)nx * ny * nz;
    const long long p = (long long)blockIdx.x * MC_BRICK + threadIdx.x;
    bool in = false;
    if (p < npts) {
        float xyz[3];
        in = mc_inside(X, Y, Z, mc_point(p, ny, nz), xyz);
    }
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[2 * blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
        cnt[2 * blockIdx.x + 1] = 0;
    }
}

__global__ void grid_chunk_rows_kernel(const long long* __restrict__ off, long long nb, long long chunk_bricks, int nchunks,
                                       long long* __restrict__ rows) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nchunks) return;
    long long b = (long long)c * chunk_bricks;
    b = b < nb ? b : nb;
    rows[c] = off[2 * b];
}

// mode 0: write the x rows of the inside points of [p0, p0 + n) (compacted, point order); mode 1: u[p] = inside ? val[row] : outside_val
__global__ __launch_bounds__(256) void grid_compact_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                                          int nx, int ny, int nz, long long p0, long long n,
                                                          const long long* __restrict__ off, int mode, float* __restrict__ rows,
                                                          const float* __restrict__ val, float outside_val, float* __restrict__ u) {
    __shared__ int lds[4];
    const long long b = p0 / MC_BRICK + blockIdx.x;
    const long long p = b * MC_BRICK + threadIdx.x;
    const bool valid = p >= p0 && p < p0 + n;
    float xyz[3];
    const bool in = valid && mc_inside(X, Y, Z, mc_point(p, ny, nz), xyz);
    const long long r = off[2 * b] - off[2 * (p0 / MC_BRICK)] + mc_block_excl_bit(in, lds);
    if (mode == 0) {
        if (in) {
            rows[3 * r + 0] = xyz[0];
            rows[3 * r + 1] = xyz[1];
            rows[3 * r + 2] = xyz[2];
        }
    } else if (valid) {
        u[p] = in ? val[r] : outside_val;
    }
}

static bool grid_args_ok(const float* X, const float* Y, const float* Z, int nx, int ny, int nz) {
    return X != nullptr && Y != nullptr && Z != nullptr && nx > 0 && ny > 0 && nz > 0;
}

extern "C" int nu_grid_inside_count(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long chunk_points,
                                    void* workspace, long long workspace_bytes, long long* chunk_rows, hipStream_t stream) {
    const long long npts = (long long)nx * ny * nz;
    if (!grid_args_ok(X, Y, Z, nx, ny, nz) || chunk_points <= 0 || chunk_points % MC_BRICK != 0 || chunk_rows == nullptr) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(workspace, workspace_bytes, npts, w)) return NU_ERR_WORKSPACE;
    hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)w.nb), dim3(256), 0, stream, X, Y, Z, nx, ny, nz, w.cnt);
    const int rc = mc_scan_launch(w, stream);
    if (rc != NU_OK) return rc;
    const long long nchunks = (npts + chunk_points - 1) / chunk_points;
    hipLaunchKernelGGL(grid_chunk_rows_kernel, dim3((unsigned)nu_cdivl(nchunks + 1, 256)), dim3(256), 0, stream, w.off, w.nb,
                       chunk_points / MC_BRICK, (int)nchunks, chunk_rows);
    return nu_launch_status();
}

static int grid_chunk_launch(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long p0, long long n,
                             const void* workspace, long long workspace_bytes, int mode, float* rows, const float* val, float outside_val,
                             float* u, hipStream_t stream) {
    const long long npts = (long long)nx * ny * nz;
    if (!grid_args_ok(X, Y, Z, nx, ny, nz) || p0 < 0 || p0 % MC_BRICK != 0 || n < 0 || p0 + n > npts) return NU_ERR_ARG;
    McWs w;
    if (!mc_ws(const_cast<void*>(workspace), workspace_bytes, npts, w)) return NU_ERR_WORKSPACE;
    if (n == 0) return NU_OK;
    hipLaunchKernelGGL(grid_compact_kernel, dim3((unsigned)nu_cdivl(n, MC_BRICK)), dim3(256), 0, stream, X, Y, Z, nx, ny, nz, p0, n,
                       w.off, mode, rows, val, outside_val, u);
    return nu_launch_status();
}

extern "C" int nu_grid_compact(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long p0, long long n,
                               const void* workspace, long long workspace_bytes, float* rows, hipStream_t stream) {
    if (rows == nullptr) return NU_ERR_ARG;
    return grid_chunk_launch(X, Y, Z, nx, ny, nz, p0, n, workspace, workspace_bytes, 0, rows, nullptr, 0.f, nullptr, stream);
}

extern "C" int nu_grid_scatter(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long p0, long long n,
                               const void* workspace, long long workspace_bytes, const float* val, float outside_val, float* u,
                               hipStream_t stream) {
    if (u == nullptr) return NU_ERR_ARG;
    return grid_chunk_launch(X, Y, Z, nx, ny, nz, p0, n, workspace, workspace_bytes, 1, nullptr, val, outside_val, u, stream);
}
