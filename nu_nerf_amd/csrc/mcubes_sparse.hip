// mcubes_sparse.hip -- block-sparse mesh extraction: the SDF is evaluated only in the blocks of grid points that the zero set can
// reach, and marching cubes runs on that block list.  The dense path (mcubes.hip) is untouched; with every block
// active the two return the same vertices and triangles bit for bit, in another order.
//
// Grid: the lattice (X[i], Y[j], Z[k]) of the dense path, nx x ny x nz points.  Point-blocks of B^3 points, B = 4 or 8: block
// (bi, bj, bk) owns the points [B bi, B bi + B) per axis, clipped at the grid edge; block id = (bi nby + bj) nbz + bk (int32).
//   slot[nbx][nby][nbz]   int32: -1 for an inactive block, its slot otherwise; active blocks are numbered in ascending block id
//   blocks[nslots]        int32: the block id of every slot
//   u[nslots][B^3]        fp32 values, in-block C order t = (a B + b) B + c; rows r = slot B^3 + t are addressed in 64-bit.
//                         In-block points beyond the grid edge hold padding that nothing reads.
//
// Which blocks (nu_smc_regions, nu_smc_activate): a cell crossed by the isosurface needs its eight corners stored; each block that
// holds one of them contains the whole cell in its REGION, the lattice box [B b - 1, B b + B] per axis clipped to the grid.  The
// region is probed once, at its centre c (pulled radially to |p| = 0.999 when it lies farther out), and is active when the field can
// vanish within r = half diagonal + |c - p| of the probe under the Lipschitz bound lambda.  Region geometry is computed in double
// (a few operations per block), so that a host restatement reproduces the probe points bit for bit.
//
// Marching cubes: the tables, the inside rule u < iso, the edge ownership (+x, +y, +z of the owner point) and the interpolation
// t = (iso - u_p) / (u_q - u_p) of mcubes.hip.  One workgroup per active block (B^3 threads, thread = in-block point): it looks up
// the slots of its 27 neighbour blocks once, gathers the (B+1)^3 halo of values into LDS and classifies from there (the few reads
// two points past the block, for the rank of a vertex among its owner's, go through the slot table).
//   a cell belongs to the block of its min corner and is processed iff all eight corners lie in active blocks
//   an owned edge gives a vertex iff both endpoints are active and straddle
//   vertices are ordered by (slot, in-block point, axis), triangles by (slot, in-block cell, table slot)
//   passes: count -> scan (reduce-then-scan, restated from mcubes.hip with three components) -> [one host read] -> vertices -> triangles;
//   no atomics place anything, so two runs give the same bits.
// Open edges: the count pass also counts the owned straddling edges with an in-grid incident cell that is not processed -- the
// mesh has a hole there, because the band of active blocks cut the surface.  totals = (Nv, Nf, open_edges).
#include "nu_common.h"
#include "mc_tables.h"

#define SMC_SCAN_PER_THREAD 16
#define SMC_SCAN_CHUNK (256 * SMC_SCAN_PER_THREAD)        // slots per workgroup of the scan's reduce / downsweep passes

// ------------------------------------------------------------------------------------------------ workspace
// [cnt: int3 per slot][off: long long3 per slot + 1 (exclusive; off[nslots] = totals)][bsum: long long3 per scan chunk]
struct SmcWs {
    int* cnt;
    long long* off;
    long long* bsum;
    long long n, nchunk;
};

static inline long long smc_align(long long b) { return (b + 255) / 256 * 256; }

static inline long long smc_ws_bytes(long long n, long long* b_cnt, long long* b_off) {
    const long long nchunk = (n + SMC_SCAN_CHUNK - 1) / SMC_SCAN_CHUNK;
    *b_cnt = smc_align(n * 3 * 4);
    *b_off = smc_align((n + 1) * 3 * 8);
    return *b_cnt + *b_off + smc_align(nchunk * 3 * 8);
}

static inline bool smc_ws(void* ws, long long ws_bytes, long long n, SmcWs& w) {
    long long b_cnt, b_off;
    if (n <= 0 || ws == nullptr || ws_bytes < smc_ws_bytes(n, &b_cnt, &b_off)) return false;
    w.n = n;
    w.nchunk = (n + SMC_SCAN_CHUNK - 1) / SMC_SCAN_CHUNK;
    char* p = static_cast<char*>(ws);
    w.cnt = reinterpret_cast<int*>(p);
    w.off = reinterpret_cast<long long*>(p + b_cnt);
    w.bsum = reinterpret_cast<long long*>(p + b_cnt + b_off);
    return true;
}

extern "C" long long nu_smc_workspace_bytes(int nslots) {
    if (nslots <= 0) return NU_ERR_ARG;
    long long b_cnt, b_off;
    return smc_ws_bytes(nslots, &b_cnt, &b_off);
}

// ------------------------------------------------------------------------------------------------ block prefix
// exclusive prefix of v over the NW waves of a workgroup (shuffle scan inside a wave, wave totals through LDS); *total: the sum
template <typename T, int NW>
static __device__ inline T smc_block_excl(T v, T* lds, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const T s = lds[w];
        base += w < wv ? s : T(0);
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------------ reduce-then-scan, 3 components
__global__ __launch_bounds__(256) void smc_scan_reduce_kernel(const int* __restrict__ cnt, long long n, long long* __restrict__ bsum) {
    __shared__ long long lds[4];
    const long long b0 = blockIdx.x * (long long)SMC_SCAN_CHUNK + threadIdx.x * (long long)SMC_SCAN_PER_THREAD;
    long long s[3] = {0, 0, 0};
    for (int e = 0; e < SMC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < n) { s[0] += cnt[3 * b]; s[1] += cnt[3 * b + 1]; s[2] += cnt[3 * b + 2]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long t;
        smc_block_excl<long long, 4>(s[c], lds, &t);
        if (threadIdx.x == 0) bsum[3 * blockIdx.x + c] = t;
    }
}

// one workgroup scans the chunk sums in place (exclusive) and writes the grand totals to off[3 n .. 3 n + 2]
__global__ __launch_bounds__(256) void smc_scan_top_kernel(long long* __restrict__ bsum, long long nchunk, long long* __restrict__ off,
                                                          long long n) {
    __shared__ long long lds[4];
    long long run[3] = {0, 0, 0};
    for (long long c0 = 0; c0 < nchunk; c0 += 256) {
        const long long c = c0 + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long v = c < nchunk ? bsum[3 * c + k] : 0;
            long long t;
            const long long e = smc_block_excl<long long, 4>(v, lds, &t);
            if (c < nchunk) bsum[3 * c + k] = run[k] + e;
            run[k] += t;
        }
    }
    if (threadIdx.x == 0) { off[3 * n] = run[0]; off[3 * n + 1] = run[1]; off[3 * n + 2] = run[2]; }
}

__global__ __launch_bounds__(256) void smc_scan_down_kernel(const int* __restrict__ cnt, long long n, const long long* __restrict__ bsum,
                                                           long long* __restrict__ off) {
    __shared__ long long lds[4];
    const long long b0 = blockIdx.x * (long long)SMC_SCAN_CHUNK + threadIdx.x * (long long)SMC_SCAN_PER_THREAD;
    long long s[3] = {0, 0, 0};
    for (int e = 0; e < SMC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < n) { s[0] += cnt[3 * b]; s[1] += cnt[3 * b + 1]; s[2] += cnt[3 * b + 2]; }
    }
    long long r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long t;
        r[c] = bsum[3 * blockIdx.x + c] + smc_block_excl<long long, 4>(s[c], lds, &t);
    }
    for (int e = 0; e < SMC_SCAN_PER_THREAD; ++e) {
        const long long b = b0 + e;
        if (b < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                off[3 * b + c] = r[c];
                r[c] += cnt[3 * b + c];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the block's view of the grid
struct SmcDims {
    int nx, ny, nz, nbx, nby, nbz;
};

static inline bool smc_dims(int nx, int ny, int nz, int B, SmcDims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || (B != 4 && B != 8)) return false;
    d.nx = nx; d.ny = ny; d.nz = nz;
    d.nbx = (nx + B - 1) / B; d.nby = (ny + B - 1) / B; d.nbz = (nz + B - 1) / B;
    return (long long)d.nbx * d.nby * d.nbz < (1ll << 31);
}

// in-block coordinates run over [-1, B + 1]: -1 is the neighbour block below, B and B + 1 the one above
template <int B>
struct SmcBlock {
    static constexpr int H = B + 1, T = B * B * B;
    const float* u;
    const float* hu;          // LDS: the (B+1)^3 halo of values, [a][b][c], a, b, c in [0, B]
    const int* nbr;           // LDS: slots of the 27 neighbour blocks, [dx+1][dy+1][dz+1]; -1: inactive or beyond the block grid
    int gi, gj, gk;           // lattice coordinates of the block's first point
    int nx, ny, nz;

    static __device__ inline int side(int a) { return a < 0 ? 0 : (a >= B ? 2 : 1); }
    __device__ inline int slot_of(int a, int b, int c) const { return nbr[(side(a) * 3 + side(b)) * 3 + side(c)]; }
    // the point exists and its block is active
    __device__ inline bool act(int a, int b, int c) const {
        const int i = gi + a, j = gj + b, k = gk + c;
        return i >= 0 && j >= 0 && k >= 0 && i < nx && j < ny && k < nz && slot_of(a, b, c) >= 0;
    }
    static __device__ inline long long row(int s, int a, int b, int c) {
        return (long long)s * T + (((a + B) % B) * B + ((b + B) % B)) * B + ((c + B) % B);
    }
    // value of an active point
    __device__ inline float val(int a, int b, int c) const {
        if (a >= 0 && b >= 0 && c >= 0 && a <= B && b <= B && c <= B) return hu[(a * H + b) * H + c];
        return u[row(slot_of(a, b, c), a, b, c)];
    }
    // bits 0..2 below `naxes`: the +x / +y / +z edges of the active point (a, b, c) have an active far end and straddle iso
    __device__ inline int owned(int a, int b, int c, float iso, int naxes) const {
        const bool in0 = val(a, b, c) < iso;
        int m = 0;
        if (naxes > 0 && act(a + 1, b, c) && ((val(a + 1, b, c) < iso) != in0)) m |= 1;
        if (naxes > 1 && act(a, b + 1, c) && ((val(a, b + 1, c) < iso) != in0)) m |= 2;
        if (naxes > 2 && act(a, b, c + 1) && ((val(a, b, c + 1) < iso) != in0)) m |= 4;
        return m;
    }
    // all eight corners of the cell whose min corner is (a, b, c) are active
    __device__ inline bool processed(int a, int b, int c) const {
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 8; ++e) ok = ok && act(a + (e & 1), b + ((e >> 1) & 1), c + (e >> 2));
        return ok;
    }
    __device__ inline bool cell_in_grid(int a, int b, int c) const {
        const int i = gi + a, j = gj + b, k = gk + c;
        return i >= 0 && j >= 0 && k >= 0 && i + 1 < nx && j + 1 < ny && k + 1 < nz;
    }
    // cube index of a processed cell (corner numbering: mc_tables.h), -1 when the cell is not processed
    __device__ inline int cube(int a, int b, int c, float iso) const {
        if (!processed(a, b, c)) return -1;
        int q = 0;
        q |= (val(a, b, c) < iso) ? 1 : 0;
        q |= (val(a + 1, b, c) < iso) ? 2 : 0;
        q |= (val(a + 1, b + 1, c) < iso) ? 4 : 0;
        q |= (val(a, b + 1, c) < iso) ? 8 : 0;
        q |= (val(a, b, c + 1) < iso) ? 16 : 0;
        q |= (val(a + 1, b, c + 1) < iso) ? 32 : 0;
        q |= (val(a + 1, b + 1, c + 1) < iso) ? 64 : 0;
        q |= (val(a, b + 1, c + 1) < iso) ? 128 : 0;
        return q;
    }
    // the owned straddling edge of axis ax from (a, b, c) has an in-grid incident cell that is not processed
    __device__ inline bool open_edge(int a, int b, int c, int ax) const {
        bool open = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o1 = e & 1, o2 = e >> 1;
            const int ca = a - (ax == 0 ? 0 : o1), cb = b - (ax == 1 ? 0 : (ax == 0 ? o1 : o2)), cc = c - (ax == 2 ? 0 : o2);
            open = open || (cell_in_grid(ca, cb, cc) && !processed(ca, cb, cc));
        }
        return open;
    }
};

// fills the LDS tables of the workgroup's block and returns its view; every thread of the workgroup must call it
template <int B>
static __device__ inline SmcBlock<B> smc_load(const float* __restrict__ u, const int* __restrict__ slot, const int* __restrict__ blocks,
                                              SmcDims d, float* hu, int* nbr) {
    constexpr int H = B + 1, T = B * B * B;
    const int blk = blocks[blockIdx.x];
    const int bi = blk / (d.nby * d.nbz), bj = (blk / d.nbz) % d.nby, bk = blk % d.nbz;
    for (int e = threadIdx.x; e < 27; e += T) {
        const int x = bi + e / 9 - 1, y = bj + (e / 3) % 3 - 1, z = bk + e % 3 - 1;
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < d.nbx && y < d.nby && z < d.nbz;
        nbr[e] = in ? slot[((long long)x * d.nby + y) * d.nbz + z] : -1;
    }
    __syncthreads();
    SmcBlock<B> g;
    g.u = u; g.hu = hu; g.nbr = nbr;
    g.gi = B * bi; g.gj = B * bj; g.gk = B * bk;
    g.nx = d.nx; g.ny = d.ny; g.nz = d.nz;
    for (int e = threadIdx.x; e < H * H * H; e += T) {
        const int a = e / (H * H), b = (e / H) % H, c = e % H;
        hu[e] = g.act(a, b, c) ? u[SmcBlock<B>::row(g.slot_of(a, b, c), a, b, c)] : 0.f;
    }
    __syncthreads();
    return g;
}

static __device__ inline int smc_ntri_of(const signed char* row) {
    int n = 0;
    while (n < 5 && row[3 * n] >= 0) ++n;
    return n;
}

// owner corner offset (bits 0/1/2: +1 in i/j/k) and axis of each of the 12 cube edges (as in mcubes.hip)
__constant__ unsigned char smc_edge_owner[12] = {0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 3, 2};
__constant__ unsigned char smc_edge_axis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

template <int B>
__global__ __launch_bounds__(B* B* B) void smc_count_kernel(const float* __restrict__ u, const int* __restrict__ slot,
                                                           const int* __restrict__ blocks, SmcDims d, float iso, int* __restrict__ cnt) {
    constexpr int T = B * B * B, NW = T / 64;
    __shared__ float hu[(B + 1) * (B + 1) * (B + 1)];
    __shared__ int nbr[27];
    __shared__ int lds[NW];
    const SmcBlock<B> g = smc_load<B>(u, slot, blocks, d, hu, nbr);
    const int a = threadIdx.x / (B * B), b = (threadIdx.x / B) % B, c = threadIdx.x % B;
    int nv = 0, nt = 0, no = 0;
    if (g.act(a, b, c)) {
        const int m = g.owned(a, b, c, iso, 3);
        nv = __popc(m);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            if ((m >> ax) & 1) no += g.open_edge(a, b, c, ax) ? 1 : 0;
        const int q = g.cube(a, b, c, iso);
        nt = q >= 0 ? smc_ntri_of(nu_mc_tri_table[q]) : 0;        // the 4 KB table is read in place: most cells stop at its first byte
    }
    int tv, tt, to;
    smc_block_excl<int, NW>(nv, lds, &tv);
    smc_block_excl<int, NW>(nt, lds, &tt);
    smc_block_excl<int, NW>(no, lds, &to);
    if (threadIdx.x == 0) {
        cnt[3 * (long long)blockIdx.x] = tv;
        cnt[3 * (long long)blockIdx.x + 1] = tt;
        cnt[3 * (long long)blockIdx.x + 2] = to;
    }
}

template <int B>
__global__ __launch_bounds__(B* B* B) void smc_vertex_kernel(const float* __restrict__ u, const int* __restrict__ slot,
                                                            const int* __restrict__ blocks, SmcDims d, float iso,
                                                            const int* __restrict__ cnt, const long long* __restrict__ off,
                                                            float* __restrict__ V, int* __restrict__ first_vid) {
#pragma clang fp contract(off)
    constexpr int T = B * B * B, NW = T / 64;
    __shared__ float hu[(B + 1) * (B + 1) * (B + 1)];
    __shared__ int nbr[27];
    __shared__ int lds[NW];
    if (cnt[3 * (long long)blockIdx.x] == 0) return;                  // workgroup-uniform
    const SmcBlock<B> g = smc_load<B>(u, slot, blocks, d, hu, nbr);
    const int a = threadIdx.x / (B * B), b = (threadIdx.x / B) % B, c = threadIdx.x % B;
    const int m = g.act(a, b, c) ? g.owned(a, b, c, iso, 3) : 0;
    int tot;
    const long long base = off[3 * (long long)blockIdx.x] + smc_block_excl<int, NW>(__popc(m), lds, &tot);
    if (m == 0) return;
    first_vid[(long long)blockIdx.x * T + threadIdx.x] = (int)base;
    const float ua = g.val(a, b, c);
    long long v = base;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!(m & (1 << ax))) continue;
        const float ub = g.val(a + (ax == 0), b + (ax == 1), c + (ax == 2));
        const float t = (iso - ua) / (ub - ua);
        float x = (float)(g.gi + a), y = (float)(g.gj + b), z = (float)(g.gk + c);
        if (ax == 0) x = x + t;
        else if (ax == 1) y = y + t;
        else z = z + t;
        V[3 * v + 0] = x;
        V[3 * v + 1] = y;
        V[3 * v + 2] = z;
        ++v;
    }
}

template <int B>
__global__ __launch_bounds__(B* B* B) void smc_triangle_kernel(const float* __restrict__ u, const int* __restrict__ slot,
                                                              const int* __restrict__ blocks, SmcDims d, float iso,
                                                              const int* __restrict__ cnt, const long long* __restrict__ off,
                                                              const int* __restrict__ first_vid, int* __restrict__ F) {
    constexpr int T = B * B * B, NW = T / 64;
    __shared__ float hu[(B + 1) * (B + 1) * (B + 1)];
    __shared__ int nbr[27];
    __shared__ int lds[NW];
    if (cnt[3 * (long long)blockIdx.x + 1] == 0) return;              // workgroup-uniform
    const SmcBlock<B> g = smc_load<B>(u, slot, blocks, d, hu, nbr);
    const int a = threadIdx.x / (B * B), b = (threadIdx.x / B) % B, c = threadIdx.x % B;
    const int q = g.act(a, b, c) ? g.cube(a, b, c, iso) : -1;
    const signed char* tri = q >= 0 ? nu_mc_tri_table[q] : nullptr;    // read in place, as the count pass does
    const int nt = q >= 0 ? smc_ntri_of(tri) : 0;
    int tot;
    const long long base = off[3 * (long long)blockIdx.x + 1] + smc_block_excl<int, NW>(nt, lds, &tot);
    for (int s = 0; s < 3 * nt; ++s) {
        const int e = tri[s];
        const int ow = smc_edge_owner[e], ax = smc_edge_axis[e];
        const int oa = a + (ow & 1), ob = b + ((ow >> 1) & 1), oc = c + ((ow >> 2) & 1);
        // rank of this axis among the edges the owner holds: its straddling edges of lower axis come first
        const int rank = ax ? __popc(g.owned(oa, ob, oc, iso, ax)) : 0;
        F[3 * base + s] = first_vid[SmcBlock<B>::row(g.slot_of(oa, ob, oc), oa, ob, oc)] + rank;
    }
}

static bool smc_grid_args(const float* u, const int* slot, const int* blocks, int nslots) {
    return u != nullptr && slot != nullptr && blocks != nullptr && nslots > 0;
}

extern "C" int nu_smc_count(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block, float iso,
                            void* workspace, long long workspace_bytes, hipStream_t stream) {
    SmcDims d;
    if (!smc_grid_args(u, slot, blocks, nslots) || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    SmcWs w;
    if (!smc_ws(workspace, workspace_bytes, nslots, w)) return NU_ERR_WORKSPACE;
    if (block == 4) hipLaunchKernelGGL(smc_count_kernel<4>, dim3((unsigned)nslots), dim3(64), 0, stream, u, slot, blocks, d, iso, w.cnt);
    else hipLaunchKernelGGL(smc_count_kernel<8>, dim3((unsigned)nslots), dim3(512), 0, stream, u, slot, blocks, d, iso, w.cnt);
    return nu_launch_status();
}

extern "C" int nu_smc_scan(int nslots, void* workspace, long long workspace_bytes, long long* totals, hipStream_t stream) {
    SmcWs w;
    if (nslots <= 0) return NU_ERR_ARG;
    if (!smc_ws(workspace, workspace_bytes, nslots, w)) return NU_ERR_WORKSPACE;
    hipLaunchKernelGGL(smc_scan_reduce_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, stream, w.cnt, w.n, w.bsum);
    hipLaunchKernelGGL(smc_scan_top_kernel, dim3(1), dim3(256), 0, stream, w.bsum, w.nchunk, w.off, w.n);
    hipLaunchKernelGGL(smc_scan_down_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, stream, w.cnt, w.n, w.bsum, w.off);
    const int rc = nu_launch_status();
    if (rc != NU_OK) return rc;
    if (totals != nullptr && hipMemcpyAsync(totals, w.off + 3 * w.n, 3 * sizeof(long long), hipMemcpyDeviceToDevice, stream) != hipSuccess)
        return NU_ERR_LAUNCH;
    return NU_OK;
}

extern "C" int nu_smc_write_vertices(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block,
                                     float iso, const void* workspace, long long workspace_bytes, float* V, int* first_vid,
                                     hipStream_t stream) {
    SmcDims d;
    if (!smc_grid_args(u, slot, blocks, nslots) || V == nullptr || first_vid == nullptr || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    SmcWs w;
    if (!smc_ws(const_cast<void*>(workspace), workspace_bytes, nslots, w)) return NU_ERR_WORKSPACE;
    if (block == 4)
        hipLaunchKernelGGL(smc_vertex_kernel<4>, dim3((unsigned)nslots), dim3(64), 0, stream, u, slot, blocks, d, iso, w.cnt, w.off, V, first_vid);
    else
        hipLaunchKernelGGL(smc_vertex_kernel<8>, dim3((unsigned)nslots), dim3(512), 0, stream, u, slot, blocks, d, iso, w.cnt, w.off, V, first_vid);
    return nu_launch_status();
}

extern "C" int nu_smc_write_triangles(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block,
                                      float iso, const void* workspace, long long workspace_bytes, const int* first_vid, int* F,
                                      hipStream_t stream) {
    SmcDims d;
    if (!smc_grid_args(u, slot, blocks, nslots) || F == nullptr || first_vid == nullptr || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    SmcWs w;
    if (!smc_ws(const_cast<void*>(workspace), workspace_bytes, nslots, w)) return NU_ERR_WORKSPACE;
    if (block == 4)
        hipLaunchKernelGGL(smc_triangle_kernel<4>, dim3((unsigned)nslots), dim3(64), 0, stream, u, slot, blocks, d, iso, w.cnt, w.off, first_vid, F);
    else
        hipLaunchKernelGGL(smc_triangle_kernel<8>, dim3((unsigned)nslots), dim3(512), 0, stream, u, slot, blocks, d, iso, w.cnt, w.off, first_vid, F);
    return nu_launch_status();
}

// ------------------------------------------------------------------------------------------------ which blocks: regions and the rule
// the inside test of mcubes.hip (torch.norm's arithmetic for a 3-element row): NOT ((x^2 + z^2) + y^2 >= 1), every operation rounded
static __device__ inline bool smc_inside(float x, float y, float z) {
#pragma clang fp contract(off)
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = (xx + zz) + yy;
    return !(s >= 1.0f);
}

// flags: 0 = no point of the region can lie inside the unit ball (never probed), 1 = wholly inside, 2 = rim
__global__ __launch_bounds__(256) void smc_regions_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                                         SmcDims d, int B, int* __restrict__ flags, float* __restrict__ probe,
                                                         float* __restrict__ radius) {
#pragma clang fp contract(off)
    const long long nblk = (long long)d.nbx * d.nby * d.nbz;
    const long long blk = (long long)blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblk) return;
    const int b3[3] = {(int)(blk / ((long long)d.nby * d.nbz)), (int)((blk / d.nbz) % d.nby), (int)(blk % d.nbz)};
    const int n3[3] = {d.nx, d.ny, d.nz};
    const float* A3[3] = {X, Y, Z};
    float lo[3], hi[3];
    double c[3], near2 = 0.0, diag2 = 0.0, n2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int l = max(B * b3[a] - 1, 0), h = min(B * b3[a] + B, n3[a] - 1);
        lo[a] = A3[a][l];
        hi[a] = A3[a][h];
        const double x0 = lo[a], x1 = hi[a];
        c[a] = 0.5 * (x0 + x1);
        const double e = 0.5 * (x1 - x0);
        const double nr = x0 > 0.0 ? x0 : (x1 < 0.0 ? x1 : 0.0);       // the box's point nearest the origin
        near2 = near2 + nr * nr;
        diag2 = diag2 + e * e;
        n2 = n2 + c[a] * c[a];
    }
    float p[3] = {0.f, 0.f, 0.f}, r = 0.f;
    int flag = 0;
    if (!(near2 > 1.001)) {                                               // conservative: over-approximating costs only a probe
        bool all_in = true;
#pragma unroll
        for (int e = 0; e < 8; ++e) all_in = all_in && smc_inside((e & 1) ? hi[0] : lo[0], (e & 2) ? hi[1] : lo[1], (e & 4) ? hi[2] : lo[2]);
        flag = all_in ? 1 : 2;
        const double s = n2 > 0.999 * 0.999 ? 0.999 / sqrt(n2) : 1.0;
        double dist2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = (float)(c[a] * s);
            const double dd = c[a] - (double)p[a];
            dist2 = dist2 + dd * dd;
        }
        r = (float)((sqrt(diag2) + sqrt(dist2)) * 1.000001);             // the margin covers the rounding of p and r to fp32
    }
    flags[blk] = flag;
    probe[3 * blk + 0] = p[0];
    probe[3 * blk + 1] = p[1];
    probe[3 * blk + 2] = p[2];
    radius[blk] = r;
}

// f: the field at the probes; g (or null): the inner field of the stage-2 composite, whose value is g where f < 0 and 1 elsewhere.
// The rule looks for the level set at iso: a single field is tested as f - iso; of the composite, f still decides the SIGN (against 0)
// and g - iso the level.  The one-sided rim form needs outside_val > iso (and the composite iso < 1): the caller checks that.
// Every comparison is written so that a NaN probe value activates the block.
__global__ __launch_bounds__(256) void smc_activate_kernel(const int* __restrict__ flags, const float* __restrict__ radius,
                                                          const int* __restrict__ probe_blocks, int nprobe, const float* __restrict__ f,
                                                          const float* __restrict__ g, float lipschitz, float iso, int* __restrict__ active) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nprobe) return;
    const int blk = probe_blocks[i];
    const bool rim = flags[blk] != 1;
    const float lr = lipschitz * radius[blk];
    const float s = g == nullptr ? f[i] - iso : f[i];
    bool on;
    if (isinf(lipschitz)) on = true;
    else if (g == nullptr) on = rim ? !(s > lr) : !(fabsf(s) > lr);
    else {
        const float gg = g[i] - iso;
        const bool g_zero = rim ? !(gg > lr) : !(fabsf(gg) > lr);
        on = !(s > lr) && (g_zero || (!(fabsf(s) > lr) && !(gg > lr)));
    }
    active[blk] = on ? 1 : 0;
}

// x rows of the block points r0 .. r0 + n (r = slot B^3 + t); indices beyond the grid are clamped
__global__ __launch_bounds__(256) void smc_rows_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                                      SmcDims d, int B, const int* __restrict__ blocks, long long r0, long long n,
                                                      float* __restrict__ rows) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long long r = r0 + e;
    const int T = B * B * B;
    const int blk = blocks[r / T], t = (int)(r % T);
    const int bi = blk / (d.nby * d.nbz), bj = (blk / d.nbz) % d.nby, bk = blk % d.nbz;
    const int i = min(B * bi + t / (B * B), d.nx - 1), j = min(B * bj + (t / B) % B, d.ny - 1), k = min(B * bk + t % B, d.nz - 1);
    rows[3 * e + 0] = X[i];
    rows[3 * e + 1] = Y[j];
    rows[3 * e + 2] = Z[k];
}

// u[r] = outside_val at the points that fail the inside test (and at the padding beyond the grid edge)
__global__ __launch_bounds__(256) void smc_finish_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z,
                                                        SmcDims d, int B, const int* __restrict__ blocks, long long n, float outside_val,
                                                        float* __restrict__ u) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int T = B * B * B;
    const int blk = blocks[r / T], t = (int)(r % T);
    const int bi = blk / (d.nby * d.nbz), bj = (blk / d.nbz) % d.nby, bk = blk % d.nbz;
    const int i = B * bi + t / (B * B), j = B * bj + (t / B) % B, k = B * bk + t % B;
    const bool keep = i < d.nx && j < d.ny && k < d.nz && smc_inside(X[i], Y[j], Z[k]);
    if (!keep) u[r] = outside_val;
}

static bool smc_axes_ok(const float* X, const float* Y, const float* Z) { return X != nullptr && Y != nullptr && Z != nullptr; }

extern "C" int nu_smc_regions(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, int* flags, float* probe,
                              float* radius, hipStream_t stream) {
    SmcDims d;
    if (!smc_axes_ok(X, Y, Z) || flags == nullptr || probe == nullptr || radius == nullptr || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    const long long nblk = (long long)d.nbx * d.nby * d.nbz;
    hipLaunchKernelGGL(smc_regions_kernel, dim3((unsigned)nu_cdivl(nblk, 256)), dim3(256), 0, stream, X, Y, Z, d, block, flags, probe, radius);
    return nu_launch_status();
}

extern "C" int nu_smc_activate(const int* flags, const float* radius, const int* probe_blocks, int nprobe, const float* f, const float* g,
                               float lipschitz, float iso, int* active, hipStream_t stream) {
    if (flags == nullptr || radius == nullptr || probe_blocks == nullptr || f == nullptr || active == nullptr || nprobe < 0 ||
        !(lipschitz > 0.f) || !(iso == iso))
        return NU_ERR_ARG;
    if (nprobe == 0) return NU_OK;
    hipLaunchKernelGGL(smc_activate_kernel, dim3((unsigned)nu_cdiv(nprobe, 256)), dim3(256), 0, stream, flags, radius, probe_blocks, nprobe,
                       f, g, lipschitz, iso, active);
    return nu_launch_status();
}

extern "C" int nu_smc_block_rows(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, const int* blocks,
                                 int nslots, long long r0, long long n, float* rows, hipStream_t stream) {
    SmcDims d;
    if (!smc_axes_ok(X, Y, Z) || blocks == nullptr || rows == nullptr || nslots <= 0 || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    const long long total = (long long)nslots * block * block * block;
    if (r0 < 0 || n < 0 || r0 + n > total) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    hipLaunchKernelGGL(smc_rows_kernel, dim3((unsigned)nu_cdivl(n, 256)), dim3(256), 0, stream, X, Y, Z, d, block, blocks, r0, n, rows);
    return nu_launch_status();
}

extern "C" int nu_smc_finish(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, const int* blocks, int nslots,
                             float outside_val, float* u, hipStream_t stream) {
    SmcDims d;
    if (!smc_axes_ok(X, Y, Z) || blocks == nullptr || u == nullptr || nslots <= 0 || !smc_dims(nx, ny, nz, block, d)) return NU_ERR_ARG;
    const long long total = (long long)nslots * block * block * block;
    hipLaunchKernelGGL(smc_finish_kernel, dim3((unsigned)nu_cdivl(total, 256)), dim3(256), 0, stream, X, Y, Z, d, block, blocks, total,
                       outside_val, u);
    return nu_launch_status();
}
