// metrics.hip -- validation metrics on uint8 images (network/metrics.py of the reference): quantisation, PSNR's squared error and
// the uniform-window SSIM of skimage.metrics.structural_similarity(..., win_size=win, channel_axis=2, data_range=255) (gfx950).
//
// Images are [n, h, w, c] uint8, channel-interleaved.  A row is w * c bytes and a window walks it with a stride of c bytes, so the
// kernels never look at pixels: "byte column" j = x * c + channel, and the horizontal window sum at j is the sum of bytes j + t * c.
//
// Everything up to the last step is integer and exact:
//   - the five window sums (x, y, x^2, y^2, x y) are int32: win <= 15 gives at most 225 * 255^2 < 2^24;
//   - the covariance numerators NP * sum(x y) - sum(x) sum(y) (NP = win^2) are int64;
//   - S is then a few dozen fp64 operations per window, without contraction, in the order tests/metrics_oracle.py uses.
// The mean of S is reduced in a fixed order (per wave, per block, then one block per image over the per-block partial sums in the
// workspace): no floating-point atomics, the same bits on every run and for every batch size.
//
// SSIM keeps the windows that lie wholly inside the image (skimage crops its map by (win - 1) / 2 on every side before taking
// the mean), so there is no border mode: (h - win + 1) * (w - win + 1) windows per channel and nothing else.
#include "nu_common.h"

#define NU_SS_TX 64                                    // SSIM: output byte columns per block, one per lane
#define NU_SS_TY 16                                    // SSIM: output rows per block, four per wave
#define NU_SS_WMAX 15                                  // largest window: keeps the window sums below 2^24
#define NU_SS_ROWS (NU_SS_TY + NU_SS_WMAX - 1)         // staged rows: tile + halo
#define NU_SS_LDW ((NU_SS_TX + (NU_SS_WMAX - 1) * 3 + 3) / 4 + 1)   // words per staged row (c <= 3): 27 used, 28 allocated
#define NU_SQ_WORDS 16                                 // squared error: 32-bit words per thread

// A byte array whose first element sits `off` (0..3) bytes after the 4-byte aligned address `base`; `end` = off + its length.
// Reading the aligned words that hold the first and the last element touches no other allocation.
struct NuByteSpan {
    const unsigned char* base;
    long long off, end;
};
static NuByteSpan nu_byte_span(const unsigned char* p, long long len) {
    const long long mis = (long long)((uintptr_t)p & 3);
    return NuByteSpan{p - mis, mis, mis + len};
}
// the aligned word at byte b of the span (b % 4 == 0), bytes at or past the end read as 0
static __device__ inline unsigned nu_span_word(const NuByteSpan& s, long long b) {
    if (b + 3 < s.end) return *(const unsigned*)(s.base + b);
    unsigned v = 0;
    for (int j = 0; j < 4; ++j)
        if (b + j < s.end) v |= (unsigned)s.base[b + j] << (8 * j);
    return v;
}
// elements [pos, pos + 4) of the span as one little-endian word: one aligned 32-bit load, two when pos is not a multiple of 4
static __device__ inline unsigned nu_span_load4(const NuByteSpan& s, long long pos) {
    const long long p = s.off + pos, b = p & ~3LL;
    const int sh = (int)(p & 3) * 8;
    const unsigned lo = nu_span_word(s, b);
    if (sh == 0) return lo;
    return (lo >> sh) | (nu_span_word(s, b + 4) << (32 - sh));
}

// color_map_backward (utils/base_utils.py:501-504): one fp32 multiply, clamp, truncate.  fmaxf(NaN, 0) = 0.
static __device__ inline unsigned nu_quant(float x) { return (unsigned)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

__global__ __launch_bounds__(256) void img_quantize_kernel(const float* __restrict__ x, long long count, unsigned char* __restrict__ out,
                                                           int vec) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    if (vec && i + 3 < count) {                     // x 16-byte and out 4-byte aligned (checked on the host)
        const f32x4 v = *(const f32x4*)(x + i);
        *(unsigned*)(out + i) = nu_quant(v[0]) | nu_quant(v[1]) << 8 | nu_quant(v[2]) << 16 | nu_quant(v[3]) << 24;
    } else {
        for (long long e = i; e < min(i + 4, count); ++e) out[e] = (unsigned char)nu_quant(x[e]);
    }
}

// one block per 256 * NU_SQ_WORDS words of one image: ssd[image] += sum (a - b)^2, one 64-bit integer atomic per block
__global__ __launch_bounds__(256) void img_sqdiff_kernel(NuByteSpan a, NuByteSpan b, long long per_image, int bpi,
                                                         unsigned long long* __restrict__ ssd) {
    __shared__ unsigned wsum[4];
    const int img = blockIdx.x / bpi, blk = blockIdx.x - img * bpi;
    const long long ibase = (long long)img * per_image;
    const int tid = threadIdx.x;
    unsigned acc = 0;                               // <= NU_SQ_WORDS * 4 * 255^2 per thread, * 64 per wave: below 2^32
    for (int i = 0; i < NU_SQ_WORDS; ++i) {
        const long long p = ((long long)blk * NU_SQ_WORDS + i) * 1024 + tid * 4;     // byte of the image; consecutive lanes, consecutive words
        if (p >= per_image) break;
        unsigned va = nu_span_load4(a, ibase + p), vb = nu_span_load4(b, ibase + p);
        const int nb = (int)min(4LL, per_image - p);                                  // the next image starts here: leave its bytes out
        for (int j = 0; j < nb; ++j) {
            const int d = (int)((va >> (8 * j)) & 255u) - (int)((vb >> (8 * j)) & 255u);
            acc += (unsigned)(d * d);
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long s = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (s) atomicAdd(&ssd[img], s);
    }
}

// S of one window from its five exact sums.  No contraction: the operations and their order are those of the numpy oracle.
static __device__ inline double nu_ssim_window(int sx, int sy, int sxx, int syy, int sxy, int np, double c1, double c2) {
#pragma clang fp contract(off)
    const long long nxx = (long long)np * sxx - (long long)sx * sx;
    const long long nyy = (long long)np * syy - (long long)sy * sy;
    const long long nxy = (long long)np * sxy - (long long)sx * sy;
    const double den = (double)np * (double)(np - 1);       // cov_norm / NP^2 = 1 / (NP (NP - 1))
    const double ux = (double)sx / (double)np, uy = (double)sy / (double)np;
    const double vx = (double)nxx / den, vy = (double)nyy / den, vxy = (double)nxy / den;
    const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
    const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
    return (a1 * a2) / (b1 * b2);
}

// one block per NU_SS_TY rows x NU_SS_TX byte columns of windows of one image pair
__global__ __launch_bounds__(256) void img_ssim_kernel(NuByteSpan a, NuByteSpan b, int h, int w, int c, int win, double c1, double c2,
                                                       double* __restrict__ part, double* __restrict__ smap) {
    __shared__ unsigned ta[NU_SS_ROWS][NU_SS_LDW], tb[NU_SS_ROWS][NU_SS_LDW];
    __shared__ int rs[5][NU_SS_ROWS][NU_SS_TX];     // row sums; lane = column in both passes: bank = lane mod 32, conflict-free
    __shared__ double wsum[4];
    const int oh = h - win + 1, owc = (w - win + 1) * c, wc = w * c;
    const int tx = nu_cdiv(owc, NU_SS_TX), ty = nu_cdiv(oh, NU_SS_TY);
    const int img = blockIdx.x / (tx * ty), t = blockIdx.x - img * tx * ty;
    const int j0 = (t % tx) * NU_SS_TX, y0 = (t / tx) * NU_SS_TY;
    const int ncol = min(NU_SS_TX, owc - j0), nout = min(NU_SS_TY, oh - y0);
    const int nrows = nout + win - 1;                               // staged rows y0 .. y0 + nrows - 1 <= h - 1
    const int nwords = (ncol + (win - 1) * c + 3) / 4;              // bytes j0 .. j0 + ncol - 1 + (win - 1) c <= w c - 1, rounded up
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nrows * nwords; i += 256) {
        const int r = i / nwords, k = i - r * nwords;
        const long long pos = ((long long)img * h + y0 + r) * wc + j0 + 4 * k;
        ta[r][k] = nu_span_load4(a, pos);
        tb[r][k] = nu_span_load4(b, pos);
    }
    __syncthreads();
    // row pass: one wave per staged row; four neighbouring lanes read the same LDS word (a broadcast)
    for (int r = wave; r < nrows; r += 4) {
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        if (lane < ncol) {
            const unsigned char *ra = (const unsigned char*)ta[r] + lane, *rb = (const unsigned char*)tb[r] + lane;
            for (int q = 0; q < win; ++q) {
                const int x = ra[q * c], y = rb[q * c];
                sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
        }
        rs[0][r][lane] = sx; rs[1][r][lane] = sy; rs[2][r][lane] = sxx; rs[3][r][lane] = syy; rs[4][r][lane] = sxy;
    }
    __syncthreads();
    // column pass: each wave slides the window down its four output rows (integer sums: adding and removing a row is exact)
    double acc = 0.0;
    const int r0 = wave * (NU_SS_TY / 4);
    if (lane < ncol && r0 < nout) {
        int s[5];
        for (int k = 0; k < 5; ++k) {
            s[k] = 0;
            for (int q = 0; q < win; ++q) s[k] += rs[k][r0 + q][lane];
        }
        const long long obase = ((long long)img * oh + y0) * owc + j0 + lane;
        for (int q = 0; q < NU_SS_TY / 4; ++q) {
            const int r = r0 + q;
            const double v = nu_ssim_window(s[0], s[1], s[2], s[3], s[4], win * win, c1, c2);
            acc += v;
            if (smap) smap[obase + (long long)r * owc] = v;
            if (r + 1 >= nout) break;
            for (int k = 0; k < 5; ++k) s[k] += rs[k][r + win][lane] - rs[k][r][lane];
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one block per image: the per-block partial sums in a fixed order, divided by the number of windows
__global__ __launch_bounds__(256) void img_ssim_mean_kernel(const double* __restrict__ part, int tiles, double count, double* __restrict__ mssim) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    const double* p = part + (long long)blockIdx.x * tiles;
    double acc = 0.0;
    for (int i = tid; i < tiles; i += 256) acc += p[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) mssim[blockIdx.x] = (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / count;
}

extern "C" int nu_img_quantize(const float* x, long long count, unsigned char* out, hipStream_t stream) {
    if (count < 0 || (count > 0 && (!x || !out))) return NU_ERR_ARG;
    if (count == 0) return NU_OK;
    const long long blocks = nu_cdivl(count, 1024);
    if (blocks > 0x7fffffffLL) return NU_ERR_ARG;
    const int vec = ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0;
    hipLaunchKernelGGL(img_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, count, out, vec);
    return nu_launch_status();
}

extern "C" int nu_img_sqdiff(const unsigned char* a, const unsigned char* b, int n, long long per_image, long long* ssd,
                             hipStream_t stream) {
    if (n < 0 || per_image < 0 || (n > 0 && (!ssd || (per_image > 0 && (!a || !b))))) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    if (hipMemsetAsync(ssd, 0, (size_t)n * 8, stream) != hipSuccess) return NU_ERR_LAUNCH;
    if (per_image == 0) return NU_OK;
    const long long bpi = nu_cdivl(per_image, 1024LL * NU_SQ_WORDS);
    if (bpi * n > 0x7fffffffLL) return NU_ERR_ARG;                 // the caller chunks over images
    hipLaunchKernelGGL(img_sqdiff_kernel, dim3((unsigned)(bpi * n)), dim3(256), 0, stream, nu_byte_span(a, n * per_image),
                       nu_byte_span(b, n * per_image), per_image, (int)bpi, (unsigned long long*)ssd);
    return nu_launch_status();
}

static bool nu_ssim_shape_ok(int n, int h, int w, int c) { return n >= 0 && h > 0 && w > 0 && (c == 1 || c == 3); }
static long long nu_ssim_tiles(int h, int w, int c, int win) {
    return (long long)nu_cdiv(h - win + 1, NU_SS_TY) * nu_cdivl((long long)(w - win + 1) * c, NU_SS_TX);
}

// sized for the smallest window (3), which has the most tiles: the query does not know win
extern "C" long long nu_img_ssim_workspace_bytes(int n, int h, int w, int c) {
    if (!nu_ssim_shape_ok(n, h, w, c) || h < 3 || w < 3) return 0;
    return (long long)n * nu_ssim_tiles(h, w, c, 3) * 8;
}

extern "C" int nu_img_ssim(const unsigned char* a, const unsigned char* b, int n, int h, int w, int c, int win, double* mssim,
                           double* smap, void* work, long long work_bytes, hipStream_t stream) {
    if (!nu_ssim_shape_ok(n, h, w, c) || win < 3 || win > NU_SS_WMAX || win % 2 == 0 || h < win || w < win) return NU_ERR_ARG;
    if ((long long)w * c > 0x7fffffffLL) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    if (!a || !b || !mssim) return NU_ERR_ARG;
    if (!work || work_bytes < nu_img_ssim_workspace_bytes(n, h, w, c)) return NU_ERR_WORKSPACE;
    const long long tiles = nu_ssim_tiles(h, w, c, win);
    if (tiles * n > 0x7fffffffLL) return NU_ERR_ARG;               // the caller chunks over images
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    const long long total = (long long)n * h * w * c;
    double* part = (double*)work;
    hipLaunchKernelGGL(img_ssim_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, stream, nu_byte_span(a, total), nu_byte_span(b, total),
                       h, w, c, win, c1, c2, part, smap);
    const double count = (double)(h - win + 1) * (double)(w - win + 1) * (double)c;
    hipLaunchKernelGGL(img_ssim_mean_kernel, dim3((unsigned)n), dim3(256), 0, stream, part, (int)tiles, count, mssim);
    return nu_launch_status();
}
