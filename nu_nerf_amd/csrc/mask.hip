// mask.hip -- erosion of the stage-2 object masks (mask_erosion.py), batched over images (gfx950).
//
// Per image m (uint8 [h, w]) and box size k >= 1, anchor a = k / 2 (OpenCV's default):
//   eroded[y, x] = min m[y + dy, x + dx] over dy, dx in [-a, k - 1 - a], positions outside the image left out
//   out[y, x]    = eroded[y, x] + (max(m) - m[y, x])              (no wrap: eroded <= m)
// mask_erosion.py:33 calls cv.erode(img, kernel, cv.BORDER_REFLECT); the third positional parameter of cv.erode is `dst`, not
// `borderType`, so the default border applies: BORDER_CONSTANT with morphologyDefaultBorderValue(), which for erosion is the
// largest value of the type (255) -- the same as leaving outside positions out of the minimum.
//
// Min is exact in any order, so the box is two separable passes: rows (into a workspace image, with the per-image maximum reduced
// on the device), then columns (composed with the maximum and the original).  Each pass stages its tile plus the window halo in
// LDS with aligned 32-bit loads, once per pixel; a halo that does not fit is walked in further LDS chunks.
#include "nu_common.h"

#define NU_EROW_T 1024          // row pass: outputs per block (one row segment)
#define NU_EROW_CAP 4096        // row pass: LDS bytes per chunk (tile + halo)
#define NU_ECOL_TC 256          // column pass: columns per block
#define NU_ECOL_TR 32           // column pass: output rows per block
#define NU_ECOL_CAPR 64         // column pass: LDS rows per chunk

// bytes [g, g + len) of src (total bytes in all) -> dst[0, len): aligned 32-bit loads, bytewise only for a final partial word
static __device__ inline void nu_fill_bytes(const unsigned char* __restrict__ src, long long total, long long g, int len,
                                            unsigned char* dst, int tid, int nthr) {
    const long long w0 = g >> 2, w1 = (g + len - 1) >> 2;
    for (long long wi = w0 + tid; wi <= w1; wi += nthr) {
        const long long b = wi * 4;
        unsigned v = 0;
        if (b + 3 < total) {
            v = *(const unsigned*)(src + b);
        } else {
            for (int j = 0; j < 4; ++j)
                if (b + j < total) v |= (unsigned)src[b + j] << (8 * j);
        }
        for (int j = 0; j < 4; ++j) {
            const long long p = b + j - g;
            if (p >= 0 && p < len) dst[p] = (unsigned char)(v >> (8 * j));
        }
    }
}

// one block per NU_EROW_T outputs of one row: tmp = the row min over [x - a, x + k - 1 - a]; the row's maximum -> img_max
__global__ __launch_bounds__(256) void mask_erode_rows_kernel(const unsigned char* __restrict__ m, int h, int w, int k,
                                                              unsigned char* __restrict__ tmp, int* __restrict__ img_max, long long total) {
    __shared__ unsigned char lds[NU_EROW_CAP];
    __shared__ int smax;
    const int segs = nu_cdiv(w, NU_EROW_T);
    const long long row = blockIdx.x / segs;                 // image * h + y
    const int x0 = (int)(blockIdx.x - row * segs) * NU_EROW_T;
    const int x1 = min(x0 + NU_EROW_T, w);                   // outputs [x0, x1)
    const int a = k / 2, b = k - 1 - a;
    const int lo = max(x0 - a, 0), hi = (int)min((long long)x1 - 1 + b, (long long)w - 1);      // inputs [lo, hi]
    const long long base = row * w;
    const int tid = threadIdx.x;
    if (tid == 0) smax = 0;
    unsigned char r[NU_EROW_T / 256];
    for (int i = 0; i < NU_EROW_T / 256; ++i) r[i] = 255;
    int mx = 0;
    for (int c0 = lo; c0 <= hi; c0 += NU_EROW_CAP) {
        const int c1 = min(c0 + NU_EROW_CAP - 1, hi);
        __syncthreads();
        nu_fill_bytes(m, total, base + c0, c1 - c0 + 1, lds, tid, 256);
        __syncthreads();
        for (int i = 0; i < NU_EROW_T / 256; ++i) {
            const int x = x0 + tid + i * 256;
            if (x >= x1) break;
            const int s0 = max(x - a, c0), s1 = min(x + b, c1);
            unsigned char v = r[i];
            for (int s = s0; s <= s1; ++s) v = min(v, lds[s - c0]);
            r[i] = v;
            if (x >= c0 && x <= c1) mx = max(mx, (int)lds[x - c0]);
        }
    }
    for (int i = 0; i < NU_EROW_T / 256; ++i) {
        const int x = x0 + tid + i * 256;
        if (x < x1) tmp[base + x] = r[i];
    }
    // the block's maximum, then one atomic per block (image maxima start at 0 from the host-side memset)
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) atomicMax(&smax, mx);
    __syncthreads();
    if (tid == 0 && smax > 0) atomicMax(&img_max[row / h], smax);
}

// one block per NU_ECOL_TC columns x NU_ECOL_TR output rows: out = min over [y - a, y + k - 1 - a] of tmp + (max - m)
__global__ __launch_bounds__(256) void mask_erode_cols_kernel(const unsigned char* __restrict__ m, const unsigned char* __restrict__ tmp,
                                                              int h, int w, int k, const int* __restrict__ img_max, long long total,
                                                              unsigned char* __restrict__ out) {
    __shared__ unsigned char lds[NU_ECOL_CAPR][NU_ECOL_TC];
    const int cx = nu_cdiv(w, NU_ECOL_TC), cy = nu_cdiv(h, NU_ECOL_TR);
    const int img = blockIdx.x / (cx * cy);
    const int t = blockIdx.x - img * cx * cy, ty = t / cx, tx = t - ty * cx;
    const int x0 = tx * NU_ECOL_TC, y0 = ty * NU_ECOL_TR;
    const int ncol = min(NU_ECOL_TC, w - x0), y1 = min(y0 + NU_ECOL_TR, h);   // outputs rows [y0, y1), columns [x0, x0 + ncol)
    const int a = k / 2, b = k - 1 - a;
    const int lo = max(y0 - a, 0), hi = (int)min((long long)y1 - 1 + b, (long long)h - 1);
    const long long ibase = (long long)img * h * w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char r[NU_ECOL_TR];
    for (int i = 0; i < NU_ECOL_TR; ++i) r[i] = 255;
    for (int c0 = lo; c0 <= hi; c0 += NU_ECOL_CAPR) {
        const int c1 = min(c0 + NU_ECOL_CAPR - 1, hi);
        __syncthreads();
        for (int yy = c0 + wave; yy <= c1; yy += 4)          // one wave per staged row
            nu_fill_bytes(tmp, total, ibase + (long long)yy * w + x0, ncol, lds[yy - c0], lane, 64);
        __syncthreads();
        if (tid < ncol) {
            for (int i = 0; i < NU_ECOL_TR; ++i) {
                const int y = y0 + i;
                if (y >= y1) break;
                const int s0 = max(y - a, c0), s1 = min(y + b, c1);
                unsigned char v = r[i];
                for (int s = s0; s <= s1; ++s) v = min(v, lds[s - c0][tid]);
                r[i] = v;
            }
        }
    }
    if (tid < ncol) {
        const int mx = img_max[img];
        for (int i = 0; i < NU_ECOL_TR; ++i) {
            const int y = y0 + i;
            if (y >= y1) break;
            const long long p = ibase + (long long)y * w + x0 + tid;
            out[p] = (unsigned char)(r[i] + (mx - m[p]));
        }
    }
}

extern "C" long long nu_mask_erode_workspace_bytes(int n, int h, int w) {
    if (n < 0 || h <= 0 || w <= 0) return 0;
    return ((long long)n * h * w + 255) / 256 * 256 + (long long)n * 4;
}

extern "C" int nu_mask_erode(const unsigned char* m, int n, int h, int w, int k, void* work, long long work_bytes, unsigned char* out,
                             hipStream_t stream) {
    if (n < 0 || h <= 0 || w <= 0 || k < 1 || !m || !out) return NU_ERR_ARG;
    if (n == 0) return NU_OK;
    if (!work || work_bytes < nu_mask_erode_workspace_bytes(n, h, w)) return NU_ERR_WORKSPACE;
    const long long total = (long long)n * h * w;
    const long long rblocks = (long long)n * h * nu_cdiv(w, NU_EROW_T);
    const long long cblocks = (long long)n * nu_cdiv(h, NU_ECOL_TR) * nu_cdiv(w, NU_ECOL_TC);
    if (rblocks > 0x7fffffffLL || cblocks > 0x7fffffffLL) return NU_ERR_ARG;   // the caller chunks over images
    unsigned char* tmp = (unsigned char*)work;
    int* img_max = (int*)((char*)work + (total + 255) / 256 * 256);
    if (hipMemsetAsync(img_max, 0, (size_t)n * 4, stream) != hipSuccess) return NU_ERR_LAUNCH;
    hipLaunchKernelGGL(mask_erode_rows_kernel, dim3((unsigned)rblocks), dim3(256), 0, stream, m, h, w, k, tmp, img_max, total);
    hipLaunchKernelGGL(mask_erode_cols_kernel, dim3((unsigned)cblocks), dim3(256), 0, stream, m, tmp, h, w, k, img_max, total, out);
    return nu_launch_status();
}
