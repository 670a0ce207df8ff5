// sdf_trace.hip -- sphere tracing of the SDF network as ONE kernel: ray -> first point where |f| < threshold (or where the march gave up).
//
// Reference: sphere_tracing(), network/tracing.py:103-164 -- bounding-sphere entry (:118-133), then up to num_iterations times
// x += d * clamp(f(x), -10, 10) (:138-149), leaving the sphere ends a ray (:150-152), |f| < threshold converges it (:153).  There it is
// a Python loop over whole-batch MLP calls whose `break` (:156) fires when EVERY ray is done, so a converged ray is evaluated (not moved)
// again and again and, at i == 0, is moved once whatever its state: a ray's result is that of the function called on the ray alone,
// which is what this kernel computes, ray by ray:
//
//   fgr = finite(o) && (fg == NULL || fg[r]);  x = o;  t = 0
//   if Rb > 0:  a = (d0 d0 + d1 d1) + d2 d2;  b = 2 ((d0 o0 + d1 o1) + d2 o2);  c = ((o0 o0 + o1 o1) + o2 o2) - Rb Rb
//               disc = b b - (4 a) c;  bounded = disc >= 0;  t0 = (-b - sqrt(disc)) / (2 a);  ENTRY_FORWARD: t0 = max(t0, 0)
//               if bounded: x = o + d t0, t = t0;   fgr &= bounded
//   for i < max_iter while fgr:  s = clamp(f(x), -10, 10), NaN -> 10;  x = x + d s;  t = t + s;  iters = i + 1;  sdf_last = s
//                                if Rb > 0: fgr &= sqrt((x0 x0 + x1 x1) + x2 x2) < Rb;   conv = |s| < threshold;  stop if conv or !fgr
//   hit = conv && fgr;  a ray that never was foreground: pos = o, t = 0, iters = 0, sdf_last = 0, hit = 0
// Every operation is a separately rounded fp32 multiply / add / divide / square root in exactly this order (st_mul .. st_sqrt below: no
// contraction; division and square root correctly rounded), so a numpy-float32 or torch restatement returns the same bits.
//
// Design.  The march is a data-dependent loop (4 .. max_iter evaluations per ray) around an eight-layer MLP.  A persistent workgroup
// holds 64 ray SLOTS (position, direction, t, ray index, iteration count: 2.5 KB of LDS) and runs, per iteration, the whole network on the
// 64 slot positions with the pipeline of csrc/fused_mlp.h and the epilogue and head of sdf_fused_fwd_kernel<2> (csrc/fused_sdf.hip): f
// carries the bits of nu_sdf_fused_fwd.  After the head
// wave 0 (lane = slot) applies the step, retires the rays that are done (their outputs go straight to global memory) and refills the
// free slots from the workgroup's own ray sequence: rays b, b + G, b + 2 G, .. for workgroup b of G.  The
// assignment is static: no global counter, no atomics, no workspace, no host read; a ray's arithmetic involves its own row of the tile
// only, so its result does not depend on its slot, its neighbours, the grid or the ray order.  Rays that never become foreground (fg
// 0, a non-finite origin, a miss of the bounding sphere) are retired inside the refill loop and never occupy a slot.
// LDS: 66 576 (activations) + 10 240 (embedding) + 73 728 (weight stages) + 2 564 (slots, head results) = 153 108 B: one workgroup per CU.
#include "fused_mlp.h"

#define ST_TM 64                   // ray slots per workgroup

// One rounding per operation, never contracted.  (HIP's __fsqrt_rn is the native, not correctly rounded, square root unless the
// library is built with OCML_BASIC_ROUNDED_OPERATIONS; sqrtf and `/` are correctly rounded under hipcc's defaults, which build.py keeps.)
static __device__ inline float st_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
static __device__ inline float st_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
static __device__ inline float st_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
static __device__ inline float st_div(float a, float b) { return a / b; }
static __device__ inline float st_sqrt(float a) { return __builtin_sqrtf(a); }
static __device__ inline float st_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return st_add(st_add(st_mul(a0, b0), st_mul(a1, b1)), st_mul(a2, b2));
}

struct StNet {                     // what the kernel needs of NuSdfNet (kernel-argument block)
    const float* Wp[8]; const float* bias[8];
    const float* w8; const float* b8;
    int Kp[8], N[8];
};
struct StRays {
    const float* O; const float* D; const unsigned char* fg;
    int o_ld, d_ld, R, max_iter, entry_forward;
    float threshold, rb;
};
struct StOut { float *pos, *t, *sdf; int* iters; unsigned char* hit; };

static __device__ inline void st_write(const StOut& out, long long ray, float x0, float x1, float x2, float t, float s, int iters, bool hit) {
    if (out.pos) { out.pos[3 * ray] = x0; out.pos[3 * ray + 1] = x1; out.pos[3 * ray + 2] = x2; }
    if (out.t) out.t[ray] = t;
    if (out.sdf) out.sdf[ray] = s;
    if (out.iters) out.iters[ray] = iters;
    if (out.hit) out.hit[ray] = hit ? 1 : 0;
}

__global__ __launch_bounds__(256, 1) void sdf_trace_kernel(StNet net, StRays rays, StOut out) {
    constexpr int TM = ST_TM;
    __shared__ __attribute__((aligned(16))) float act[TM * FM_ALD + FM_APAD];
    __shared__ __attribute__((aligned(16))) float emb[TM * FM_ELD];
    __shared__ __attribute__((aligned(16))) float bst[2 * FM_BSTAGE];
    __shared__ float sx[TM * 3], sd[TM * 3], st[TM], res[TM];               // slot state: position, direction, t; the head's f(x)
    __shared__ int sray[TM], sit[TM];                                        // ray of the slot (-1: free), evaluations so far
    __shared__ int s_live;

    const FmThread T = fm_thread();
    const int tid = threadIdx.x, lane = T.lane, wc = T.wc, li = T.li, lh = T.lh;
    const int a0_off = li * FM_ALD + 4 * lh, a1_off = a0_off + 32 * FM_ALD;

    // this workgroup's ray sequence: position q -> ray q gridDim + blockIdx, q < nq.  Neighbouring rays march alike (the rays that graze
    // the surface and run to max_iter lie along the silhouette), so they go to different workgroups; nothing is gained by keeping them
    // together, a pass costs the same whatever the slots hold
    const long long nq = (int)blockIdx.x < rays.R ? (rays.R - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    long long nxt = 0;                                         // (wave 0) next position of the sequence

    if (tid < TM) {
        sray[tid] = -1; sit[tid] = 0;
        sx[3 * tid] = sx[3 * tid + 1] = sx[3 * tid + 2] = 0.f;
        sd[3 * tid] = sd[3 * tid + 1] = sd[3 * tid + 2] = 0.f;
        st[tid] = 0.f; res[tid] = 0.f;
    }
    __syncthreads();

    FmStream S;
    FmFrag F0;

    for (;;) {
        // ---- wave 0, lane = slot: the step of the slot's ray on the f(x) of the last pass, then refill of the free slots ----
        if (wc == 0) {
            int ray = sray[lane];
            if (ray >= 0) {
                float s = res[lane];
                s = s != s ? 10.f : fminf(fmaxf(s, -10.f), 10.f);
                const float d0 = sd[3 * lane], d1 = sd[3 * lane + 1], d2 = sd[3 * lane + 2];
                const float x0 = st_add(sx[3 * lane], st_mul(d0, s)), x1 = st_add(sx[3 * lane + 1], st_mul(d1, s)),
                            x2 = st_add(sx[3 * lane + 2], st_mul(d2, s));
                const float t = st_add(st[lane], s);
                const int it = sit[lane] + 1;
                const bool inside = rays.rb > 0.f ? st_sqrt(st_dot3(x0, x1, x2, x0, x1, x2)) < rays.rb : true;
                const bool conv = fabsf(s) < rays.threshold;
                if (conv || !inside || it >= rays.max_iter) {
                    st_write(out, ray, x0, x1, x2, t, s, it, conv && inside);
                    ray = -1;
                    sray[lane] = -1;
                    sx[3 * lane] = sx[3 * lane + 1] = sx[3 * lane + 2] = 0.f;       // a free slot evaluates f(0); nobody reads it
                } else {
                    sx[3 * lane] = x0; sx[3 * lane + 1] = x1; sx[3 * lane + 2] = x2;
                    st[lane] = t; sit[lane] = it;
                }
            }
            for (;;) {
                const unsigned long long free_mask = __ballot(ray < 0);
                if (free_mask == 0ull || nxt >= nq) break;
                const long long q = nxt + __popcll(free_mask & ((1ull << lane) - 1ull));
                const long long left = nq - nxt;
                const int nfree = __popcll(free_mask);
                nxt += nfree < left ? nfree : left;
                const long long r = q * (long long)gridDim.x + blockIdx.x;
                if (ray < 0 && q < nq && r < rays.R) {
                    const float* po = rays.O + r * rays.o_ld;
                    const float* pd = rays.D + r * rays.d_ld;
                    const float o0 = po[0], o1 = po[1], o2 = po[2], d0 = pd[0], d1 = pd[1], d2 = pd[2];
                    bool fgr = isfinite(o0) && isfinite(o1) && isfinite(o2) && (rays.fg == nullptr || rays.fg[r] != 0);
                    float x0 = o0, x1 = o1, x2 = o2, t = 0.f;
                    if (rays.rb > 0.f) {
                        const float a = st_dot3(d0, d1, d2, d0, d1, d2);
                        const float b = st_mul(2.f, st_dot3(d0, d1, d2, o0, o1, o2));
                        const float c = st_sub(st_dot3(o0, o1, o2, o0, o1, o2), st_mul(rays.rb, rays.rb));
                        const float disc = st_sub(st_mul(b, b), st_mul(st_mul(4.f, a), c));
                        const bool bounded = disc >= 0.f;
                        if (bounded) {
                            float t0 = st_div(st_sub(-b, st_sqrt(disc)), st_mul(2.f, a));
                            if (rays.entry_forward) t0 = t0 < 0.f ? 0.f : t0;       // (a NaN stays)
                            x0 = st_add(o0, st_mul(d0, t0)); x1 = st_add(o1, st_mul(d1, t0)); x2 = st_add(o2, st_mul(d2, t0));
                            t = t0;
                        }
                        fgr = fgr && bounded;
                    }
                    if (fgr) {
                        ray = (int)r;
                        sray[lane] = ray; sit[lane] = 0; st[lane] = t;
                        sx[3 * lane] = x0; sx[3 * lane + 1] = x1; sx[3 * lane + 2] = x2;
                        sd[3 * lane] = d0; sd[3 * lane + 1] = d1; sd[3 * lane + 2] = d2;
                    } else {
                        st_write(out, r, o0, o1, o2, 0.f, 0.f, 0, false);
                    }
                }
            }
            const unsigned long long busy = __ballot(ray >= 0);
            if (lane == 0) s_live = busy != 0ull ? 1 : 0;
        }
        __syncthreads();
        if (s_live == 0) break;                               // every slot free and the sequence used up (uniform)

        // ---- embedding of the slot positions: columns 0..38 (zero pad to 64) -> act, and a copy for layer 4's skip input ----
        for (int idx = tid; idx < TM * 64; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            float x[3] = {sx[3 * r], sx[3 * r + 1], sx[3 * r + 2]};
            const float v = c < 39 ? fm_embed_col(x, c) : 0.f;
            act[r * FM_ALD + c] = v;
            if (c < FM_ELD) emb[r * FM_ELD + c] = v;
        }
        S.prologue(net, 8, bst, T);
        S.first_b(F0, bst, T);

        for (int l = 0; l < 8; ++l) {
            const FmAcc<2> A = fm_layer<2>(S, net, 8, net.Kp[l] / 32, act, a0_off, a1_off, bst, F0, T);
            const f32x16 (&acc)[2][2] = A.v;
            // ---- epilogue: h = softplus(acc + bias) back over the activation tile (all reads of it retired at the last barrier) ----
            const int N = net.N[l];
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = wc * 64 + tn * 32 + li;
                const float bv = col < N ? net.bias[l][col] : 0.f;
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        // columns [N, 256) (layer 3: the slots of the skip embedding) are not this layer's
                        if (col < N) act[row * FM_ALD + col] = nu_softplus100_fast(acc[tm][tn][r] + bv);
                    }
            }
            if (l == 3) fm_skip_reinsert(act, emb, TM);
            __syncthreads();
        }
        // ---- sdf head: one wave per slot, the arithmetic of skinny_fwd_kernel<1, 256> (16 bytes per lane, xor-shuffle reduction) ----
        {
            const f32x4 w = *reinterpret_cast<const f32x4*>(net.w8 + 4 * lane);
            const float b = net.b8[0];
            for (int r = wc; r < TM; r += 4) {
                const float a = fm_row_dot(&act[r * FM_ALD], w, lane);
                if (lane == 0) res[r] = a + b;
            }
        }
        __syncthreads();            // res is complete; the tile's LDS is free for the next pass
    }
}

// Sphere tracing of R rays (O [R, o_ld], D [R, d_ld]: the first three floats of a row; fg [R] bytes or NULL) against the SDF network,
// per ray as stated at the top of this file.  pos [R,3], t [R], sdf_last [R], iters [R], hit [R] (bytes 0 / 1); every output pointer may
// be NULL.  Exact fp32 on the fp32 packed tables, no workspace, no host read.
extern "C" int nu_sdf_trace(const NuSdfNet* net, const float* O, int o_ld, const float* D, int d_ld, int R, const unsigned char* fg,
                            int max_iter, float threshold, float bound_radius, int flags, float* pos, float* t, float* sdf_last,
                            int* iters, unsigned char* hit, hipStream_t stream) {
    if (!net || !O || !D || R < 0 || o_ld < 3 || d_ld < 3 || max_iter < 1 || !(threshold > 0.f)) return NU_ERR_ARG;
    if (R == 0) return NU_OK;
    StNet n;
    for (int l = 0; l < 8; ++l) {
        const NuLin& L = net->lin[l];
        const int Kexp = l == 0 ? 64 : 256;
        if (L.Kp != Kexp || L.N > 256 || L.N < 1 || !L.Wp || !L.bias) return NU_ERR_ARG;     // SDFNetwork(dims 39 -> 8 x 256 -> 257, skip at 4)
        n.Wp[l] = L.Wp; n.bias[l] = L.bias; n.Kp[l] = L.Kp; n.N[l] = L.N;
    }
    if (net->lin[3].N != 217 || net->lin[8].Kp != 256 || !net->lin[8].Wp || !net->lin[8].bias) return NU_ERR_ARG;
    n.w8 = net->lin[8].Wp; n.b8 = net->lin[8].bias;
    StRays r;
    r.O = O; r.D = D; r.fg = fg; r.o_ld = o_ld; r.d_ld = d_ld; r.R = R; r.max_iter = max_iter;
    r.entry_forward = (flags & NU_TRACE_ENTRY_FORWARD) ? 1 : 0;
    r.threshold = threshold; r.rb = bound_radius;
    const StOut out = {pos, t, sdf_last, iters, hit};
    const int ntiles = nu_cdiv(R, ST_TM);
    hipLaunchKernelGGL(sdf_trace_kernel, dim3(ntiles < 256 ? ntiles : 256), dim3(256), 0, stream, n, r, out);
    return nu_launch_status();
}
