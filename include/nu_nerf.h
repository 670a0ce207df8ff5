/* nu_nerf.h -- C ABI of libnunerf.so: the MI355X (gfx950) hot path of NU-NeRF's stage-1 training step.
 *
 * The reference (jjjkkyz/NU-NeRF) has no FFI: its hot path is eager PyTorch inside
 * network/renderer_zerothick.py and network/field.py.  This header is the boundary a maintainer binds instead
 * (ctypes stub: INTEGRATION.md); each entry names the reference code it replaces (paths relative to the
 * reference repository root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (fp32 unless stated; indices int32; masks uint8),
 *     row-major, contiguous unless a leading dimension (ld*) is given; nothing is allocated or freed inside;
 *     scratch memory comes in through (workspace, workspace_bytes) with a *_workspace_bytes() size query;
 *   - all work is enqueued on `stream` (the caller's current HIP stream); no call synchronises the device;
 *   - return value: 0 on success, negative NU_ERR_* otherwise (never throws);
 *   - "P" counts points, "R" rays, "S" samples per ray.  Activation buffers use padded leading dimensions whose pad
 *     columns are zero (see DESIGN.md "Data layout").
 */
#ifndef NU_NERF_H
#define NU_NERF_H

/* the HIP runtime's own definition, repeated so that plain-C consumers need no HIP headers
 * (an identical typedef redeclaration is legal in C11 and C++) */
typedef struct ihipStream_t* hipStream_t;

#ifdef __cplusplus
extern "C" {
#endif

#define NU_OK 0
#define NU_ERR_ARG (-1)
#define NU_ERR_LAUNCH (-2)
#define NU_ERR_WORKSPACE (-3)

/* ---------------------------------------------------------------------------------------------------------
 * fp32-MFMA GEMMs: the contractions of every `lin(x)` / autograd matmul in field.py:133-150 (SDFNetwork.forward),
 * :158-170 (SDFNetwork.gradient and its double backward), :265-289 (NeRFNetwork.forward), :371-408 (make_predictor).
 * --------------------------------------------------------------------------------------------------------- */
enum NuEpi {                   /* epilogue applied to v = alpha * (A . B^T)[row, col] */
    NU_EPI_BIAS_NONE = 0,      /* C = v + bias[col]                                         (last linear layers) */
    NU_EPI_BIAS_RELU = 1,      /* C = relu(v + bias[col])                                   (field.py:274, :387-391) */
    NU_EPI_BIAS_SOFTPLUS = 2,  /* C = softplus_beta100(v + bias[col])                       (field.py:126-127, :147-148) */
    NU_EPI_MUL_DRELU = 3,      /* C = v * (H > 0)                                           (ReLU backward) */
    NU_EPI_MUL_DSP = 4,        /* C = v * sp'(H),  sp' = 1 - exp(-100 H)                    (Softplus backward) */
    NU_EPI_Q_SP = 5,           /* C = v * sp'(H);  C2 = v * D * 100 * (1 - sp'(H))          (second-order sweep) */
    NU_EPI_B_SP = 6,           /* C = v * sp'(H) + Cadd */
    NU_EPI_PLAIN = 7,          /* C = v */
    NU_EPI_B_RELU = 8,         /* C = v * (H > 0) + Cadd */
    NU_EPI_COUNT = 9
};

#define NU_GEMM_B16 8
#define NU_GEMM_A16 16
#define NU_GEMM_PRESPLIT_ALWAYS 4   /* mode 2 with B6: take the pre-split kernel whatever the tile count (tests; the library otherwise picks) */
#define NU_GEMM_C16 32
#define NU_GEMM_X16 64
typedef struct NuGemmNT {      /* C[M,N] = epi(A[M,K] . B[N,K]^T);  K % 32 == 0, lda/ldb % 4 == 0, A/B 16-byte aligned */
    const float* A; int lda;
    const float* B; int ldb;   /* packed weights: >= ceil128(N) rows, zero padded */
    int M, N, K;
    float* C; int ldc;
    float* C2; int ldc2;
    const float* bias;
    const float* H; int ldh;
    const float* D; int ldd;
    const float* Cadd; int ldadd;
    int zero_to;               /* columns [N, zero_to) of C/C2 are written as 0 */
    int act_cols;              /* derivative epilogues: columns >= act_cols are written as plain v (0: all columns) */
    float alpha;
    int groups;                /* grouped launch; element strides per group follow */
    long long sA, sB, sC, sC2, sBias, sH, sD, sCadd;
    int epi;                   /* enum NuEpi */
    int bf16;                  /* bits 0-1: 0 exact fp32 MFMA (default); 1 bf16 MFMA, fp32 accumulate (operands rounded to bf16);
                                  2 exact 3-way bf16 split of both operands, the six partial products >= 2^-16 (fp32-equivalent).
                                  With mode 1, storage flags (bf16 tensors in HBM, `float*` fields then point to __bf16 data,
                                  leading dimensions stay in ELEMENTS): NU_GEMM_B16 (required: selects the bf16-storage kernel)
                                  B is a bf16 weight table (NuPackDesc.Wp16 / WpT16); NU_GEMM_A16: A is bf16; NU_GEMM_C16: C and
                                  C2 are written as bf16; NU_GEMM_X16: H, D, Cadd are bf16 */
    /* ReLU sign bits (optional): NU_EPI_BIAS_RELU writes, NU_EPI_MUL_DRELU / NU_EPI_B_RELU read them INSTEAD of H -- 2 KB per
     * 128x128 tile in place of 64 KB of activations.  Layout is private to the kernel (wave ballots per 4-row group):
     * cdiv(M,128) * mask_nct * 256 words, mask_nct = column tiles of the activation matrix as the WRITER saw it
     * (groups * cdiv(N,128)); reader and writer must tile the same [M, columns] matrix. */
    unsigned long long* mask; int mask_nct;
    int mask_ct0;              /* first column tile of this problem in the sign-bit matrix: a problem that is one column group of a
                                  wider activation matrix (the four material predictors side by side) when it is launched on its own */
    const void* B6;            /* mode 2 only, optional: B already split into its three bf16 planes by the pack launch (NuPackDesc.planes = 3).
                                  Layout: the table [rows][ldb] (ldb % 16 == 0, rows padded to a multiple of 256) is cut into blocks of 256
                                  rows; a block stores its 16-wide k-groups one after the other, each as [256 rows][hi x16 | mid x16 | lo x16]
                                  (24 576 contiguous bytes -- one LDS stage of the kernel).  bf16 index of element (n, k) of plane p:
                                  ((n >> 8) * (ldb >> 4) + (k >> 4)) * 12288 + (n & 255) * 48 + 16 p + ((k & 15) ^ (n & 8))   [the two halves of a
                                  16-group are swapped in rows with bit 3 set: LDS bank spreading of the kernel's fragment reads].  B6 points at the block the
                                  problem's first row opens (its row offset in the table must be a multiple of 256 -- then 3 x the fp32
                                  table's element offset, and sB applies with the same factor 3).
                                  Selects gemm_nt6_kernel (csrc/gemm_nt6.hip): same results as without it, bit for bit */
} NuGemmNT;

typedef struct NuGemmTN {      /* dW[N1,N2] = A0^T B0 (+ A1^T B1), reduced over P rows in S deterministic splits */
    const float* A0; int lda0; const float* B0; int ldb0;
    const float* A1; int lda1; const float* B1; int ldb1;   /* A1 == NULL: single pair */
    int P, N1, N2;
    float* slab; float* bias_slab;                           /* filled by nu_wgrad from the workspace */
    int S, groups;
    long long sA0, sB0, sA1, sB1, sSlab, sBiasSlab;
    int bf16, pad_;                                          /* bits 0-1 as NuGemmNT.bf16; storage flags (mode 1): NU_TN_A0_16 ... */
} NuGemmTN;
#define NU_TN_A0_16 16
#define NU_TN_B0_16 32
#define NU_TN_A1_16 64
#define NU_TN_B1_16 128

/* One deterministic split reduction: out[n1*ldo + n2] (+)= alpha * sum_{s<S} slab[s*ss + n1*rs + n2], n1 < N1, n2 < N2.
 * Producers (nu_wgrad_enqueue, nu_skinny_bwd_enqueue, nu_colsum_enqueue) append these to a caller-owned HOST array;
 * nu_slab_reduce_batched runs up to NU_REDUCE_MAX of them per launch.  G and blk_begin are filled by the library. */
#define NU_REDUCE_MAX 48
typedef struct NuReduceDesc {
    const float* slab; float* out;
    long long ss;
    int S, N1, N2, rs, ldo, accumulate, G, blk_begin;
    float alpha; int pad_;
} NuReduceDesc;
int nu_reduce_desc_size(void);
int nu_slab_reduce_batched(const NuReduceDesc* descs_host, int n, hipStream_t stream);

int nu_gemm_nt_size(void);      /* sizeof(NuGemmNT) / sizeof(NuGemmTN) as compiled: binding-side ABI check */
int nu_gemm_tn_size(void);
int nu_gemm_nt_ex(const NuGemmNT* g, hipStream_t stream);
/* n independent problems (HOST array; own M, N, K, pointers and epilogue arguments) in as few persistent launches as possible: runs
 * of problems with one epilogue kind share ONE tile list -- the four light predictors of AppShadingNetwork.forward (field.py:636-682),
 * the IoR / thickness pair of stage 2 (field.py:1046-1087).  Results are bit-identical to n calls of nu_gemm_nt_ex. */
#define NU_NT_BATCH_MAX 8
int nu_gemm_nt_batch(const NuGemmNT* problems_host, int n, hipStream_t stream);
/* Which row-tile height a launch of these problems takes (host only: launches nothing, reads no device memory).  64 or 128: the tiles of
 * the exact-fp32 kernel that nu_gemm_nt_ex (n == 1) or nu_gemm_nt_batch (the first run of the list that shares a launch) picks, by the
 * very code the dispatch decides with.  0: the launch does not reach that kernel (another arithmetic mode, M <= 0, n == 0).
 * Negative NU_ERR_*: arguments the launch itself rejects. */
int nu_gemm_nt_tile_rows(const NuGemmNT* problems_host, int n);
long long nu_wgrad_workspace_bytes(int N1, int N2, int S, int groups);
/* the split (number of deterministic partial slabs) the library's own sequencing uses for a weight gradient of this shape */
int nu_wgrad_pick_split(int P, int N1, int N2, int groups, int prec);
/* deferred weight gradient: split GEMM now, reductions appended to descs[*ndesc...] (capacity cap); the workspace must
 * stay untouched until nu_slab_reduce_batched(descs, *ndesc) has been enqueued */
int nu_wgrad_enqueue(const NuGemmTN* g, float* dW, int ldw, long long sW, float* db, long long sDb, void* workspace,
                     long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream);
/* dW (ld = ldw, group stride sW) and optionally db[N1] = column sums of A0 (group stride sDb) */
int nu_wgrad(const NuGemmTN* g, float* dW, int ldw, long long sW, float* db, long long sDb, void* workspace,
             long long workspace_bytes, hipStream_t stream);
/* flat-argument variants (tests / stand-alone use) */
int nu_gemm_nt(const float* A, int lda, const float* B, int ldb, int M, int N, int K, float* C, int ldc, float* C2,
               int ldc2, const float* bias, const float* H, int ldh, const float* D, int ldd, const float* Cadd,
               int ldadd, int zero_to, float alpha, int epi, hipStream_t stream);
long long nu_gemm_tn_workspace_bytes(int N1, int N2, int S);
int nu_gemm_tn(const float* A0, int lda0, const float* B0, int ldb0, const float* A1, int lda1, const float* B1,
               int ldb1, int P, int N1, int N2, float* C, int ldc, float* bias_out, int S, void* workspace,
               long long workspace_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Weight packing: nn.utils.weight_norm (W = v * g / ||v||_row, field.py:121-122, :386-393) folded into padded,
 * optionally column-permuted and transposed operand buffers; and its chain rule back to (weight_v, weight_g).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct NuPackDesc {
    const float* v; const float* g; const int* colmap;
    float* Wp; float* WpT; const float* dWp;
    long long dv_off, dg_off;                 /* offsets (floats) into the flat gradient buffer */
    const float* bias; float* bias_p;
    float scale;
    int N, K, Kp, ldT, ldd, row_begin, col_off;
    void* Wp16; void* WpT16;                  /* optional bf16 copies of Wp / WpT (same shapes, same leading dimensions) */
    int planes, pad_;                         /* 1 (or 0): the copies are Wp / WpT rounded to bf16.  3: the exact hi / mid / lo split in the
                                                 layout of NuGemmNT.B6 (the bf16x6 mode's weight tables): Wp16 / WpT16 then point at the START of
                                                 the twin of the whole table, and the layer's place in it is given below */
    int w6_row0, w6_ld, t6_row0, t6_col0, t6_ld, pad2_;   /* planes == 3: first row (and leading dimension) of this layer in the Wp table;
                                                 first row / first column / leading dimension in the WpT table */
} NuPackDesc;
int nu_pack_desc_size(void);
int nu_pack_layers(const void* descs_dev, int ndesc, int total_rows, hipStream_t stream);
int nu_unpack_grads(const void* descs_dev, int ndesc, int total_rows, float* flat_grads, hipStream_t stream);
/* The same for the rows [row0, row0 + nrows) of the table only (rows are numbered through all layers in descriptor order): what one
 * network-level op of stage 2 owns -- its weight-norm gradients land in `flat_grads`, every other slot stays untouched. */
int nu_unpack_grads_range(const void* descs, int ndesc, int row0, int nrows, float* flat_grads, hipStream_t stream);

/* 1..6-wide output heads (field.py:393 final Linear of make_predictor; :260-261 alpha_linear / rgb_linear) */
int nu_skinny_fwd(const float* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO, float* out,
                  int ldo, hipStream_t stream);
long long nu_skinny_bwd_workspace_bytes(int K, int NO);
int nu_skinny_bwd(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws, int ldw, int NO,
                  float* dH, int lddh, int relu_mask, int accumulate, float* dWs, int lddw, float* db, void* workspace,
                  long long workspace_bytes, hipStream_t stream);
int nu_skinny_bwd_enqueue(const float* dy, int ldy, const float* H, int ldh, int P, int K, const float* Ws, int ldw,
                          int NO, float* dH, int lddh, int relu_mask, int accumulate, float* dWs, int lddw, float* db,
                          void* workspace, long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap,
                          hipStream_t stream);
/* bf16-storage forms (NuOpCtx.h16): the hidden rows H -- and the dH written -- are __bf16; head weights, dy, outputs and every
 * reduction stay fp32 */
int nu_skinny_fwd_h16(const void* H, int ldh, int P, int K, const float* Ws, int ldw, const float* b, int NO, float* out, int ldo,
                      hipStream_t stream);
int nu_skinny_bwd_enqueue_h16(const float* dy, int ldy, const void* H, int ldh, int P, int K, const float* Ws, int ldw, int NO,
                              void* dH, int lddh, int relu_mask, int accumulate, float* dWs, int lddw, float* db, void* workspace,
                              long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream);
long long nu_colsum_workspace_bytes(int ncols);
int nu_colsum_enqueue(const float* A, int lda, int P, int ncols, float* out, int accumulate, void* workspace,
                      long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream);
int nu_colsum(const float* A, int lda, int P, int ncols, float* out, int accumulate, void* workspace,
              long long workspace_bytes, hipStream_t stream);
/* D = w[col] * softplus'(H): seed of the reverse sweep of SDFNetwork.gradient (field.py:158-170) */
int nu_rowscale_dsp(const float* H, int ldh, int P, int K, const float* w, float* D, int ldd, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Encodings
 * --------------------------------------------------------------------------------------------------------- */
/* get_embedder(6,3) of the SDF input (field.py:14-61, :133-136): E[P,64], skip-concat slot of U4[P,256], x-slot of YX */
int nu_sdf_embed(const float* pt, int pt_ld, int P, float* E, float* U4, float* YX, hipStream_t stream);
/* Generic get_embedder(n_freq <= 10, 3) (network/field.py:14-61) for the widths the SDF path does not use -- the 8-frequency position
 * code and the 2-frequency refraction codes of AppShadingNetwork_SpecInner (field.py:1351-1354): out [P, ldo >= 3 + 6 n_freq];
 * _bwd: g [P, ldg] -> dx [P,3]. */
int nu_embed_n_fwd(const float* x, int P, int n_freq, float* out, int ldo, hipStream_t stream);
int nu_embed_n_bwd(const float* x, const float* g, int ldg, int P, int n_freq, float* dx, hipStream_t stream);
/* n = J_emb^T (G0 + Gs): last step of d sdf / d x (field.py:163-170);  q0 = J_emb nbar: first step of its adjoint */
int nu_embed_jt(const float* E, const float* G0, int ldg0, const float* Gs, int ldgs, int P, float* n, hipStream_t stream);
int nu_embed_j(const float* E, const float* nbar, int P, float* Q0, float* Q4, hipStream_t stream);
/* integrated directional encoding, 72-d (utils/ref_utils.py:84-114) and its gradient */
int nu_ide(const float* dirs, const float* kappa_inv, int P, float* out, int ldo, hipStream_t stream);
int nu_ide_bwd(const float* dirs, const float* kappa_inv, const float* gout, int ldg, int P, float* ddirs,
               float* dkappa, hipStream_t stream);
/* inputs of the four light predictors (field.py:636-682, :686-689, :717) and the backward to normals / roughness */
/* sphere = shader_config.sphere_direction (144-d outer_light input, field.py:641-646, :675-679);
 * refrac_dim = 3 + 6 * refrac_freq (field.py:590-591) */
int nu_shade_encode_fwd(const float* nrm, const float* pt, int pt_ld, const float* E, const float* Mraw, int ldm, int P,
                        int sphere, int ld_ol, int refrac_dim, int ld_rl, float* OLin, float* ILin, float* IWin,
                        float* RLin, float* SD, hipStream_t stream);
int nu_shade_encode_bwd(const float* nrm, const float* pt, int pt_ld, const float* SD, const float* dOLin, int ld_ol,
                        int sphere, const float* dILin, const float* dNoV, int P, float* dn, float* dMraw, int ldm,
                        hipStream_t stream);
/* input rows of human_light_predictor (field.py:411-445, :618-629; csrc/human_light.hip): the reflection r of row p meets the XY plane
 * of the human frame poses[idx[p] / S] ([n_poses,3,4], renderer.get_human_coordinate_poses; S = samples per ray, idx = ray-major sample
 * index); HLin [P, ld_hl >= 24] = IPE(0.3 inter.xy, rho (0.3 dist)^2, 0, 6) with zero padding, rec [P,4] = hit flag, dist, mean.  Rows
 * without a hit encode mean = var = 0 (selected, never multiplied).  _bwd ADDS into dn [P,3] (w.r.t. the raw normal) and into column 1
 * of dMraw, after nu_shade_encode_bwd on the same stream; points and poses carry no gradient. */
int nu_human_encode_fwd(const float* nrm, const float* pt, int pt_ld, const float* Mraw, int ldm, const int* idx, int S,
                        const float* poses, int n_poses, int P, int ld_hl, float* HLin, float* rec, hipStream_t stream);
int nu_human_encode_bwd(const float* nrm, const float* pt, int pt_ld, const float* Mraw, int ldm, const int* idx, int S,
                        const float* poses, int n_poses, const float* rec, const float* dHLin, int ld_hl, int P, float* dn,
                        float* dMraw, int lddm, hipStream_t stream);
/* per-ray mirror query of colour_spec (renderer_zerothick.py:780-781; network/renderer.py:710-725) */
int nu_spec_encode(const float* dirs, const float* x, int R, int sphere, float* out, int ldo, hipStream_t stream);
/* NeRF++ inputs (x/|x|, 1/|x|) L=10 and view -d L=4 (renderer_zerothick.py:687-690; field.py:266-269) */
int nu_nerf_embed(const float* pt, int pt_ld, int P, float* E4, float* U5, float* V, hipStream_t stream);
/* input gradients (stage 2: sample positions depend on the learned IoR, renderer_zerothick.py:1642-1684): d L / d x of the
 * SDF network incl. the second-order term of its normal, and d L / d x, d L / d dir of the NeRF++ inputs */
int nu_embed_jt2(const float* E, const float* dE, int lde, const float* dS, int lds, const float* G0, int ldg0,
                 const float* Gs, int ldgs, const float* nbar, int P, float* dx, int accumulate, hipStream_t stream);
int nu_nerf_embed_bwd(const float* pt, int pt_ld, const float* E4, const float* V, const float* gE, int lde,
                      const float* gS, int lds, const float* gV, int ldv, int P, float* dx, float* ddir,
                      hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * render_core (renderer_zerothick.py:725-820)
 * --------------------------------------------------------------------------------------------------------- */
/* mid-points, section lengths, inner mask |x| <= 1 and its compaction (:730-736, boolean-mask gathers :748-767) */
int nu_partition_count(const float* o, const float* d, const float* z, int R, int S, int* cnt_in, int* off_in,
                       int* totals, hipStream_t stream);
int nu_partition_write(const float* o, const float* d, const float* z, int R, int S, const int* off_in, float* pt_in,
                       int* idx_in, float* pt_out, int* idx_out, unsigned char* inner_rm, hipStream_t stream);
/* compute_sdf_alpha (:657-685) + eikonal term (:769) */
/* also writes max(n.d, 0) into colour channel 3 (the loss_normal integrand of network/renderer.py:693-705) */
int nu_neus_alpha_fwd(const float* YX, int ldy, const float* nrm, const float* pt, const int* idx, int P,
                      const float* variance, float anneal, float* alpha_rm, float* gerr, float* color_rm,
                      hipStream_t stream);
/* dvar (optional): d L / d variance, a sum over all points -- per-block partials go to `workspace`
 * (nu_neus_alpha_bwd_workspace_bytes(P)) and ONE deferred reduction problem is appended to descs (finished by
 * nu_slab_reduce_batched, like every weight gradient): deterministic, and no state inside the library */
long long nu_neus_alpha_bwd_workspace_bytes(int P);
int nu_neus_alpha_bwd(const float* YX, int ldy, const float* nrm, const float* pt, const int* idx, int P,
                      const float* variance, float anneal, const float* dalpha_rm, const float* dgerr,
                      const float* dn_shade, const float* dcolor_rm, float* dYX, int lddy, float* nbar, float* dvar,
                      void* workspace, long long workspace_bytes, NuReduceDesc* descs, int* ndesc, int cap, hipStream_t stream);
/* density_activation + colour activation of compute_density_alpha (:515-516, :691-692) */
int nu_nerf_act_fwd(const float* sigma, int lds, const float* rgb, int ldr, const float* pt, const int* idx, int P,
                    float* alpha_rm, float* color_rm, hipStream_t stream);
int nu_nerf_act_bwd(const float* sigma, int lds, const float* rgb, int ldr, const float* pt, const int* idx, int P,
                    const float* dalpha_rm, const float* dcolor_rm, float* dsigma, int ldds, float* drgb, int lddr,
                    hipStream_t stream);
/* BRDF mix, split-sum LUT lookup (nvdiffrast dr.texture, field.py:719-722), Fresnel, sRGB (field.py:698-740) */
int nu_shade_combine_fwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo,
                         const float* RLo, const float* SD, const float* lut, const int* idx, int P, float exp_max,
                         float* color_rm, float* aux, hipStream_t stream);
int nu_shade_combine_bwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo,
                         const float* RLo, const float* SD, const float* lut, const int* idx, int P, float exp_max,
                         const float* dcolor_rm, float* dMraw, float* dOLo, float* dILo, float* dIWo, float* dRLo,
                         float* dNoV, hipStream_t stream);
/* the same mix with shader_config.human_light (field.py:630-634, :662-665): HLo [P,4] raw heads of human_light_predictor, hrec [P,4]
 * the record of nu_human_encode_fwd (column 0 = hit flag).  On hit rows h = exp(min(raw, 0)), w = clamp(exp(min(raw_3, 0)), 0, 1) and
 * both direct lights become h w + direct (1 - w); a row without a hit is selected through unchanged and its dHLo row is zero.
 * hw (optional) [P,4]: h w and w (the `human_light` validation image before its sRGB curve). */
int nu_shade_combine_hl_fwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo,
                            const float* RLo, const float* HLo, const float* hrec, const float* SD, const float* lut,
                            const int* idx, int P, float exp_max, float* color_rm, float* aux, float* hw, hipStream_t stream);
int nu_shade_combine_hl_bwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo,
                            const float* RLo, const float* HLo, const float* hrec, const float* SD, const float* lut,
                            const int* idx, int P, float exp_max, const float* dcolor_rm, float* dMraw, float* dOLo,
                            float* dILo, float* dIWo, float* dRLo, float* dHLo, float* dNoV, hipStream_t stream);
/* front-to-back composite incl. the background-only composite (:773-779); colour is [R*S,4] = rgb + one auxiliary
 * channel whose composite goes to aux_sum[R] (normal-orientation loss, network/renderer.py:705) */
int nu_composite_fwd(const float* alpha, const float* color, const unsigned char* inner, int R, int S, float* weights,
                     float* rgb, float* acc, float* rgb_bg, float* aux_sum, hipStream_t stream);
int nu_composite_bwd(const float* alpha, const float* color, const unsigned char* inner, int R, int S,
                     const float* drgb, const float* dacc, const float* drgb_bg, const float* daux, float* dalpha,
                     float* dcolor, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Hierarchical sampler (renderer_zerothick.py:572-612, :525-570; field.py:468-498, :501-554)
 * --------------------------------------------------------------------------------------------------------- */
int nu_sample_coarse(const float* o, const float* d, const float* near, const float* far, const float* lin,
                     const float* lower, const float* upper, const float* u1, const float* u2, int R, int Nc, int Nbg,
                     float* zc, float* zbg, float* X, hipStream_t stream);
int nu_upsample(const float* o, const float* d, const float* z, const float* sdf, int R, int sn, const float* variance,
                float inv_s_cap, int use_variance, const float* uvals, int n_new, float* z_new, float* Xn,
                hipStream_t stream);
int nu_probe_weights(const float* o, const float* d, const float* z, const float* sdf, int R, int sn,
                     const float* variance, const float* uvals, int n_new, float* z_new, float* Xn, float* wsum,
                     hipStream_t stream);
int nu_merge_sorted(const float* z, const float* sdf, int sn, const float* zn, const float* sdfn, int nn, int R,
                    float* zo, float* sdfo, hipStream_t stream);
int nu_concat_cols(const float* A, int a, const float* B, int b, int R, float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Mesh closest-hit tracing (stage 2): replaces the OptiX GAS build (network/tracing_optix.py:20-23, :142-146), the
 * launch/IO wrapper (:74-117, :154-158) and the device programs of cuda/triangle.cu:48-99.
 *   rays [N,6] = (origin, direction); hit[N] = 1.0/0.0; idx[N] = face id of the closest hit with tmin < t < tmax, or
 *   10000000 on a miss; ties in t -> lowest face id.  `bvh` is a caller-owned buffer of nu_lbvh_bytes(n_faces) bytes.
 * --------------------------------------------------------------------------------------------------------- */
long long nu_lbvh_bytes(int n_faces);
int nu_lbvh_build(const float* V, int n_verts, const int* F, int n_faces, void* bvh, long long bvh_bytes,
                  hipStream_t stream);
int nu_lbvh_trace(const void* bvh, int n_faces, const float* rays, int N, float tmin, float tmax, float* hit, int* idx,
                  float* t_out, hipStream_t stream);
/* O(N*F) sweep with the same ray/triangle test (cross-check, tiny meshes) */
int nu_brute_trace(const float* V, const int* F, int n_faces, const float* rays, int N, float tmin, float tmax,
                   float* hit, int* idx, float* t_out, hipStream_t stream);
/* closest point on the mesh to each query point (postprocess_stage2_mesh.py's Open3D compute_closest_points; mesh distances):
 * pts [N,3];
 *   d2[N]        squared distance |p - q|^2 in fp32 (no sqrt on the path),
 *   idx[N]       face id of the closest triangle (ties in d2 -> lowest face id),
 *   closest[N,3] q (may be NULL).
 * Only triangles with d2 <= max_d2 count (pass +inf for no bound).  When none qualifies: idx = 10000000, d2 = +inf,
 * closest = (0, 0, 0).  Point/triangle = the regions of Ericson, Real-Time Collision Detection 5.1.5, one rounding per operation in
 * a fixed order; a zero-area triangle is the minimum over its three edges as segments.  Traverses the tree of nu_lbvh_build; two
 * kernels on `stream`, no other stream. */
int nu_lbvh_closest(const void* bvh, int n_faces, const float* pts, int N, float max_d2, float* d2, int* idx, float* closest,
                    hipStream_t stream);
/* O(N*F) sweep with the same point/triangle routine (cross-check; small meshes) */
int nu_brute_closest(const float* V, const int* F, int n_faces, const float* pts, int N, float max_d2, float* d2, int* idx,
                     float* closest, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stage-2 object masks of real captures: render_mask.py -> utils/render_mask_real.py (one OptiX trace per pixel of every training
 * image against the stage-1 mesh) and mask_erosion.py (cv.erode with a k x k box, composed with the inverted original).
 *   cams [n_img, 21] per image: Kinv [3x3] then the world -> camera [R|t] [3x4], both row-major.  Pixel (x, y) of image i:
 *   c = (x + 0.5, y + 0.5, 1), d = normalize(R^T (Kinv c)), o = -R^T t; tmin = 0, tmax = 1e16 (cuda/triangle.cu).
 *   out [n_img, h, w] uint8 = 255 where the pixel's ray hits a triangle, 0 elsewhere: any-hit traversal of the tree of
 *   nu_lbvh_build, the ray made in registers (no ray buffer); the same predicate as nu_lbvh_trace's hit flag, bit for bit.
 *   n_img * ceil(h / 4) * ceil(w / 4) must stay below 2^31 (chunk over images).
 * --------------------------------------------------------------------------------------------------------- */
int nu_mask_pinhole_trace(const void* bvh, int n_faces, const float* cams, int n_img, int h, int w, unsigned char* out,
                          hipStream_t stream);
/* the same rays as rays [n_img * h * w, 6] = (origin, direction), pixel-major per image (tests; not on the hot path) */
int nu_mask_pinhole_rays(const float* cams, int n_img, int h, int w, float* rays, hipStream_t stream);
/* m, out [n, h, w] uint8, k >= 1 (anything else: NU_ERR_ARG), anchor a = k / 2:
 *   eroded[y, x] = min m[y + dy, x + dx], dy, dx in [-a, k - 1 - a], positions outside the image left out (OpenCV's default
 *                  constant border of 255 for erosion);
 *   out          = eroded + (max(m) - m), max over each image (computed on the device).
 * `work` is a caller-owned buffer of nu_mask_erode_workspace_bytes(n, h, w) bytes; out must not alias m. */
long long nu_mask_erode_workspace_bytes(int n, int h, int w);
int nu_mask_erode(const unsigned char* m, int n, int h, int w, int k, void* work, long long work_bytes, unsigned char* out,
                  hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Relighting of the baked mesh under a lat-long HDR environment (relight.py -> blender_backend/relight_backend.py; the light transport
 * is the project's own).  All launches on `stream`, no allocation, no atomics: results are the same bits from
 * run to run and however pixels, images and sample ranges are chunked.
 *   G-buffer row (20 floats): t, hit point [3], geometric normal [3], shading normal [3], albedo [3], metallic, roughness, view vector
 *   [3], image index, pixel index y * w + x (the last two as int bits).  Unit normals; the geometric one faces the viewer, the shading
 *   one (barycentric mix of vnormals [V,3]) lies on its side.  materials [V,5] = albedo, metallic, roughness per vertex.
 *   nu_relight_gbuffer     rows [y0, y0 + rows) of n_img images (cams as nu_mask_pinhole_trace, image i hashes as img0 + i): closest hit
 *                          of the pixel centre -> face [n_img, rows, w] (face id, 10000000 on a miss; face id and t are those of
 *                          nu_lbvh_trace, bit for bit) and gbuf [n_img, rows, w, 20] (zero on a miss).
 *   nu_relight_visibility  pix [n_pix] = G-buffer rows of HIT pixels; samples [s0, s0 + s_count) of `samples` (even): the shadow ray of
 *                          (pixel, sample) -- origin = hit point + eps * geometric normal, direction = sample s of the pixel, see
 *                          DESIGN 20 -- is made in registers and traced any-hit, tmin = 0, tmax = 1e16.  vis [n_pix, s_count] uint8:
 *                          1 = unoccluded, 0 = occluded or not traced (direction below the shading or the geometric horizon).
 *                          n_pix * ceil(s_count / 16) must stay below 2^31.
 *   nu_relight_resolve     out [rows of the G-buffer, 4] += per listed pixel, in sample order, scale * weight * radiance of every sample
 *                          with vis = 1 (rgb); alpha = 1.  env [env_h, env_w, 4] RGBA fp32, 16-byte aligned.  The caller zeroes out
 *                          before the first sample range and passes scale = 2 / samples.
 *   nu_relight_shadow_rays the rays nu_relight_visibility traces, rays [n_pix * s_count, 6]; bits (may be NULL) [n_pix * s_count, 3] =
 *                          the two 24-bit sample integers, 1 where the ray is traced (tests; not on the hot path)
 *   nu_relight_env_lookup  out [N,3] = the bilinear environment lookup of resolve at dirs [N,3] (tests)
 * --------------------------------------------------------------------------------------------------------- */
int nu_relight_gbuffer(const void* bvh, int n_faces, const float* V, const int* F, const float* vnormals, const float* materials,
                       const float* cams, int n_img, int img0, int h, int w, int y0, int rows, int* face, float* gbuf,
                       hipStream_t stream);
int nu_relight_visibility(const void* bvh, int n_faces, const float* gbuf, const int* pix, int n_pix, int samples, int s0, int s_count,
                          int seed, float eps, unsigned char* vis, hipStream_t stream);
int nu_relight_resolve(const float* gbuf, const int* pix, int n_pix, int samples, int s0, int s_count, int seed, const float* env,
                       int env_h, int env_w, const unsigned char* vis, float scale, float* out, hipStream_t stream);
int nu_relight_shadow_rays(const float* gbuf, const int* pix, int n_pix, int samples, int s0, int s_count, int seed, float eps,
                           float* rays, int* bits, hipStream_t stream);
int nu_relight_env_lookup(const float* env, int env_h, int env_w, const float* dirs, int N, float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Split-sum relighting from a prefiltered environment pyramid: the image formation the networks were trained
 * under (network/field.py:684-735), evaluated on the baked mesh with no Monte-Carlo sum, no visibility and no interreflection.
 *   nu_env_prefilter       zonal kernel regression on the sphere.  src_dir [M,4] = unit direction and quadrature weight w, src_rgb [M,4]
 *                          (the fourth value is not read), dirs [N,3], L lobes (lobe_kind, lobe_param: HOST arrays [L]).
 *                            out[l,i] = sum_j w_j f_l(c_ij) rgb_j / sum_j w_j f_l(c_ij),   c_ij = dirs_i . src_dir_j   (rgb; alpha = 1)
 *                            NU_LOBE_COSINE      f = max(c, 0)                                       (param not read)
 *                            NU_LOBE_GGX, alpha  f = c D(NoH) for c > 0, else 0;  NoH^2 = (1 + c) / 2,
 *                                                D = alpha^2 / (pi (NoH^2 (alpha^2 - 1) + 1)^2)     (the GGX prefilter with N = V = R)
 *                            NU_LOBE_VMF, kappa  f = exp(kappa (c - 1))
 *                          out [L,N,4] is WRITTEN.  One query per thread, the source streamed through LDS, c shared by the lobes, sums
 *                          in ONE fixed order (per tile of 256 source entries from zero, tiles added in order), no atomics: a
 *                          query's bits do not depend on N, on its position or on the other lobes.  When N is too small to fill the
 *                          chip the tile range is split over workgroups and folded in tile order by a second launch (the same
 *                          additions, the same bits); that needs ws of nu_env_prefilter_workspace_bytes(N, M, L) bytes (a pure host
 *                          function; 0 when the split is not taken; 16-byte aligned).
 *                          NU_ERR_ARG: a NULL pointer (of an array that is not empty), N < 0, M < 0, L outside 1..NU_ENV_MAX_LOBES, an unknown kind, alpha <= 0,
 *                          kappa <= 0 (or not finite).  NU_ERR_WORKSPACE: ws missing or too small.  N == 0 or M == 0 launches nothing.
 *   nu_env_pyramid_lookup  out [N,3] = L(dirs_i, rho_i): pyr [L,ph,pw,4] RGBA fp32 (16-byte aligned), levels [L] a HOST array, strictly
 *                          ascending, L <= NU_ENV_MAX_LOBES.  rho is clamped to [levels[0], levels[L-1]]; with levels[i] <= rho <=
 *                          levels[i+1] (the largest such i), t = (rho - levels[i]) / (levels[i+1] - levels[i]) and the value is
 *                          (1 - t) tap_i(d) + t tap_{i+1}(d), tap = the bilinear lat-long tap of nu_relight_env_lookup, its operations.
 *                          L = 1: that level's tap.  At a level the value has the bits of that level's tap.
 *   nu_relight_splitsum    the listed HIT pixels of a G-buffer (rows as above), out [rows of the G-buffer, 4] WRITTEN (rgb; alpha = 1):
 *                            NoV = n.v;  r = 2 NoV n - v;  F0 = 0.04 (1 - m) + m a
 *                            (A, B) = fg [256,256,2] bilinear at (clamp(NoV, 0, 1), clamp(rho, 0, 1)), texel centres at (i + 1/2) / 256,
 *                                     clamped to the edge (the lookup of the training kernels)
 *                            rgb = (1 - m) a Ld(n) + (F0 A + B) L(r, rho)
 *                          Ld = diffuse [dh,dw,4], one bilinear tap; L = nu_env_pyramid_lookup's value.  Pixels that are not listed are
 *                          not touched.
 *                          NU_ERR_ARG (both): a NULL pointer, N / n_pix < 0, L outside 1..NU_ENV_MAX_LOBES, a map side <= 0, levels
 *                          not finite or not strictly ascending.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_ENV_MAX_LOBES 16
#define NU_LOBE_COSINE 0
#define NU_LOBE_GGX 1
#define NU_LOBE_VMF 2
long long nu_env_prefilter_workspace_bytes(int N, int M, int L);
int nu_env_prefilter(const float* src_dir, const float* src_rgb, int M, const float* dirs, int N, const int* lobe_kind,
                     const float* lobe_param, int L, float* out, void* ws, long long ws_bytes, hipStream_t stream);
int nu_env_pyramid_lookup(const float* pyr, int L, int ph, int pw, const float* levels, const float* dirs, const float* rho, int N,
                          float* out, hipStream_t stream);
int nu_relight_splitsum(const float* gbuf, const int* pix, int n_pix, const float* pyr, int L, int ph, int pw, const float* levels,
                        const float* diffuse, int dh, int dw, const float* fg, float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Visibility transfer and shadowed split-sum relighting (the project's own quantity, the reference has no
 * counterpart).  All launches on `stream`, no allocation, no atomics, no workspace.
 *   nu_transfer_bake       per surface point i of points [n,3] with UNIT normals [n,3] (a precondition), hashed as id0 + i: `samples`
 *                          (>= 16, a multiple of 16) cosine-weighted hemisphere rays about the normal, origin p + eps n, made in
 *                          registers and traced any-hit against the tree of nu_lbvh_build with tmin = 0, tmax = radius (> 0; 1e16 =
 *                          unbounded, as every other trace).  Sample j of S: Hammersley point (floor(j 2^32 / S), bitreverse32(j)) shifted
 *                          (modulo 2^32) by two hash words of (id, seed), uniforms = the top 24 bits x 2^-24, cos = sqrt(1 - u2),
 *                          sin = sqrt(u2), phi = 2 pi u1 in the orthonormal frame of the normal.  out [n,16] is WRITTEN, V_s = 1 where
 *                          ray s meets nothing:
 *                            [0..8]   T_k = (1/S) sum_s V_s Y_k(w_s): order-2 real SH in the order (0,0) (1,-1) (1,0) (1,1) (2,-2) .. (2,2),
 *                                     0.282095; 0.488603 (y, z, x); 1.092548 xy, 1.092548 yz, 0.315392 (3 z^2 - 1), 1.092548 xz,
 *                                     0.546274 (x^2 - y^2) -- an estimate of the integral of V (cos / pi) Y_k
 *                            [9]      ambient occlusion = (float)(unoccluded samples) / (float)S
 *                            [10..12] bent normal normalize(sum_s V_s w_s); the input normal when the sum is shorter than 1e-12
 *                            [13..15] 0
 *                          One single-wave block per point, 16 samples per round, summed in sample order in fp32: a row's bits depend on
 *                          (point, normal, id, samples, seed, eps, radius, mesh) only -- not on n, the row's position or its neighbours.
 *   nu_transfer_bake_dump  the same kernel; also vis [n,samples] uint8 = V_s (tests)
 *   nu_transfer_rays       the rays nu_transfer_bake traces, rays [n * samples, 6]; bits (may be NULL) [n * samples, 2] = the two 24-bit
 *                          sample integers (tests; not on the hot path)
 *                          NU_ERR_ARG (all three): a NULL pointer of an array that is not empty, n < 0, n_faces <= 0, samples < 16 or not
 *                          a multiple of 16, eps or radius not finite, radius <= 0, n * samples >= 2^31 (the caller chunks over points).
 *                          n == 0 launches nothing.
 *   nu_relight_splitsum_occluded   nu_relight_splitsum shadowed by a transfer [Nv,16] of the mesh's vertices.  face = the G-buffer pass's
 *                          face ids, V, F = the mesh.  With x the stored hit point of a listed pixel and (v0, v1, v2) its face:
 *                            e1 = v1 - v0, e2 = v2 - v0, t = x - v0, den = (e1.e1)(e2.e2) - (e1.e2)^2,
 *                            u = ((e2.e2)(t.e1) - (e1.e2)(t.e2)) / den, v = ((e1.e1)(t.e2) - (e1.e2)(t.e1)) / den  (u = v = 0 unless den > 0)
 *                            row = r0 + u (r1 - r0) + v (r2 - r0) over columns 0..12, the bent normal renormalised
 *                            so = clamp(pow(clamp(NoV, 0, 1) + ao, exp2(-16 rho - 1)) - 1 + ao, 0, 1)       (Lagarde & de Rousiers 2014)
 *                          and D = (1 - m) a Ld(n), Sp = (F0 A + B) L(r, rho) the two terms of nu_relight_splitsum (its operations):
 *                            NU_OCC_AO   rgb = ao D + so Sp           -- the bits of nu_relight_splitsum where ao = 1
 *                            NU_OCC_SH   rgb = (1 - m) a max(sum_k T_k L_k, 0) + so Sp,   L_k = envsh [9,4] row k (RGB + pad, 16-byte
 *                                        aligned): the order-2 SH coefficients of the environment (not read in NU_OCC_AO)
 *                          NU_ERR_ARG: as nu_relight_splitsum, a NULL face / V / F / transfer, an unknown mode.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_OCC_AO 0
#define NU_OCC_SH 1
int nu_transfer_bake(const void* bvh, int n_faces, const float* points, const float* normals, int n, int id0, int samples, int seed,
                     float eps, float radius, float* out, hipStream_t stream);
int nu_transfer_bake_dump(const void* bvh, int n_faces, const float* points, const float* normals, int n, int id0, int samples, int seed,
                          float eps, float radius, float* out, unsigned char* vis, hipStream_t stream);
int nu_transfer_rays(const float* points, const float* normals, int n, int id0, int samples, int seed, float eps, float* rays, int* bits,
                     hipStream_t stream);
int nu_relight_splitsum_occluded(const float* gbuf, const int* face, const int* pix, int n_pix, const float* V, const int* F,
                                 const float* transfer, const float* envsh, int mode, const float* pyr, int L, int ph, int pw,
                                 const float* levels, const float* diffuse, int dh, int dw, const float* fg, float* out,
                                 hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Texture atlas of the relightable asset (the project's own, the reference has no counterpart).  All launches
 * on `stream`, one thread per item, no allocation, no LDS, no atomics, no workspace.
 * The atlas of (n_faces, size = T, pad): a square of T x T texels, texel (x, y) at row y, column x.  cols = ceil(sqrt(ceil(n_faces / 2))),
 * c = T / cols (integer), L = c - 3 - 3 pad; cell k = f >> 1 of face f has its origin at ((k % cols) c, (k / cols) c).  With (i, j) the
 * cell-local texel: the lower face 2k owns i + j <= c - 2, the upper face 2k + 1 owns i + j >= c and lives in the point-mirrored frame
 * (s, t) = (c - 1 - i, c - 1 - j) (the lower face: (s, t) = (i, j)); the diagonal i + j = c - 1, texels outside the cols x cols cells and
 * the halves of faces >= n_faces are owned by nobody.  In its frame a face has its vertices 0, 1, 2 at (pad, pad), (pad + L, pad),
 * (pad, pad + L), and an owned texel stands for the EXTRAPOLATED barycentrics b1 = (s - pad) / L, b2 = (t - pad) / L, b0 = (1 - b1) - b2
 * (integers converted to fp32, one division each).
 *   nu_atlas_texels    rows [y0, y0 + rows) of the atlas.  texel [rows, T, 4] is WRITTEN: the surface point (b0 v0 + b1 v1) + b2 v2 of the
 *                      owning face (each operation one fp32 rounding, in this order: a corner texel holds its vertex's bits) and the
 *                      face id as int bits in the fourth lane; an unowned texel, and one whose face names a vertex outside
 *                      [0, n_verts), is (0, 0, 0, -1).  vnormals [n_verts,3] (unit; may be NULL together with normal): normal
 *                      [rows, T, 4] = the same mix of the vertex normals divided by its length, 0 in the fourth lane; a mix of length 0
 *                      or >= 1e30 (or NaN) gives the unit geometric normal (v1 - v0) x (v2 - v0) instead, zero when that has no length
 *                      either; zero on unowned texels.  A texel's bits do not depend on y0 / rows.
 *   nu_atlas_sample    out [n, 5] = the bilinear lookup at barycentrics uv [n, 2] = (u, v) (weights of vertices 1 and 2) of face [n];
 *                      a face outside [0, n_faces) gives zeros.  atlas = two planes [2, T, T, 4]: (albedo r, g, b, metallic), then
 *                      (roughness, then the texel's object-space normal x, y, z or three zeros); out = albedo, metallic, roughness.  u = clamp(u, 0, 1), v = clamp(v, 0, 1 - u),
 *                      s = pad + u L, t = min(pad + v L, (2 pad + L) - s), taps floor(s), floor(s) + 1, floor(t), floor(t) + 1 in the
 *                      face's frame, fractions fs, ft; value = lo + ft (hi - lo), lo = t00 + fs (t10 - t00), hi = t01 + fs (t11 - t01),
 *                      where fs == 0 (ft == 0) leaves the +1 taps out altogether.  Every tap that takes part has s + t <= c - 2 - pad:
 *                      it is owned by the face, whatever (u, v).
 *   nu_atlas_gbuffer   pix [n_pix] = rows of a G-buffer of nu_relight_gbuffer (gbuf [*, 20], face [*]) for the mesh V, F.  Per listed row
 *                      whose face id is in [0, n_faces): (u, v) of the stored hit point in its face by the formula of
 *                      nu_relight_splitsum_occluded above, nu_atlas_sample's lookup, and columns 10..14 of the row (albedo, metallic,
 *                      roughness) are OVERWRITTEN.  Every other column, every unlisted row and listed miss rows stay as they are.
 *   nu_atlas_sample_normal   out [n, 3] = nu_atlas_sample's lookup (taps, fractions, the fs == 0 / ft == 0 rule, the mix expression, the
 *                      clamp into the triangle) on lanes y, z, w of plane 1 -- the object-space normal of the texel (DESIGN.md section
 *                      32), zero in a texture without normals -- divided by its length sqrt((x x + y y) + z z); zero when that length
 *                      is not in (0, 1e30), and for a face outside [0, n_faces).
 *   nu_atlas_gbuffer_normal  per listed row as nu_atlas_gbuffer: (u, v) of the stored hit point, the lookup of nu_atlas_sample_normal; a
 *                      mix without a length in (0, 1e30) leaves the row as it is, otherwise columns 7..9 (the shading normal) are
 *                      OVERWRITTEN with ns = mix / length, negated when ns . ng < 0, ng = columns 4..6 (the viewer-facing geometric
 *                      normal): the rule of the G-buffer pass for vertex normals.  Nothing else is written.
 *   NU_ERR_ARG (all five): n_faces < 1, size < 1 or > NU_ATLAS_MAX_SIZE, pad < 0 or > NU_ATLAS_MAX_PAD, L < 2, n_verts < 1, a negative
 *   count, rows outside the atlas, a NULL array that is read or written, vnormals without normal or the reverse.  A count of 0
 *   launches nothing.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_ATLAS_CH 5
#define NU_ATLAS_MAX_SIZE 32768
#define NU_ATLAS_MAX_PAD 64
int nu_atlas_texels(const float* V, int n_verts, const int* F, int n_faces, const float* vnormals, int size, int pad, int y0, int rows,
                    float* texel, float* normal, hipStream_t stream);
int nu_atlas_sample(const float* atlas, int size, int n_faces, int pad, const int* face, const float* uv, int n, float* out,
                    hipStream_t stream);
int nu_atlas_gbuffer(float* gbuf, const int* face, const int* pix, int n_pix, const float* V, int n_verts, const int* F, int n_faces,
                     const float* atlas, int size, int pad, hipStream_t stream);
int nu_atlas_sample_normal(const float* atlas, int size, int n_faces, int pad, const int* face, const float* uv, int n, float* out,
                           hipStream_t stream);
int nu_atlas_gbuffer_normal(float* gbuf, const int* face, const int* pix, int n_pix, const float* V, int n_verts, const int* F, int n_faces,
                            const float* atlas, int size, int pad, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Relighting of the NESTED object (the project's own transport, pinned against no other renderer): a
 * transparent outer shell (tree, V_o, F_o, unit vertex normals, index of refraction ior [V_o] >= 1) around an opaque inner mesh
 * (tree, V_i, F_i, unit vertex normals, materials_i [V_i,5]).  The outer G-buffer comes from nu_relight_gbuffer run on the outer mesh
 * with ior - 1 in column 0 of its materials, so that 1 + row[10] is the interpolated index at the primary hit (the excess over 1 is
 * what is interpolated everywhere: a constant index stays that index bit for bit, and an index-matched shell, ior = 1, is exactly absent).
 *   nu_relight_nested_chain    pix [n_pix] = HIT rows of the outer G-buffer.  Per listed pixel, in one launch: the entry interface
 *                              event, the reflection ray (any hit, outer), up to max_segments interior segments (closest hit against
 *                              the inner and the outer tree; inner first when t_inner <= t_outer; total internal reflection goes on),
 *                              the exit ray (any hit, outer).  kind [n_pix] = NU_RLN_DARK / _INNER / _EXIT; chain [n_pix, 12] =
 *                              T, exit direction [3], exit visibility, reflection direction [3], F_entry, reflection visibility,
 *                              segments walked (int bits), 0; inner_rows [n_pix, 20] = the G-buffer row of the inner hit (zero for
 *                              the other kinds; image and pixel index copied from the outer row).
 *   nu_relight_nested_light    sel [n_sel] = indices of INNER pixels into inner_rows; samples [s0, s0 + s_count) of `samples`: per
 *                              (pixel, sample) the light path -- any hit against the inner tree from x + eps n_g, closest hit against
 *                              the outer tree along the same ray, interface event going out, any hit against the outer tree along the
 *                              exit ray -- walked back to back, no ray stored.  rec [n_sel, s_count, 4] = (exit direction,
 *                              1 - F_exit), all zero for a dark or untraced sample.  n_sel * ceil(s_count / 16) stays below 2^31.
 *   nu_relight_nested_resolve  out [rows of the outer G-buffer, 4] += per listed pixel sel[i] (indices into kind / chain / inner_rows;
 *                              opix [n_pix] = the row each writes), in sample order, scale * T * weight * (1 - F_exit) * env(exit
 *                              direction) of the records rec [n_sel, s_count, 4]; when last != 0 also the reflection term and, for
 *                              an exit pixel, T * env(exit direction) * visibility.  alpha = 1.  No atomics: same bits however the
 *                              pixels, images and sample ranges are chunked.  s_count may be 0 (rec may then be NULL).
 *   nu_relight_nested_chain_dump / _light_dump   the same kernels, also writing what they traced (tests):
 *                              seg [n_pix, max_segments, 16] = per walked segment ray o [3], d [3], then as int bits the mesh that ended
 *                              it (0 none, 1 inner, 2 outer) and its face id, t, then (found, face id, t) of the inner and of the
 *                              outer walk, 1; aux [n_pix, 2, 8] = reflection ray and exit ray: o [3], d [3], traced, found.
 *                              dump [n_sel * s_count, 20] = ray o [3], d [3], traced, inner found, outer found, outer face (int bits),
 *                              outer t, refracted, exit ray o [3], d [3], exit found, 1 - F_exit.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_RLN_MAX_SEGMENTS 4
#define NU_RLN_DARK 0
#define NU_RLN_INNER 1
#define NU_RLN_EXIT 2
#define NU_RLN_CHAIN 12
#define NU_RLN_SEG 16
#define NU_RLN_LIGHT_DUMP 20
int nu_relight_nested_chain(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* gbuf, const int* pix, int n_pix, float eps, int max_segments, int* kind,
                            float* chain, float* inner_rows, hipStream_t stream);
int nu_relight_nested_chain_dump(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* gbuf, const int* pix, int n_pix, float eps, int max_segments, int* kind,
                                 float* chain, float* inner_rows, float* seg, float* aux, hipStream_t stream);
int nu_relight_nested_light(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                            int seed, float eps, float* rec, hipStream_t stream);
int nu_relight_nested_light_dump(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                                 int seed, float eps, float* rec, float* dump, hipStream_t stream);
int nu_relight_nested_resolve(const float* inner_rows, const float* chain, const int* kind, const int* opix, const int* sel, int n_sel,
                              int samples, int s0, int s_count, int seed, const float* env, int env_h, int env_w, const float* rec,
                              float scale, int last, float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Relighting through the THIN shell: the nested object of the non-zero-thickness stage-2 model.  The outer mesh
 * is a glass wall -- per vertex an index ior [V_o] > 0, a thickness [V_o] >= 0 and a Gaussian curvature [V_o] -- around an air-like
 * cavity (index 1.0001) that holds the opaque inner mesh.  A ray crosses the wall by the trained geometry (s2_shell_core of
 * csrc/stage2.hip after its sigmoids: two concentric spheres of radius 1 / sqrt(max(|curvature|, 1e-6)) at the hit); each face
 * transmits 1 - Schlick (F0 from the face's two indices, the cosine of the lower-index side); a crossing any face of which reflects
 * totally ends the path dark.  The outer G-buffer comes from nu_relight_gbuffer with ior - 1, thickness, curvature in columns 0..2
 * of the outer materials.  Records are those of the nested entries above, and nu_relight_nested_resolve shades them.
 *   nu_relight_thin_chain   as nu_relight_nested_chain with ONE cavity segment (no max_segments): entry crossing, reflection ray of its
 *                           first face (any hit, outer), the cavity ray from behind the wall (no eps) closest-hit against the inner
 *                           and the outer tree, inner first when t_inner <= t_outer; an outer hit takes the leaving crossing and the
 *                           exit ray (any hit, outer, origin pushed eps along the outward geometric normal).  chain [n_pix, 12] as
 *                           above with T = keep_entry * keep_exit, keep = (1 - F_a)(1 - F_b), and F_entry = F_a of the entry crossing.
 *   nu_relight_thin_light   as nu_relight_nested_light with the leaving crossing; rec = (exit direction, keep).
 *   nu_relight_thin_chain_dump / _light_dump   also what they traced (tests): seg [n_pix, 16] (one segment), aux and dump as above
 *                           (dump[11] = the crossing got out, dump[19] = keep).
 *   nu_relight_thin_cross   tests: the crossing of M rows -- d [M,3] unit, normal [M,3] OUTWARD shading normal, x [M,3], ior,
 *                           thickness, curvature [M], inside 0 / 1 for all rows -> refracts, tir_ok [M] bytes, nrm (oriented unit
 *                           normal), pend (point of the first face), ns, nd (ray behind the wall; zero when !refracts) [M,3],
 *                           fres [M,2] = F_a, F_b.
 * --------------------------------------------------------------------------------------------------------- */
int nu_relight_thin_chain(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* thickness, const float* curvature,
    const float* gbuf, const int* pix, int n_pix, float eps, int* kind, float* chain,
                          float* inner_rows, hipStream_t stream);
int nu_relight_thin_chain_dump(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* thickness, const float* curvature,
    const float* gbuf, const int* pix, int n_pix, float eps, int* kind, float* chain,
                               float* inner_rows, float* seg, float* aux, hipStream_t stream);
int nu_relight_thin_light(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* thickness, const float* curvature,
    const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count, int seed,
                          float eps, float* rec, hipStream_t stream);
int nu_relight_thin_light_dump(const void* bvh_o, int n_faces_o, const float* V_o, const int* F_o, const float* vnormals_o, const float* ior,
    const void* bvh_i, int n_faces_i, const float* V_i, const int* F_i, const float* vnormals_i, const float* materials_i,
    const float* thickness, const float* curvature,
    const float* inner_rows, const int* sel, int n_sel, int samples, int s0, int s_count,
                               int seed, float eps, float* rec, float* dump, hipStream_t stream);
int nu_relight_thin_cross(const float* d, const float* normal, const float* x, const float* ior, const float* thickness,
                          const float* curvature, int M, int inside, unsigned char* refracts, unsigned char* tir_ok, float* nrm,
                          float* pend, float* ns, float* nd, float* fres, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Validation metrics (network/metrics.py): PSNR and SSIM of uint8 images [n, h, w, c], channel-interleaved, c in {1, 3}.
 * Pointers need no alignment.  DESIGN.md section 18 has the exactness argument and the reduction order.
 * --------------------------------------------------------------------------------------------------------- */
/* color_map_backward (utils/base_utils.py:501-504): out = (uint8) clamp(x * 255, 0, 255) -- one fp32 multiply, truncation toward
 * zero; equal to numpy byte for byte on every finite input and on +-inf.  NaN gives 0 (numpy's cast of NaN is undefined). */
int nu_img_quantize(const float* x, long long count, unsigned char* out, hipStream_t stream);
/* ssd[i] = sum over the per_image bytes of image i of (a - b)^2, as an exact 64-bit integer (ssd is zeroed inside; integer
 * atomics, so the result does not depend on the order). */
int nu_img_sqdiff(const unsigned char* a, const unsigned char* b, int n, long long per_image, long long* ssd, hipStream_t stream);
/* skimage.metrics.structural_similarity(a[i], b[i], win_size=win, channel_axis=2, data_range=255): uniform win x win window,
 * sample covariance, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
 * on the (h - win + 1)(w - win + 1) windows that lie inside the image (skimage's crop), per channel.
 *   mssim [n]                                   the mean of S over windows and channels
 *   smap  [n, h - win + 1, w - win + 1, c]      S itself; NULL: not written
 * Window sums are exact integers, S is fp64, the mean is reduced in a fixed order: the same bits on every run, and for an image
 * whatever the batch it is in.  win must be odd, 3 <= win <= 15, win <= h, win <= w (anything else: NU_ERR_ARG; skimage raises).
 * `work` is a caller-owned buffer of nu_img_ssim_workspace_bytes(n, h, w, c) bytes (enough for every win).  n * ceil((h - win + 1)
 * / 16) * ceil((w - win + 1) c / 64) must stay below 2^31 (chunk over images). */
long long nu_img_ssim_workspace_bytes(int n, int h, int w, int c);
int nu_img_ssim(const unsigned char* a, const unsigned char* b, int n, int h, int w, int c, int win, double* mssim, double* smap,
                void* work, long long work_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Network-level entry points: one call sequences every kernel launch of a network pass from C++.
 *   nu_sdf_mlp_{fwd,normal,bwd}      SDFNetwork.forward / .gradient and their (double) backward   field.py:133-170
 *   nu_nerfpp_mlp_{fwd,bwd}          NeRFNetwork.forward / backward                               field.py:265-289
 *   nu_shading_stack_{fwd,bwd}       AppShadingNetwork.forward / backward                         field.py:684-777, :636-682
 * Buffers are the caller's (device pointers, layouts in DESIGN.md "Data layout in HBM"); NuLin holds one packed layer as
 * nu_pack_layers leaves it.  Split reductions (weight gradients, skinny heads, column sums) go to the arena of NuOpCtx and
 * are finished by nu_ctx_flush (or implicitly when the arena / descriptor list is full).  Bias gradients are written at
 * NuOpCtx.flat + NuLin.db_off (the flat gradient buffer nu_unpack_grads reads).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct NuLin {
    const float* Wp; const float* WpT; float* dWp; const float* bias;
    long long db_off;
    int N, K, Kp, ldT, ldd, pad_;
    const void* Wp16; const void* WpT16;  /* bf16 copies of Wp / WpT (NuPackDesc.Wp16 / WpT16); used when NuOpCtx.h16 */
} NuLin;

/* NuOpCtx.h16 != 0 (with prec == 1): bf16 STORAGE.  Every NT GEMM reads the bf16 weight tables and the hidden activations
 * that only GEMMs touch live in HBM as bf16; the caller allocates exactly these buffers as __bf16 (same shapes and leading
 * dimensions, in elements), everything else stays fp32:
 *   SDF      H[1..3], H[5..7] (and H[8] in the no-gradient form, want_feat == 0);  D[0..2], D[4..6];  Q[1..3], Q[5..7];
 *            C[l] / Aux[l] for l in {0,1,2,4,5,6}
 *   NeRF++   H[1..4], H[6..8];  dA[1..4], dA[6..8];  dH8a
 *   shading  M[0..2], dM[0..2];  hidden [0..2], tmp[0], tmp[1] and dH3 of every light predictor
 * Optional per-launch timing: when `ev` is set, every GEMM launch is bracketed by hipEventRecord on ev[nev], ev[nev + 1]
 * and described in ev_meta[nev / 2] = {kind (0 NT, 1 TN), algorithmic flops, algorithmic bytes} until ev_cap is reached. */
/* One queued weight gradient of a backward pass (nu_wgrad_defer): the problem, where its result goes, and its algorithmic cost
 * (roofline accounting of the launch that ends up carrying it). */
#define NU_WGRAD_QUEUE_MAX 32
typedef struct NuWgradItem {
    NuGemmTN g;
    float* dW; int ldw, pad_; long long sW;
    float* db; long long sDb;
    double flops, bytes;
} NuWgradItem;
int nu_wgrad_item_size(void);

typedef struct NuOpCtx {
    int prec, h16;                        /* NuGemmNT.bf16 arithmetic mode of every GEMM; bf16 storage */
    float* flat;                          /* flat gradient buffer of the current backward */
    float* arena; long long arena_floats; long long arena_off;
    NuReduceDesc* descs; int ndesc, cap;  /* HOST array of deferred reductions */
    void** ev; double* ev_meta; int nev, ev_cap;      /* HOST arrays: hipEvent_t handles, 3 doubles per launch */
    int forked, pad_;                     /* != 0 while ops of this context are in flight on MORE THAN ONE stream: a forced
                                             mid-step flush would reduce slabs another stream still writes and hand their space
                                             out again, so the entries return NU_ERR_WORKSPACE instead (fail closed) */
    NuWgradItem* pend; int npend, pend_cap;   /* HOST array: the weight gradients of the current pass, queued by nu_wgrad_defer and
                                             launched together by nu_wgrad_flush (NULL: every weight gradient launches at once) */
} NuOpCtx;
int nu_op_ctx_size(void);
/* launches the queued weight gradients, then the batched reductions of everything enqueued so far; resets the arena */
int nu_ctx_flush(NuOpCtx* ctx, hipStream_t stream);
/* the reductions only (queued weight gradients stay queued): frees the arena in the middle of a pass */
int nu_ctx_reduce(NuOpCtx* ctx, hipStream_t stream);
/* The weight gradients of a backward pass are independent of each other: a pass queues them and ONE launch per tile class carries
 * the whole queue (splits chosen for the queue as a whole; see csrc/gemm_tn.hip).  Operands must stay valid and unmodified until
 * the flush; every network-level entry below flushes before it returns.  flops / bytes: algorithmic cost for the event record. */
int nu_wgrad_defer(NuOpCtx* ctx, const NuGemmTN* g, float* dW, int ldw, long long sW, float* db, long long sDb, double flops,
                   double bytes, hipStream_t stream);
int nu_wgrad_flush(NuOpCtx* ctx, hipStream_t stream);

typedef struct NuSdfNet { NuLin lin[9]; } NuSdfNet;
typedef struct NuSdfBufs {
    int P, pad_;
    float *E, *U4, *YX, *sdf;             /* E [P,64]; U4 [P,256]; YX [P,288] (want_feat) or sdf [P] */
    float* H[9];                          /* H[1..8] [P,256] post-softplus, H[4] == U4 (inference: two ping-pong buffers) */
    float* D[8]; float* G0; float* n;     /* reverse sweep: delta_l [P,256], G0 [P,64], n [P,3] */
    float* Q[9]; float* C[8];             /* second-order: Q[0] [P,64], Q[1..8] [P,256] (Q[4] doubles as the skip slot), C_l [P,256] */
    float* Aux[8];                        /* abar_l [P,256] of a first-order-only backward */
    float* dE0;                           /* [P,64] (input gradient) */
} NuSdfBufs;
int nu_sdf_net_size(void);
int nu_sdf_bufs_size(void);
int nu_sdf_mlp_fwd(NuOpCtx* ctx, const NuSdfNet* net, const float* X, int x_ld, NuSdfBufs* bufs, int want_feat, hipStream_t stream);
/* The no-gradient forward as ONE fully-fused kernel (csrc/fused_sdf.hip): sdf[P] = SDFNetwork(x)[..., 0] for X [P, x_ld] (x = the
 * first three floats of a row), exact fp32, nothing kept -- embedding, the eight softplus layers and the sdf head with the
 * activations of a 32- or 64-point tile held in LDS and the weights streamed through it.  Bit-identical to nu_sdf_mlp_fwd(...,
 * want_feat = 0).  Serves the hierarchical sampler (renderer_zerothick.py:525-612: 64 + 3 x 16 queries per ray), the occlusion
 * probe (field.py:501-554), extract_fields (field.py:1286-1307) and the stage-2 inner up-sampler (renderer_zerothick.py:1742-1760). */
int nu_sdf_fused_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, hipStream_t stream);
/* the same in the bf16-STORAGE arithmetic (NuOpCtx.h16: bf16 weight tables NuLin.Wp16, activations rounded to bf16 between layers,
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation): bit-identical to nu_sdf_mlp_fwd(..., want_feat = 0) under h16 */
int nu_sdf_fused16_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, hipStream_t stream);
/* The second-order jet of the SDF as ONE fully-fused no-gradient kernel (csrc/sdf_jet.hip): value, gradient and Hessian in forward mode
 * (ten rows per point through the pipeline of nu_sdf_fused_fwd, exact fp32 on the fp32 packed tables in every mlp_dtype), and from them
 * the curvatures of the level set through each point, with g = grad f, H = Hessian f:
 *   mean = (|g|^2 tr H - g^T H g) / (2 |g|^3),  gauss = g^T adj(H) g / |g|^4,  normal = g / |g|     (f = |x| - r: 1 / r, 1 / r^2)
 * Where |g|^2 < 1e-12: mean = gauss = 0, normal = 0.
 *   X [P, x_ld] (x = the first three floats of a row, x_ld >= 3); sdf [P] (the bits of nu_sdf_fused_fwd), grad [P,3], hess [P,6] in the
 *   order xx, yy, zz, xy, xz, yz; mean, gauss [P]; normal [P,3].  Every output pointer may be NULL.  No workspace.
 *   NU_ERR_ARG: net or X NULL, P < 0, x_ld < 3.  P == 0 launches nothing. */
int nu_sdf_jet_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, float* grad, float* hess, float* mean,
                   float* gauss, float* normal, hipStream_t stream);
/* The FIRST-order jet of the SDF as ONE fully-fused no-gradient kernel (csrc/sdf_grad.hip): value, gradient and unit
 * normal, four rows per point (value, d/dx, d/dy, d/dz) through the pipeline of nu_sdf_jet_fwd, 16 points on all 64 rows of a tile where
 * the second-order jet has 6 on 60.  The bulk tool of the normal-map bake; exact fp32 on the fp32 packed tables in every mlp_dtype.
 *   X [P, x_ld] (x = the first three floats of a row, x_ld >= 3); sdf [P] (the bits of nu_sdf_fused_fwd), grad [P,3] and normal [P,3] =
 *   grad / |grad| (the bits of nu_sdf_jet_fwd; normal = 0 where |grad|^2 < 1e-12).  Every output pointer may be NULL.  No workspace.
 *   A point's outputs do not depend on P, on its position in X or on its neighbours.
 *   NU_ERR_ARG: net or X NULL, P < 0, x_ld < 3.  P == 0 launches nothing. */
int nu_sdf_grad_fwd(const NuSdfNet* net, const float* X, int x_ld, int P, float* sdf, float* grad, float* normal, hipStream_t stream);
/* Sphere tracing of the SDF as ONE fully-fused no-gradient kernel (csrc/sdf_trace.hip; network/tracing.py:103-164 called on each ray
 * alone): persistent workgroups hold 64 ray slots in LDS, run the pipeline of nu_sdf_fused_fwd on the slot positions, apply the step
 * behind the head and refill finished slots from a statically assigned ray sequence.  Per ray, every operation a separately rounded
 * fp32 multiply / add / divide / square root in this order (f = the bits of nu_sdf_fused_fwd, Rb = bound_radius):
 *   fgr = finite(o) && (fg == NULL || fg[r]);  x = o;  t = 0
 *   if Rb > 0:  a = (d0 d0 + d1 d1) + d2 d2;  b = 2 ((d0 o0 + d1 o1) + d2 o2);  c = ((o0 o0 + o1 o1) + o2 o2) - Rb Rb
 *               disc = b b - (4 a) c;  bounded = disc >= 0;  t0 = (-b - sqrt(disc)) / (2 a)
 *               flags & NU_TRACE_ENTRY_FORWARD: t0 = max(t0, 0)   (off, the reference: an origin inside the sphere steps BACK to its entry)
 *               if bounded: x = o + d t0, t = t0;   fgr &= bounded
 *   for i < max_iter while fgr:  s = clamp(f(x), -10, 10), NaN -> 10;  x = x + d s;  t = t + s;  iters = i + 1;  sdf_last = s
 *               if Rb > 0: fgr &= sqrt((x0 x0 + x1 x1) + x2 x2) < Rb;   conv = |s| < threshold;   stop when conv or !fgr
 *   hit = conv && fgr;  pos, t = x, t as left.  A ray that never was foreground: pos = o, t = 0, iters = 0, sdf_last = 0, hit = 0.
 *   O [R, o_ld], D [R, d_ld] (the first three floats of a row; leading dimensions >= 3), fg [R] bytes or NULL; pos [R,3], t [R],
 *   sdf_last [R], iters [R] int, hit [R] bytes (0 / 1).  Every output pointer may be NULL.  No workspace, no host read.  A ray's result
 *   does not depend on its neighbours, the ray order or the grid.  Reads the fp32 packed tables (every mlp_dtype has them).
 *   NU_ERR_ARG: net, O or D NULL, R < 0, a leading dimension < 3, max_iter < 1, threshold not > 0.  R == 0 launches nothing. */
#define NU_TRACE_ENTRY_FORWARD 1
int nu_sdf_trace(const NuSdfNet* net, const float* O, int o_ld, const float* D, int d_ld, int R, const unsigned char* fg,
                 int max_iter, float threshold, float bound_radius, int flags, float* pos, float* t, float* sdf_last, int* iters,
                 unsigned char* hit, hipStream_t stream);
int nu_sdf_mlp_normal(NuOpCtx* ctx, const NuSdfNet* net, NuSdfBufs* bufs, hipStream_t stream);
int nu_sdf_mlp_bwd(NuOpCtx* ctx, const NuSdfNet* net, NuSdfBufs* bufs, const float* dYX, const float* nbar, float* dx,
                   hipStream_t stream);

typedef struct NuNerfNet { NuLin pts[8]; NuLin feat, alpha, view, rgb; } NuNerfNet;
typedef struct NuNerfBufs {
    int P, pad_;
    float* H[9];                          /* H[0] = E4 [P,96]; H[i] = input of layer i ([P,256]; H[5] = U5 [P,352]); H[8] last hidden */
    unsigned long long* mask[9];          /* ReLU sign bits of H[1..8] */
    float *V, *HV, *sig, *rgb;            /* V [P,288] = feature | view embedding; HV [P,128]; raw heads sig [P], rgb [P,4] */
    float *dHV, *dF, *dH8a;               /* backward: [P,128], [P,256|288], [P,256] */
    float* dA[9];                         /* dA[i] = d pre-activation of layer i-1's output, i = 1..8 ([P,256]; dA[5] [P,352] with dx) */
    float *dE4, *dx, *ddir;               /* input gradients (stage 2): [P,96], [P,3], [P,3]; dx == NULL: parameters only */
} NuNerfBufs;
int nu_nerf_net_size(void);
int nu_nerf_bufs_size(void);
int nu_nerfpp_mlp_fwd(NuOpCtx* ctx, const NuNerfNet* net, const float* pt, int pt_ld, NuNerfBufs* bufs, hipStream_t stream);
int nu_nerfpp_mlp_bwd(NuOpCtx* ctx, const NuNerfNet* net, const float* pt, int pt_ld, NuNerfBufs* bufs, const float* dsig,
                      const float* drgb, hipStream_t stream);
/* The learned NeRF++ background of R rays as ONE fully-fused no-gradient kernel (csrc/background.hip): color_bkgr of render_core
 * (renderer_zerothick.py:757, :777-779), the front-to-back composite of a ray's samples with every inner (|x| <= 1) alpha zero, without
 * point records, workspace or host read.  Per ray r and sample j < S, every operation a separately rounded fp32 one unless stated:
 *   du = d / max(|d|, 1e-12)                                        (partition_write_kernel; |d|^2 = d2 d2 + fma(d1, d1, d0 d0))
 *   dist_j = z_{j+1} - z_j (the last section repeats its predecessor; 0 for S == 1);  mid_j = z_j + 0.5 dist_j;  x_j = o + d mid_j
 *                                                                   (nu_sample_point of csrc/render.hip: d as given, not du)
 *   live_j = !(sqrt((x0 x0 + x1 x1) + x2 x2) <= 1) && (t_stop == NULL || mid_j < t_stop[r])
 *   input row: embed((x / |x|, 1 / |x|), L = 10) = 84 columns padded to 96 and embed(-du, L = 4) = 27 columns padded to 32, the
 *              arithmetic of nerf_embed_kernel (|x|^2 = x2 x2 + fma(x1, x1, x0 x0))
 *   layers:    eight 256-wide ReLU layers, the input row concatenated behind the hidden row at layer 5 (U5 = [h (256) | E4 (96)], K = 352);
 *              sig = alpha_linear(h8) as nu_skinny_fwd <1, 256>;  feat = feature_linear(h8), no activation;
 *              hv = ReLU(views_linears.0([feat | view (32)])), 288 -> 128;  raw = rgb_linear(hv) as nu_skinny_fwd <3, 128>.
 *              Exact fp32 on v_mfma_f32_32x32x2f32 in the k order of nu_gemm_nt: the bits of nu_nerfpp_mlp_fwd (fp32 mode).
 *   activation (nerf_act_fwd_kernel):  alpha_j = live_j ? 1 - expf(-softplus1(sig) dist_j) : 0;   c_j = srgb(expf(fminf(raw, 5)))
 *   composite, in sample order j = 0 .. S - 1 starting from T = 1, color = 0:
 *              color += (alpha_j T) c_j;   T *= fl(fl(1 - alpha_j) + 1e-7)        (no step fused; a sample that is not live still
 *              multiplies T by fl(1 + 1e-7), as the reference's cumprod does);   trans = T after the last sample.
 *   O [R, o_ld], D [R, d_ld] (the first three floats of a row; leading dimensions >= 3), z [R, S] ascending nodes, S >= 1, t_stop [R] or
 *   NULL; color [R,3], trans [R].  Test outputs, rows in (ray, sample) order, zero on rows that are not live: enc_dbg [R S, 128] = the 96
 *   input columns and the 32 view columns, raw_dbg [R S, 4] = sig, raw rgb, act_dbg [R S, 4] = alpha, c.  Every output pointer may be
 *   NULL.  A ray's result does not depend on R, the ray's position, its neighbours or the grid.  Reads the fp32 packed tables (every
 *   mlp_dtype has them) and nothing behind the 128 rows of the view layer's.
 *   NU_ERR_ARG: net, O, D or z NULL, R < 0, S < 1, a leading dimension < 3, tables that are not the NeRF++ of NuNerfNet (pts 84 -> 256,
 *   256 x 3, the 340-wide skip layer at index 5, 256 x 2, feat 256, alpha 1, view 283 -> 128, rgb 3).  R == 0 launches nothing. */
int nu_background_fwd(const NuNerfNet* net, const float* O, int o_ld, const float* D, int d_ld, const float* z, int S,
                      const float* t_stop, int R, float* color, float* trans, float* enc_dbg, float* raw_dbg, float* act_dbg,
                      hipStream_t stream);

typedef struct NuShadeNet {
    const float *WpM0, *WpTM0, *bM0; float* dWpM0;                  /* materials layer 0, 4 predictors side by side (N = 1024) */
    const float* WpM[3]; const float* WpTM[3]; const float* bM[3]; float* dWpM[3];      /* [1], [2]: grouped x4 */
    long long dbM_off[3];
    const float *Ws6, *b6; float* dWs6; long long db6_off;          /* block-diagonal 6-wide head */
    NuLin outer_light[4], inner_light[4], inner_weight[4], refrac_light[4];
    const float* lut;
    float exp_max; int sphere, ld_ol, refrac_dim, ld_rl, pad_;
    const void *WpM0_16, *WpTM0_16; const void* WpM16[3]; const void* WpTM16[3];     /* bf16 copies (NuOpCtx.h16) */
} NuShadeNet;
typedef struct NuShadeBufs {
    int P, R;                             /* inner points; per-ray mirror queries riding along the outer_light batch */
    const float *extra_dirs, *extra_pts;
    float* M[3]; unsigned long long* maskM[3]; float* Mraw;         /* materials hidden [P,1024] x3, raw heads [P,8] */
    float *OLin, *ILin, *IWin, *RLin, *SD;                          /* predictor inputs, shading directions [P,8] */
    float* OLh[3]; float* ILh[3]; float* IWh[3]; float* RLh[3];     /* hidden activations [rows,256] */
    unsigned long long* maskOL[3]; unsigned long long* maskIL[3]; unsigned long long* maskIW[3]; unsigned long long* maskRL[3];
    float *OLo, *ILo, *IWo, *RLo, *aux;                             /* raw heads, aux [P,4] */
    float *dMraw, *dOLo, *dILo, *dIWo, *dRLo, *dNoV;                /* backward of the combine */
    float* dH3[4]; float* tmpOL[2]; float* tmpIL[2]; float* tmpIW[2]; float* tmpRL[2];
    float *dOLin, *dILin, *dn; float* dM[3]; float* dYX;
} NuShadeBufs;
int nu_shade_net_size(void);
int nu_shade_bufs_size(void);
int nu_shading_stack_fwd(NuOpCtx* ctx, const NuShadeNet* net, NuShadeBufs* bufs, const float* YX, const float* E, const float* nrm,
                         const float* pt, const int* idx, float* color_rm, hipStream_t stream);
/* stage 0: combine backward only (fills dMraw, dOLo, dILo, dIWo, dRLo, dNoV); stage 1: everything after it */
int nu_shading_stack_bwd(NuOpCtx* ctx, const NuShadeNet* net, NuShadeBufs* bufs, const float* YX, const float* nrm, const float* pt,
                         const int* idx, const float* dcolor_rm, int stage, hipStream_t stream);

/* Per-vertex material baking (predict_materials, network/renderer_zerothick.py:846-864; the arrays relight_backend.py:26-28 reads)
 * as ONE fully-fused no-gradient kernel (csrc/bake.hip): x -> embedding -> SDF network -> [sdf | feature | x] kept in LDS -> the
 * material predictors (288 -> 256 -> 256 -> 256 ReLU -> head) -> sigmoid.  Exact fp32 in the k order of the layered path
 * (nu_sdf_mlp_fwd(..., want_feat = 1) + the materials part of nu_shading_stack_fwd): sdf, feature columns and raw heads are
 * bit-identical to it.  NuBakeNet: the SDF network's layers plus the packed material tables as NuShadeNet holds them (4 predictors
 * side by side: metallic, roughness, albedo, transmission weight; n_pred = 3 for a network without the last).
 *   X [P, x_ld] (x = the first three floats of a row, x_ld >= 3); metallic, roughness [P]; albedo [P,3]; transmission, sdf [P].
 *   Every output pointer may be NULL; a predictor whose output is NULL is not evaluated.  P <= 0 returns at once.
 *   Debug / test fields: feat != NULL also writes the feature columns [P,256]; raw != 0 writes the heads before the sigmoid. */
typedef struct NuBakeNet {
    NuSdfNet sdf;
    const float *WpM0, *bM0;                        /* [256 n_pred, 288], [256 n_pred] */
    const float* WpM[3]; const float* bM[3];        /* [1], [2]: [n_pred, 256, 256], [n_pred, 256] */
    const float *Ws6, *b6;                          /* block-diagonal heads [6, 1024], [6] */
    float* feat;
    int n_pred, raw;
} NuBakeNet;
int nu_bake_net_size(void);
int nu_material_bake_fwd(const NuBakeNet* net, const float* X, int x_ld, int P, float* metallic, float* roughness, float* albedo,
                         float* transmission, float* sdf, hipStream_t stream);

/* The illumination the shading network learned, for a caller's directions, as ONE fully-fused no-gradient kernel (csrc/light_bake.hip;
 * predict_specular_lights with reflective = d and no human light, network/field.py:636-667, :1399-1430).  Row p = (direction
 * dirs[p] [N,3], roughness kinv[p] = the kappa_inv of nu_ide, point): x == NULL is the origin for every row, x_stride == 0 the one
 * point x[0..2] for every row, otherwise row p reads x + p * x_stride (x_stride >= 3).
 *   probe == 0: light = direct = exp(min(outer_light([IDE(d, rho) | IDE(sph(x, d), rho) if net->sphere]), exp_max)); the input row is
 *               the one nu_spec_encode writes (net->ld_ol columns) at the row's roughness.
 *   probe != 0 (needs x): indirect = exp(min(inner_light([pos_enc(x) | IDE(d, rho)]), exp_max)) * occ,
 *               occ = clamp(0.5 inner_weight([pos_enc(x) | dir_enc(d)]) + 0.5, 0, 1), light = indirect + direct (1 - occ); pos_enc has
 *               pos_freq <= 8 frequencies, the input rows are ILin / IWin of nu_s2_shade_encode_fwd.
 *   light, direct, indirect [N,3]; occ [N]; every output pointer may be NULL.  Exact fp32 in the k order of the layered path
 *   (nu_gemm_nt + nu_skinny_fwd): the raw heads are bit-identical to it.  It reads the fp32 packed tables only.
 *   Test outputs: enc_dbg [N, ld_ol (+ 128 + 96 with probe)] the encoded rows, raw_dbg [N,8] the heads before their activations
 *   (direct 3, indirect 3, occlusion 1, 0).
 *   NU_ERR_ARG: net / dirs / kinv NULL, N < 0, probe without x, 0 < x_stride < 3, tables that are not the 3 x 256 predictors.
 *   N == 0 launches nothing. */
int nu_light_bake_fwd(const NuShadeNet* net, const float* dirs, const float* kinv, const float* x, int x_stride, int pos_freq, int N,
                      int probe, float* light, float* direct, float* indirect, float* occ, float* enc_dbg, float* raw_dbg,
                      hipStream_t stream);

/* The appearance the shading network learned, at a caller's surface points, as ONE fully-fused no-gradient kernel
 * (csrc/surface_shade.hip): AppShadingNetwork.forward in its stage-1 form (network/field.py:684-777; AppShadingNetwork_SpecInner is the
 * same form) on explicit rows -- n^, v^, NoV, r = 2 NoV n^ - v^, rho = sigmoid(Mraw[:, 1]); the seven predictor rows outer_light x 3
 * (IDE(n^, 1) | IDE(r, rho) | IDE(r, 0), + the sphere points with net->sphere), inner_light x 2, inner_weight, refrac_light;
 * exp(min(., exp_max)); occlusion mix; split-sum FG table (bilinear, clamp); Schlick; transmission mix; sRGB.  One launch for any P, no
 * workspace, no host read; it reads the fp32 packed tables only.
 *   X [P, x_ld] the point, V [P, v_ld] the view direction TOWARDS the camera, Nrm [P, n_ld] the normal (neither is normalised by the
 *   caller; the first three floats of a row, every leading dimension >= 3); Mraw [P, ldm >= 6] the raw material heads in the layered
 *   layout (metallic, roughness, albedo x 3, transmission).  pos_freq: the network's light_pos_freq (<= 8).  refrac_exp_max: the cap
 *   shade() applies to the raw refrac_light head of AppShadingNetwork_SpecInner (-0.2); pass net->exp_max for no extra cap.
 *   flags & NU_SHADE_LINEAR: `color` skips linear_to_srgb.
 *   Outputs, every pointer may be NULL: color [P,3]; the validation images of field.py:751-770 BEFORE their display clamps, sRGB
 *   applied where the reference applies it: diffuse_color = srgb(diffuse), specular_color = srgb(specular) (1 - T) + F light0 T,
 *   indirect_light = indirect occ (linear), refraction_light = srgb((1 - F) refraction T) [P,3], occ_prob = 0.5 raw + 0.5,
 *   reflection_weight = F [P]; and the two light images LINEAR: diffuse_light = exp(min(outer_light(IDE(n^, 1)), exp_max)),
 *   specular_light = light0, the blended roughness-0 specular light (the reference's pictures are clamp(srgb(.)) of them).
 *   The human-light stack is NEVER evaluated: for a model trained with shader_config.human_light the photographer's term is left
 *   out (human_weight = 0), as nu_light_bake_fwd leaves it out.
 *   Exact fp32 in the k order of the layered path: the encoded rows are the bits of nu_s2_shade_encode_fwd, the raw heads those of
 *   nu_gemm_nt + nu_skinny_fwd, the colour those of nu_shade_combine_fwd on them.
 *   Test outputs: enc_dbg [P, 3 ld_ol + 2 * 128 + 96 + ld_rl]: per point its OLin rows (diffuse | specular | mirror), ILin rows
 *   (specular | mirror), IWin row and RLin row; raw_dbg [P,20]: the heads before activation in the same order (3 3 3 3 3 1 3, then 0).
 *   NU_ERR_ARG: net / X / V / Nrm / Mraw NULL, P < 0, a leading dimension < 3, ldm < 6, unknown flags, pos_freq that is not the
 *   network's (or > 8), tables that are not the four 3 x 256 predictors with the rows above, no FG table.  P == 0 launches nothing. */
#define NU_SHADE_LINEAR 1
int nu_surface_shade_fwd(const NuShadeNet* net, const float* X, int x_ld, const float* V, int v_ld, const float* Nrm, int n_ld,
                         const float* Mraw, int ldm, int P, int pos_freq, float refrac_exp_max, int flags, float* color,
                         float* diffuse_color, float* specular_color, float* diffuse_light, float* specular_light, float* indirect_light,
                         float* refraction_light, float* occ_prob, float* reflection_weight, float* enc_dbg, float* raw_dbg,
                         hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fused loss assembly: from the renderer's per-ray outputs to the scalar the trainer back-propagates, for
 * the loss set of the shipped stage-1 configs -- white background + clamp (renderer_zerothick.py:783-787), charbonier RGB
 * loss (:501-513), colour_spec activation (:780-781), NeRFRenderLoss / EikonalLoss / OuterRegLoss / NormalOrientationLoss
 * (network/loss.py:26-48, :194-213) and the trainer's sum of means (train/trainer_zero.py:153-161).
 *   rgb, rgb_bg, spec_raw, gt [R,3]; acc, nrm_sum (optional) [R]; gerr [P] (P = 0: no inner point); cand (optional) u8[R]:
 *   rays that take part in the outer regulariser.  Weights of inactive terms are passed as 0.
 *   terms[6] = {loss_rgb, loss_eikonal, loss_outer_reg, loss_normal, their sum, candidate count}; per-ray outputs
 *   ray_rgb / color_spec [R,3], loss_rgb [R].  nu_loss_bwd reads the upstream gradient from device memory.
 *   point_weight (optional device scalar, NULL = 1): factor on the eikonal mean and its gradient -- under data parallelism
 *   this rank's share n_local * world / sum_r n_r of the mean over all ranks' inner points, so the N > 1 step
 *   runs the same fused assembly as the N = 1 step.
 * --------------------------------------------------------------------------------------------------------- */
long long nu_loss_workspace_bytes(int R, int P);
int nu_loss_fwd(const float* rgb, const float* acc, const float* rgb_bg, const float* spec_raw, const float* gerr,
                const float* nrm_sum, const float* gt, const unsigned char* cand, int R, int P, int white_bg, float exp_max,
                float w_eik, float w_reg, float w_nrm, float* ray_rgb, float* color_spec, float* loss_rgb, float* terms,
                const float* point_weight, void* workspace, long long workspace_bytes, hipStream_t stream);
int nu_loss_bwd(const float* rgb, const float* acc, const float* rgb_bg, const float* spec_raw, const float* gt,
                const unsigned char* cand, const float* ray_rgb, const float* color_spec, const float* loss_rgb,
                const float* terms, const float* upstream, const float* point_weight, int R, int P, int white_bg, float exp_max,
                float w_eik, float w_reg, float w_nrm, float* d_rgb, float* d_acc, float* d_rgb_bg, float* d_spec_raw, float* d_gerr, float* d_nrm,
                hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stage 2 (zero-thickness Stage2Renderer, network/renderer_zerothick.py:1571-2011): kernels of the renderer's own logic.
 * A segment is a set of N rays with S1 nodes x_{n,j} = start_n + v_n * z_{n,j}; its S = S1 - 1 samples sit at the nodes
 * j < S, section length |x_{j+1} - x_j| (the last one repeats its predecessor).
 *   nu_s2_seg_count / nu_s2_seg_write   outer samples (|x| > 1) compacted in (ray, sample) order into 32-byte point records
 *                                       (x, dist, dir) for nu_nerfpp_mlp_fwd; idx = ray-major scatter target (idx_base + n S + j),
 *                                       pos_rm = compact index per (ray, sample) or -1          (:1835-1870)
 *   nu_s2_ddist                         d alpha / d dist of compute_density_alpha               (:1531-1540)
 *   nu_s2_seg_bwd                       cotangents of the point records -> d start, d v, d dirs
 *   nu_s2_composite_fwd / _bwd          linear-RGB composite with the running transmittance     (:1976-1990); colour [N,S,4] sRGB
 *   nu_s2_refract_fwd / _bwd            Snell refraction / total internal reflection per hit ray (:1642-1684)
 * --------------------------------------------------------------------------------------------------------- */
int nu_s2_seg_count(const float* start, const float* v, const float* z, int N, int S1, int* cnt, int* off, int* total, hipStream_t stream);
int nu_s2_seg_write(const float* start, const float* v, const float* z, const float* dirs, int N, int S1, const int* off, int pt_base,
                    int idx_base, float* pt, int* idx, int* pos_rm, hipStream_t stream);
int nu_s2_ddist(const float* sigma, const float* pt, const int* idx, int P, const float* dalpha_rm, float* ddist, hipStream_t stream);
int nu_s2_seg_bwd(const float* start, const float* v, const float* z, int N, int S1, int idx_base, const int* pos_rm, const float* dx,
                  const float* ddist, const float* ddir, float* dstart, float* dv, float* ddirs, hipStream_t stream);
int nu_s2_composite_fwd(const float* alpha, const float* color, const float* Tin, int N, int S, float* out, float* Tout, hipStream_t stream);
int nu_s2_composite_bwd(const float* alpha, const float* color, const float* Tin, int N, int S, const float* dout, const float* dTout,
                        float* dalpha, float* dcolor, float* dTin, hipStream_t stream);
int nu_s2_refract_fwd(const float* d, const float* nrm, const float* ior, const float* point, int M, int outside, unsigned char* flag,
                      float* eta, float* nd, float* ns, hipStream_t stream);
int nu_s2_refract_bwd(const float* d, const float* nrm, const float* ior, int M, int outside, const float* g_nd, const float* g_ns,
                      const float* g_eta, float* dd, float* dn, float* dior, float* dpoint, hipStream_t stream);
/*   nu_s2_shade_encode_fwd / _bwd       inputs of the shading stacks for explicit points / normals / view directions [P,3] (stage 2:
 *                                       AppShadingNetwork, _S2, _SpecInner; field.py:636-682, :828-907, :1399-1445): n^, v^, NoV,
 *                                       r = 2 NoV n^ - v^, rho = sigmoid(Mraw[:,1]);  OLin [3P, ld_ol] IDE rows (+ sphere points when
 *                                       `sphere`), ILin [2P,128] = [pe(x) | IDE], IWin [P,96] = [pe(x) | embed(r,6)], RLin [P, ld_rl]
 *                                       = [embed(x, rf) | embed(v^, rf)] (refrac_freq < 0: none), SD [P,12] = n^, NoV, 1/|n|, rho,
 *                                       1/|v|, 0, r, 0; pe(x) has pos_freq frequencies (6 or 8).  _bwd: cotangents of OLin / ILin /
 *                                       RLin / NoV (each may be NULL) -> d x, d n, d v [P,3] and d Mraw[:,1] [P] -- the stage-1 pair
 *                                       nu_shade_encode_* returns d n and d rho only. */
int nu_s2_shade_encode_fwd(const float* x, const float* nrm, const float* view, const float* Mraw, int ldm, int P, int sphere, int pos_freq,
                           int ld_ol, int refrac_freq, int ld_rl, float* OLin, float* ILin, float* IWin, float* RLin, float* SD,
                           hipStream_t stream);
int nu_s2_shade_encode_bwd(const float* x, const float* nrm, const float* view, const float* SD, int P, int sphere, int pos_freq, int ld_ol,
                           int refrac_freq, int ld_rl, const float* dOLin, const float* dILin, const float* dRLin, const float* dNoV,
                           float* dx, float* dn, float* dv, float* drho_raw, hipStream_t stream);
/*   nu_s2_shell_fwd / _bwd              thin-shell refraction of the NON-zero-thickness stage-2 model (network/renderer.py:1692-2032,
 *                                       Stage2Renderer.ray_trace): per hit ray the two refractions through a shell of learned thickness
 *                                       whose faces are concentric spheres of the local curvature radius.  In: d, raw interpolated
 *                                       normal, hit point [M,3], raw IoR / thickness network outputs and Gaussian curvature [M];
 *                                       `inside`: the ray leaves the object.  Out: refracts / tir_ok flags [M] u8, eta [M] (the first
 *                                       face's ratio), unit normal facing the ray, end point of the incoming segment, next origin, next
 *                                       direction [M,3].  _bwd: cotangents of the four [M,3] outputs (each may be NULL) -> d d, d normal,
 *                                       d point, d ior, d g_k, d thickness (a 12 x 12 forward-mode Jacobian per ray in registers). */
int nu_s2_shell_fwd(const float* d, const float* nraw, const float* p, const float* ior_raw, const float* gk, const float* th_raw, int M,
                    int inside, unsigned char* refracts, unsigned char* tir_ok, float* eta, float* nrm, float* pend, float* ns, float* nd,
                    hipStream_t stream);
int nu_s2_shell_bwd(const float* d, const float* nraw, const float* p, const float* ior_raw, const float* gk, const float* th_raw, int M,
                    int inside, const float* g_nrm, const float* g_pend, const float* g_ns, const float* g_nd, float* g_d, float* g_nraw,
                    float* g_p, float* g_ior, float* g_gk, float* g_th, hipStream_t stream);
/*   nu_s2_hit_fwd / _bwd                differentiable Moeller-Trumbore + vertex-normal interpolation of the rays that hit
 *                                       (Scene.Dintersect, network/DiffRender.py:61-125): face [M] int64 from nu_lbvh_trace, faces [F,3]
 *                                       int64, verts / vnrm [V,3] constants; backward -> d o, d d
 *   nu_s2_far_points / _far_resample    importance pass of the rays that miss the mesh (:1786-1812, no gradient): 192 coarse nodes
 *                                       -> point records; alpha [M,192] -> 64 inverse-CDF samples merged in: zout [M,256] sorted */
int nu_s2_hit_fwd(const float* o, const float* d, const long long* face, const float* verts, const float* vnrm, const long long* faces,
                  int M, float* point, float* nrm, float* t, const float* vcurv /* optional [V]: per-vertex Gaussian curvature */,
                  float* gk /* [M]: its barycentric interpolation (DiffRender.py:116) */, hipStream_t stream);
int nu_s2_hit_bwd(const float* o, const float* d, const long long* face, const float* verts, const float* vnrm, const long long* faces,
                  int M, const float* g_point, const float* g_nrm, const float* g_t, float* g_o, float* g_d, const float* vcurv,
                  const float* g_gk, hipStream_t stream);
int nu_s2_far_points(const float* start, const float* dirs, const float* zo, int M, int S, float* pt, int* idx, hipStream_t stream);
int nu_s2_far_resample(const float* alpha, const float* zo, int M, int S, int n_new, float* zout, hipStream_t stream);
/*   nu_s2_shade_combine_fwd / _bwd      AppShadingNetwork_S2.forward's BRDF mix (field.py:909-1010) on raw head outputs, layouts as
 *                                       nu_shade_combine_*: colour = (diffuse + specular)(1 - T) + F light0 T (x 0 when `internal`),
 *                                       rc [P] = (1 - F) T */
/*   nu_s2_neus_alpha_fwd / _bwd          NeuS alpha of the inner segment on explicit points (renderer_zerothick.py:1897-1915): sdf, unit
 *                                       normal, direction, section length, inv_s [1] on device; backward -> d sdf, d n, d d, d dist and
 *                                       the per-point share of d inv_s */
int nu_s2_neus_alpha_fwd(const float* sdf, const float* nrm, const float* dir, const float* dist, const float* inv_s, float cos_anneal,
                         int P, float* alpha, hipStream_t stream);
int nu_s2_neus_alpha_bwd(const float* sdf, const float* nrm, const float* dir, const float* dist, const float* inv_s, float cos_anneal,
                         int P, const float* g_alpha, float* g_sdf, float* g_nrm, float* g_dir, float* g_dist, float* g_s,
                         hipStream_t stream);
int nu_s2_shade_combine_fwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo, const float* SD,
                            const float* lut, const int* idx, int P, float exp_max, int internal, float* color_rm, float* rc,
                            hipStream_t stream);
int nu_s2_shade_combine_bwd(const float* Mraw, int ldm, const float* OLo, const float* ILo, const float* IWo, const float* SD,
                            const float* lut, const int* idx, int P, float exp_max, int internal, const float* dcolor_rm, const float* d_rc,
                            float* dMraw, float* dOLo, float* dILo, float* dIWo, float* dNoV, hipStream_t stream);


/* ---------------------------------------------------------------------------------------------------------
 * Trainer glue: torch.optim.Adam's update (train/trainer_zero.py:74-85, lr from
 * train/lr_common_manager.py:22-46) over many parameter tensors in one launch per NU_ADAM_MAX tensors.
 * p, g, m (exp_avg), v (exp_avg_sq): contiguous fp32 of n elements; step >= 1 is the count AFTER this update.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_ADAM_MAX 80
typedef struct NuAdamDesc {
    float* p; const float* g; float* m; float* v;
    long long n;
    int blk_begin, pad_;                      /* filled by the library */
} NuAdamDesc;
int nu_adam_desc_size(void);
int nu_adam_step(const NuAdamDesc* descs_host, int n, double lr, double beta1, double beta2, double eps, int step,
                 hipStream_t stream);   /* hyper-parameters in double: 1 - beta and the bias corrections are formed as torch forms them */

/* ---------------------------------------------------------------------------------------------------------
 * Mesh extraction (extract_mesh_stage1.py / _stage2.py: extract_geometry, network/field.py:1286-1317 -- PyMCubes on a host grid).
 * Grid u[nx][ny][nz] fp32, C order (point p = (i ny + j) nz + k), nx, ny, nz >= 2; the workspace (nu_mc_workspace_bytes, 8-byte
 * aligned) carries per-brick counts and offsets from one call to the next and must stay untouched in between.
 *   nu_mc_count             per-brick vertex / triangle counts (a corner is inside when u < iso; tables: csrc/mc_tables.h)
 *   nu_mc_scan              exclusive offsets of those counts; totals[2] (device, int64) = (Nv, Nf) -- the caller's one host read
 *   nu_mc_write_vertices    V [Nv,3] in index space, ordered by (owner point, axis): point p owns its +x, +y, +z edges, a straddling
 *                           edge gives one vertex at p + t e_axis, t = (iso - u_p) / (u_{p+e} - u_p); first_vid [nx ny nz] int32 gets
 *                           the first vertex id of every owner (other entries are not written)
 *   nu_mc_write_triangles   F [Nf,3] int32 ordered by (cell, table slot), normals (right-handed) towards u < iso
 * Grid compaction for the SDF evaluation of a dense grid at points (X[i], Y[j], Z[k]) (extract_fields, field.py:1286-1307): a point is
 * evaluated iff NOT torch.norm(x) >= 1, with torch's arithmetic ((x^2 + z^2) + y^2, correctly rounded sqrt).  Same workspace layout.
 *   nu_grid_inside_count    counts + scan; chunk_rows[c] (device, int64, c = 0 .. ceil(npts / chunk_points)) = first compact row of the
 *                           chunk of points [c chunk_points, (c+1) chunk_points); the last entry is the inside total.  chunk_points % 256 == 0
 *   nu_grid_compact         the inside points of [p0, p0 + n) (p0 % 256 == 0) as x rows [P,3] in point order, row 0 = first inside point
 *   nu_grid_scatter         u[p] = val[row of p] for the inside points of [p0, p0 + n), outside_val for the others
 * --------------------------------------------------------------------------------------------------------- */
long long nu_mc_workspace_bytes(int nx, int ny, int nz);
int nu_mc_count(const float* u, int nx, int ny, int nz, float iso, void* workspace, long long workspace_bytes, hipStream_t stream);
int nu_mc_scan(int nx, int ny, int nz, void* workspace, long long workspace_bytes, long long* totals, hipStream_t stream);
int nu_mc_write_vertices(const float* u, int nx, int ny, int nz, float iso, const void* workspace, long long workspace_bytes, float* V,
                         int* first_vid, hipStream_t stream);
int nu_mc_write_triangles(const float* u, int nx, int ny, int nz, float iso, const void* workspace, long long workspace_bytes,
                          const int* first_vid, int* F, hipStream_t stream);
int nu_grid_inside_count(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long chunk_points, void* workspace,
                         long long workspace_bytes, long long* chunk_rows, hipStream_t stream);
int nu_grid_compact(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long p0, long long n,
                    const void* workspace, long long workspace_bytes, float* rows, hipStream_t stream);
int nu_grid_scatter(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, long long p0, long long n,
                    const void* workspace, long long workspace_bytes, const float* val, float outside_val, float* u, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Block-sparse mesh extraction (csrc/mcubes_sparse.hip): the same lattice (X[i], Y[j], Z[k]), cut into point-blocks of
 * block^3 points (block = 4 or 8; block (bi, bj, bk) owns [block bi, block bi + block) per axis, id = (bi nby + bj) nbz + bk, int32,
 * nb* = ceil(n* / block)).  slot [nbx nby nbz] int32: -1 = inactive, else the block's slot (ascending block id); blocks [nslots] int32:
 * block id of every slot; u [nslots][block^3] fp32, in-block C order (rows r = slot block^3 + t, 64-bit).
 *   nu_smc_regions          per block, from its REGION (the lattice box [block b - 1, block b + block] clipped to the grid): flags
 *                           [nblk] int32 (0 = no point can lie in the unit ball, 1 = wholly inside, 2 = rim), probe [nblk,3] (the
 *                           region's centre, pulled radially to |p| = 0.999 when farther out), radius [nblk] (half diagonal +
 *                           |centre - probe|, times 1 + 1e-6).  Computed in double, stored in fp32; zero where flags is 0
 *   nu_smc_activate         active[probe_blocks[i]] = the rule for the level set at iso on the probe values f[i] (and g[i], or NULL); with
 *                           f' = f - iso: interior |f'| <= L r, rim f' <= L r (needs outside_val > iso); composite (g where f < 0, 1
 *                           elsewhere; iso < 1), with g' = g - iso: f <= L r and (|g'| <= L r [rim: g' <= L r] or (|f| <= L r and
 *                           g' <= L r)); L = +inf activates every probed block.  L r is one fp32 product; a NaN value activates
 *   nu_smc_block_rows       x rows [n,3] of the block points r0 .. r0 + n (indices beyond the grid clamped)
 *   nu_smc_finish           u[r] = outside_val at the points that fail the inside test of nu_grid_compact (and at the padding)
 *   nu_smc_count / _scan / _write_vertices / _write_triangles    marching cubes on the block list, the conventions of nu_mc_*: a cell
 *                           belongs to the block of its min corner and is processed iff its eight corners lie in active blocks; an
 *                           owned edge gives a vertex iff both ends are active and straddle.  V is ordered by (slot, in-block point,
 *                           axis), F by (slot, in-block cell, table slot); first_vid [nslots block^3] int32.  totals[3] (device,
 *                           int64) = (Nv, Nf, open edges): owned straddling edges with an in-grid incident cell that is not processed
 *                           -- 0 unless the active band cut the surface.  The workspace (nu_smc_workspace_bytes, 8-byte aligned)
 *                           carries counts and offsets from one call to the next.
 * --------------------------------------------------------------------------------------------------------- */
long long nu_smc_workspace_bytes(int nslots);
int nu_smc_regions(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, int* flags, float* probe,
                   float* radius, hipStream_t stream);
int nu_smc_activate(const int* flags, const float* radius, const int* probe_blocks, int nprobe, const float* f, const float* g,
                    float lipschitz, float iso, int* active, hipStream_t stream);
int nu_smc_block_rows(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, const int* blocks, int nslots,
                      long long r0, long long n, float* rows, hipStream_t stream);
int nu_smc_finish(const float* X, const float* Y, const float* Z, int nx, int ny, int nz, int block, const int* blocks, int nslots,
                  float outside_val, float* u, hipStream_t stream);
int nu_smc_count(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block, float iso,
                 void* workspace, long long workspace_bytes, hipStream_t stream);
int nu_smc_scan(int nslots, void* workspace, long long workspace_bytes, long long* totals, hipStream_t stream);
int nu_smc_write_vertices(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block, float iso,
                          const void* workspace, long long workspace_bytes, float* V, int* first_vid, hipStream_t stream);
int nu_smc_write_triangles(const float* u, const int* slot, const int* blocks, int nslots, int nx, int ny, int nz, int block, float iso,
                           const void* workspace, long long workspace_bytes, const int* first_vid, int* F, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Isotropic remeshing (extract_mesh_stage1.py:44-50: pymeshlab meshing_isotropic_explicit_remeshing; Botsch & Kobbelt 2004), one
 * pass per entry; the driver (nu_nerf_amd/remesh.py) sorts and scans between them.  V fp32 [nv,3], F int32 [nf,3] (a dead face is
 * (-1,-1,-1)), half-edge h = 3 f + s from F[f][s] to F[f][(s+1)%3], nh = 3 nf.  Every buffer is the caller's and sized by these
 * counts, so there is no opaque workspace (and no workspace-bytes query).
 *   nu_rm_edge_keys        keys[nh] int64 = (min << 32 | max) of each half-edge's vertices, INT64_MAX for a dead face
 *   nu_rm_edges            from the STABLY sorted keys and their permutation (int64): E[nh,4] int32 per sorted slot = (h0, h1,
 *                          half-edge count, locked) at the first slot of each run (= the edge id; count 0 elsewhere), he_edge[nh]
 *                          (edge id per half-edge, -1 dead), vlock / vbound[nv] u8 (zeroed here): locked = on an edge with a count
 *                          other than 2 or two same-way half-edges; boundary = on a one-face edge
 *   mesh tables (RM args)  V, nv, F, nf, E, he_edge, vc_off [nv+1], vc_corner [3 nf] (corners sorted by vertex, then corner id:
 *                          the stable sort of F), vlock, vbound
 *   nu_rm_split_count      eflag[nh] = unlocked edge with |ab|^2 > max_len2; fcnt[nf] = 1 + split edges of the face (0: dead)
 *   nu_rm_split_write      voff / foff (int64, exclusive scans of eflag / fcnt) -> Vout [nv + splits, 3] (V, then (a + b) * 0.5
 *                          in edge-id order), Fout (per face its template's faces in slot order)
 *   nu_rm_collapse_count   npts[nh] = 4 x rewritten faces of each collapse candidate (|ab|^2 < min_len2, link condition, no new
 *                          edge above max_len2, no zero-area or flipped face), 0 for the rest
 *   nu_rm_collapse_points  their query points (centroid + 3 edge midpoints per rewritten face) at 3 poff[e] (int64 exclusive scan)
 *   nu_rm_collapse_claim   pidx = nu_lbvh_closest face ids of the points under the surface-distance bound; ckey[nh] (u64), claim[nv]
 *                          (u64, reset here) and win[nh] int32: the candidates holding the atomicMin of their key at every vertex
 *                          of their endpoints' faces
 *   nu_rm_collapse_apply   the winners merged (V_io, F_io may alias V, F)
 *   nu_rm_flip_*           the same for valence-lowering flips (claim over the edge's four vertices); cos2_max = cos^2 of the
 *                          largest normal turn allowed
 *   nu_rm_relax            Vout = tangential relaxation of every unlocked vertex (area-weighted centroid of its faces, projected
 *                          on the plane of the area-weighted normal); nu_rm_project: Vout = closest (unlocked) or V (locked)
 * --------------------------------------------------------------------------------------------------------- */
int nu_rm_edge_keys(const int* F, int nf, long long* keys, hipStream_t stream);
int nu_rm_edges(const int* F, int nf, int nv, const long long* skeys, const long long* perm, int* E, int* he_edge, unsigned char* vlock,
                unsigned char* vbound, hipStream_t stream);
int nu_rm_split_count(const float* V, const int* F, int nf, const int* E, const int* he_edge, float max_len2, int* eflag, int* fcnt,
                      hipStream_t stream);
int nu_rm_split_write(const float* V, int nv, const int* F, int nf, const int* E, const int* he_edge, const int* eflag,
                      const long long* voff, const long long* foff, float* Vout, int* Fout, hipStream_t stream);
#define NU_RM_ARGS const float *V, int nv, const int *F, int nf, const int *E, const int *he_edge, const int *vc_off, \
                   const int *vc_corner, const unsigned char *vlock, const unsigned char *vbound
int nu_rm_collapse_count(NU_RM_ARGS, float min_len2, float max_len2, int* npts, hipStream_t stream);
int nu_rm_collapse_points(NU_RM_ARGS, float min_len2, float max_len2, const int* npts, const long long* poff, float* pts,
                          hipStream_t stream);
int nu_rm_collapse_claim(NU_RM_ARGS, const int* npts, const long long* poff, const int* pidx, unsigned long long* ckey,
                         unsigned long long* claim, int* win, hipStream_t stream);
int nu_rm_collapse_apply(NU_RM_ARGS, const int* win, float* V_io, int* F_io, hipStream_t stream);
int nu_rm_flip_count(NU_RM_ARGS, float cos2_max, int* npts, hipStream_t stream);
int nu_rm_flip_points(NU_RM_ARGS, float cos2_max, const int* npts, const long long* poff, float* pts, hipStream_t stream);
int nu_rm_flip_claim(NU_RM_ARGS, float cos2_max, const int* npts, const long long* poff, const int* pidx, unsigned long long* ckey,
                     unsigned long long* claim, int* win, hipStream_t stream);
int nu_rm_flip_apply(NU_RM_ARGS, const int* win, int* F_io, hipStream_t stream);
int nu_rm_relax(NU_RM_ARGS, float* Vout, hipStream_t stream);
int nu_rm_project(const float* V, int nv, const unsigned char* vlock, const float* closest, float* Vout, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Quadric-error decimation to a face budget (csrc/decimate.hip; the driver nu_nerf_amd/decimate.py sorts and scans between the
 * entries; Garland & Heckbert 1997 with memoryless quadrics, Lindstrom & Turk 1998).  One round on a compacted mesh and its
 * remeshing tables (RM args above); float64 arithmetic, no float atomic, the same bits on every run.
 *   nu_dm_quadrics   Q[nv,10] float64: per vertex the sum over its faces (corner order) of w (n^, d)(n^, d)^T, w = area; the unique
 *                    entries (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
 *   nu_dm_eval       per edge slot: cost[nh] float64, pos[nh,3] fp32 (the placement, rounded once) and npts[nh] int32 = 7 x rewritten
 *                    faces of a collapse candidate; 0 (and zeros) for a slot that is no interior edge, has two locked ends, fails the
 *                    link condition, has an opposite vertex of <= 3 faces, rewrites more than 32 faces, has a non-finite cost, or
 *                    would leave a rewritten face with zero area, a normal turned by >= 90 degrees or a shape quality
 *                    12 |n|^2 / (sum l^2)^2 below both min_quality2 and the face's old value
 *   nu_dm_points     (surface bound) the candidates' query points (per rewritten face its 3 vertices, centroid, 3 edge midpoints) at
 *                    3 poff[e] (int64 exclusive scan of npts) and lim (fp32, at poff[e]): the squared distance each may have,
 *                    (max_dist - longest edge / sqrt(12))^2, which certifies every point of the face within max_dist; negative
 *                    for a face too large to certify
 *   nu_dm_keys       ckey[nh] u64 = ((bits(float32(cost + cost_floor)) >> 12) << 32) | mix32(e) for a candidate, INT64_MAX for
 *                    the rest and, when pd2 (nu_lbvh_closest's squared distances of the points, +inf for a miss; NULL: no bound)
 *                    exceeds lim at one of its points, for it too
 *   nu_dm_claim      candidates with ckey <= threshold[0] (u64, on the device) atomicMin their key onto every vertex of every face
 *                    of both ends (claim[nv] u64, reset here); win[nh] int32 = 1 where a candidate holds both ends and both opposite vertices
 *   nu_dm_apply      winners in place (V_io, F_io may alias V, F): the kept vertex takes pos[e], the removed vertex's faces are
 *                    rewritten, the edge's two faces become (-1,-1,-1)
 * --------------------------------------------------------------------------------------------------------- */
int nu_dm_quadrics(NU_RM_ARGS, double* Q, hipStream_t stream);
int nu_dm_eval(NU_RM_ARGS, const double* Q, double min_quality2, double* cost, float* pos, int* npts, hipStream_t stream);
int nu_dm_points(NU_RM_ARGS, const float* pos, const int* npts, const long long* poff, float max_dist, float* pts, float* lim,
                 hipStream_t stream);
int nu_dm_keys(const double* cost, const int* npts, const long long* poff, const float* pd2, const float* lim, int nh,
               double cost_floor, unsigned long long* ckey, hipStream_t stream);
int nu_dm_claim(NU_RM_ARGS, const unsigned long long* ckey, const unsigned long long* threshold, unsigned long long* claim, int* win,
                hipStream_t stream);
int nu_dm_apply(NU_RM_ARGS, const int* win, const float* pos, float* V_io, int* F_io, hipStream_t stream);
#undef NU_RM_ARGS

/* ---------------------------------------------------------------------------------------------------------
 * Mesh components: labelling, per-component statistics and compaction (csrc/components.hip; the driver nu_nerf_amd/components.py
 * sorts and scans between the entries, as remesh.py does).  Every buffer is the caller's, every launch goes on `stream`.
 * Labelling is hook-and-compress over links[nl,2] (int32 node pairs; a pair (x, x) is no link) on parent[n] (int32):
 *   nu_cc_init             parent[x] = x
 *   nu_cc_vertex_links     nodes = vertices: links[2 nf, 2] = (v0, v1), (v1, v2) of every face
 *   nu_cc_edge_links       nodes = faces: links[nh, 2] from the STABLY sorted nu_rm_edge_keys and their permutation (int64): slot i
 *                          joins the faces of slots i - 1 and i when their keys are equal (an edge of k faces chains all k)
 *   nu_cc_hook             per link: the roots ra, rb of its nodes; atomicMin(parent[max(ra, rb)], min(ra, rb)).  parent[x] <= x
 *                          always, so every walk decreases and ends; a stale read is an ancestor of the same component
 *   nu_cc_compress         parent[x] = root of x
 *   nu_cc_check            flag[0] (int32, zeroed here) = 1 when a link still joins two roots (parent[a] != parent[b])
 * One round = hook, compress, check; the driver reads flag once per round and stops at the first clean one.  The fixed point is the
 * smallest node id of each component, whatever the arrival order.
 *   nu_cc_mark_used        used[nv] int32 (zeroed here) = 1 at every vertex a face references
 *   nu_cc_root_flags       isroot[n] int32 = parent[x] == x and (used == NULL or used[x])
 *   nu_cc_labels           rinc = inclusive int64 scan of isroot: label[x] = rinc[parent[x]] - 1 (-1 where used[x] == 0): component
 *                          ids 0 .. C-1 ascend with the smallest node id
 *   nu_cc_face_labels      flabel[f] = vlabel[F[f][0]]
 *   nu_cc_keep_flags       fkeep[f] = keep_comp[flabel[f]] (int32 [C]); vkeep[nv] (zeroed here) = 1 at the vertices of kept faces
 *   nu_cc_compact          finc / vinc = inclusive int64 scans of fkeep / vkeep: kept vertices and faces in their order, indices
 *                          rewritten (Vout [vinc[nv-1], 3], Fout [finc[nf-1], 3])
 * Statistics of the components of flabel[nf] in [0, C):
 *   nu_cc_face_stats       order[nf] (int64) = the stable sort of the faces by label, foff[C+1] (int64) its segments.  Per face
 *                          0.5 |(b-a) x (c-a)| and a . (b x c) / 6 in float64 from the fp32 coordinates; each segment is cut into
 *                          NU_CC_PARTS equal slices, a slice summed by one workgroup in a fixed order into part[C, NU_CC_PARTS, 2]
 *                          (float64) and pbox[C, NU_CC_PARTS, 6] (fp32 min xyz, max xyz), the slices then in slice order into
 *                          area[C], volume[C] (float64) and aabb[C, 6]: the same bits on every run
 *   nu_cc_edge_counts      from the sorted half-edge keys and their permutation: ecount[C, 3] int32 (zeroed here) = unique edges,
 *                          one-face edges, edges of three or more faces (an edge belongs to the component of its first face)
 *   nu_cc_corner_keys      keys[nh] int64 = (flabel[f] << 32 | vertex) of every corner; sorted by the caller:
 *   nu_cc_vertex_counts    vcount[C] int32 (zeroed here) = distinct vertices of each component's faces
 * The counts use integer atomicAdd (exact in any order); there is no float atomic.
 * --------------------------------------------------------------------------------------------------------- */
#define NU_CC_PARTS 32
int nu_cc_init(int* parent, int n, hipStream_t stream);
int nu_cc_vertex_links(const int* F, int nf, int* links, hipStream_t stream);
int nu_cc_edge_links(const long long* skeys, const long long* perm, int nh, int* links, hipStream_t stream);
int nu_cc_hook(int* parent, int n, const int* links, int nl, hipStream_t stream);
int nu_cc_compress(int* parent, int n, hipStream_t stream);
int nu_cc_check(const int* parent, int n, const int* links, int nl, int* flag, hipStream_t stream);
int nu_cc_mark_used(const int* F, int nf, int nv, int* used, hipStream_t stream);
int nu_cc_root_flags(const int* parent, const int* used, int n, int* isroot, hipStream_t stream);
int nu_cc_labels(const int* parent, const int* used, const long long* rinc, int n, int* label, hipStream_t stream);
int nu_cc_face_labels(const int* F, int nf, const int* vlabel, int* flabel, hipStream_t stream);
int nu_cc_keep_flags(const int* F, int nf, int nv, const int* flabel, const int* keep_comp, int C, int* fkeep, int* vkeep,
                     hipStream_t stream);
int nu_cc_compact(const float* V, int nv, const int* F, int nf, const int* fkeep, const long long* finc, const int* vkeep,
                  const long long* vinc, float* Vout, int* Fout, hipStream_t stream);
int nu_cc_face_stats(const float* V, const int* F, int nf, const long long* order, const long long* foff, int C, double* part,
                     float* pbox, double* area, double* volume, float* aabb, hipStream_t stream);
int nu_cc_edge_counts(const long long* skeys, const long long* perm, int nh, const int* flabel, int C, int* ecount,
                      hipStream_t stream);
int nu_cc_corner_keys(const int* F, int nf, const int* flabel, long long* keys, hipStream_t stream);
int nu_cc_vertex_counts(const long long* skeys, int nh, int C, int* vcount, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NU_NERF_H */
