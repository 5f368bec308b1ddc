/* C ABI of libbasd_hip.so -- the MI355X (gfx950) kernels behind the BASD loss path.
 *
 * The reference (indrajeetadityaroy9/vit-inductive-bias-distillation) is pure Python: its
 * "FFI" for this path is the set of torch operator call sites in src/losses/<module>.py.  Each entry
 * point below replaces one (or a fused group) of those call sites; the file:line it stands in
 * for is quoted on every declaration (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is DEVICE memory unless marked host; sizes/strides are in ELEMENTS;
 *   - no entry point allocates, frees or synchronises; all work is queued on `stream`
 *     (pass torch.cuda.current_stream().cuda_stream); scratch buffers are caller-provided;
 *   - return value: 0 = ok, <0 = invalid argument / unsupported shape (BASD_E*), >0 = hipError_t;
 *   - dtype codes: 0 = fp32, 1 = bf16 (inputs only; all arithmetic and outputs are fp32/fp64), 2 = uint8 (image
 *     batches of basd_mix_batch only, which is also the one entry point that may write bf16);
 *   - entry points are re-entrant and keep no global mutable state, with a few process-wide test / tuning hooks as the
 *     only exceptions: basd_tridiag_tuning, basd_jacobi_tuning, basd_jacobi_ordering, basd_gemm_tuning, basd_procrustes_tuning,
 *     basd_procrustes_finish_tuning (none is called by the
 *     loss), and the launch counter behind basd_sfadamw_launches (diagnostics).
 */
#ifndef BASD_HIP_H
#define BASD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define BASD_OK 0
#define BASD_EINVAL (-1)
#define BASD_EUNSUPPORTED (-2)
#define BASD_DTYPE_F32 0
#define BASD_DTYPE_BF16 1
#define BASD_DTYPE_U8 2    /* basd_mix_batch sources only */

/* ---- dense contractions (fp32 MFMA, v_mfma_f32_32x32x2_f32) ------------------------------- */

/* C[z] (M x N, ldc) = beta * C[z] + scale * A[z] (M x K) * B[z]^T (N x K) - 1 bias^T   (bias nullable).
 * replaces: `tokens.reshape(-1, D_t) @ proj_t.T`  layer_selector.py:72,:135;
 *           `features @ features.T / M`           layer_selector.py:15;
 *           `U_s.T @ U_t`                          layer_selector.py:99.
 * A element (m, k): a + z*a_batch_stride + (m / a_rows_per_batch)*a_sb + (m % a_rows_per_batch)*a_sn + k*a_sd
 * (so (B, N, D) token views, CLS-sliced or channel-major, are consumed in place). B: fp32 row-major.
 * colsum_part (nullable, needs beta == 0): batch * ceil(M/128) * N floats; the kernel's epilogue leaves the column
 * sums of every 128-row tile of C there.  col_mean (nullable, needs colsum_part): batch * N floats, the column means
 * of C folded from those -- `z.mean(dim=0)` of layer_selector.py:35 without another pass over z. */
int basd_gemm_nt(const void* a, int a_dtype, long a_sb, long a_sn, long a_sd, int a_rows_per_batch,
                 long a_batch_stride, const float* b, long ldb, long b_batch_stride, int M, int N, int K, int batch,
                 float* c, long ldc, long c_batch_stride, float scale, const float* bias, float beta,
                 float* colsum_part, float* col_mean, hipStream_t stream);

/* Suggested split count over the contraction rows for basd_gemm_tn. */
int basd_gemm_tn_splits(int krows);

/* C[z] (M x N) = scale * (A[z] - 1 mean_a^T)^T (B[z] - 1 mean_b^T), contraction over `krows` rows.
 * replaces: `features.T @ features / M`  layer_selector.py:13  (mean = NULL, scale = 1/M) and the
 *           centred z^T z behind `torch.linalg.svd(z - z.mean(0))`  layer_selector.py:35-36, :90-92;
 *           also the per-sample K' A' product of the Procrustes backward (batch > 1, splits = 1).
 * `slabs`: batch*splits*M*N floats of scratch when splits > 1 (deterministic split-K reduction). */
int basd_gemm_tn(const void* a, const void* b, int dtype, long a_sb, long a_sn, long a_sd, long a_batch_stride,
                 long b_sb, long b_sn, long b_sd, long b_batch_stride, int rows_per_batch, int krows, int M, int N,
                 int batch, const float* mean_a, const float* mean_b, int splits, float* slabs, float* c, long ldc,
                 long c_batch_stride, float scale, hipStream_t stream);

int basd_colmean_parts(int rows);

/* mean[z][c] = (1/rows) * sum_r X[z](r, c).   replaces `z.mean(dim=0)`  layer_selector.py:35, :91.
 * `partial`: batch*parts*cols floats of scratch. */
int basd_colmean(const void* x, int dtype, long sb, long sn, long sd, int rows_per_batch, long batch_stride,
                 int rows, int cols, int batch, int parts, float* partial, float* mean, hipStream_t stream);

/* Test / tuning hook: 1 (default) = the Gram launches (basd_syrk_multi) run on the bf16 matrix cores with every staged fp32
 * value cut into three bf16 pieces (exact) and the six leading piece products accumulated in fp32 -- fp32-grade results at
 * 2.7x the fp32 MFMA ceiling; 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32). */
int basd_gemm_tuning(int split_bf16);
int basd_gemm_tuning_get(void);       /* the current setting */

/* means[z][c] for a DEVICE table of n_mats same-layout matrices (one launch for all extraction layers of
 * layer_selector.py:88-91).  `partial`: n_mats*parts*cols floats of scratch.  vec_ok: caller asserts every base
 * pointer is 16-byte aligned. */
int basd_colmean_multi(const void* const* x_ptrs, int dtype, long sb, long sn, long sd, int rows_per_batch, int rows,
                       int cols, int n_mats, int parts, float* partial, float* means, int vec_ok,
                       hipStream_t stream);

int basd_syrk_splits(int krows, int cols, int n_mats);

/* out[z] (cols x cols, symmetric) = scales[z] * (X_z - 1 means[z]^T)^T (X_z - 1 means[z]^T),  z < n_mats.
 * replaces the per-layer Gram matrices of the selector in one launch: `features.T @ features / M`
 * layer_selector.py:13 (means row = 0, scale 1/M) and the centred z^T z behind the thin SVD :35-36, :90-92.
 * Only lower-triangular 128x128 tiles are computed (half the operand traffic of basd_gemm_tn), then mirrored.
 * x_ptrs: DEVICE array of base pointers; element (k, c) of X_z at x_ptrs[z] + (k / rows_per_batch)*sb +
 * (k % rows_per_batch)*sn + c*sd.  means / scales (nullable): n_mats*cols / n_mats floats on the device.
 * slabs: n_mats*splits*cols*cols floats of scratch (splits from basd_syrk_splits).  vec_ok: caller asserts
 * every base pointer is 16-byte aligned.  fold (nullable): (n_mats - fold_from) x fold_parts x cols row-tile column
 * sums as left by basd_gemm_nt's epilogue; matrices z >= fold_from take their means from it (sum / krows) instead
 * of `means`, folded inside the kernel. */
int basd_syrk_multi(const void* const* x_ptrs, int dtype, long sb, long sn, long sd, int rows_per_batch, int krows,
                    int cols, int n_mats, const float* means, const float* scales, int splits, float* slabs,
                    float* out, long out_stride, int vec_ok, const float* fold, int fold_parts, int fold_from,
                    hipStream_t stream);

/* ---- one-sided Jacobi SVD / symmetric eigensolver ------------------------------------------ */

int basd_jacobi_workspace_ints(int batch, int max_sweeps);
/* Longest column (rows_dot; riding rows likewise) basd_jacobi_onesided has a kernel shape for, hence also the largest
 * order of a plain square problem. */
int basd_jacobi_max_rows(void);
/* 1 when the plain 4-lane LDS shape of basd_jacobi_onesided fits order n (39..196; the planner's answer with 4 lanes
 * forced and the round-robin ordering, whatever the batch: callers test batch >= 128 themselves):
 * basd_procrustes_forward_fused then solves the TRANSPOSED cores, without riding rows. */
int basd_jacobi_plain4_fits(int n);

/* In-place one-sided Jacobi on `batch` column-major matrices (rows_tot x n, leading dim rows_tot):
 * right rotations orthogonalise the first rows_dot rows; colnorm receives the column norms.
 * replaces the LAPACK calls behind torch.linalg.eigvalsh (layer_selector.py:16), torch.linalg.svd
 * (:36, :92), torch.linalg.svdvals (:99) and torch.linalg.matrix_norm(ord="nuc") (relational.py:48).
 * n_arr (nullable): per-matrix order 0 <= n_arr[m] <= n for plain square problems (no riding rows); storage stays that
 * of the largest problem, and what lies outside a matrix's leading n_arr[m] x n_arr[m] block is left alone.  Taken at
 * every order up to basd_jacobi_max_rows(): in LDS up to 192, by the block path beyond.
 * flags: basd_jacobi_workspace_ints() ints.
 * tol_cos: stop when every pair has |cos| <= tol_cos over a full sweep (<= 0: eps * sqrt(rows_dot)). */
/* Test / tuning hook: lanes per column pair of the LDS-resident solver; 0 = automatic (batches >= 256 of stacked
 * matrices: 4 lanes for n >= 40, 8 for n >= 16 -- fewer instruction issues per matrix round; else one DPP row of 16),
 * 4 / 8 / 16 = forced where the shape allows. */
int basd_jacobi_tuning(int lanes_per_pair);
/* Test / tuning hook: ordering of the plain batched solver (no riding rows, batches >= 128 of orders 40..200: the
 * transposed Procrustes cores) -- 1 (default) = odd-even ordering with the columns held in registers and one column per
 * pair-step passed through LDS (two 196 x 196 matrices share a CU), 0 = round-robin ordering through LDS. */
int basd_jacobi_ordering(int odd_even);

int basd_jacobi_onesided(float* W, long batch_stride, int rows_dot, int rows_tot, int n, int batch,
                         const int* n_arr, float* colnorm, int colnorm_stride, int max_sweeps, float tol_cos,
                         int* flags, int* sweeps_out, hipStream_t stream);
/* What basd_jacobi_onesided would launch for that shape under the current tuning hooks (host only, no HIP call).
 * out8: route -- 1 stacked 8-lane LDS, 2 stacked 4-lane LDS, 3 plain 8-lane LDS, 4 odd-even in registers, 5 plain
 * 4-lane LDS, 6 16-lane LDS, 7 block rounds, 0 no kernel shape (BASD_EUNSUPPORTED) --, lanes per column pair, elements
 * per lane, of which over the dot rows, threads, dynamic LDS bytes, and on the block route columns per block and
 * blocks.  basd_jacobi_plain4_fits / basd_jacobi_lds_square_fits / basd_jacobi_twopass_workspace_bytes answer from the
 * same planner. */
int basd_jacobi_plan_query(int rows_dot, int rows_tot, int n, int batch, int per_matrix_orders, int* out8);

/* The same for stacked square cores [M; L_b] (2n x n, leading dimension 2n; the Procrustes cores of relational.py:48)
 * whose 2n rows do not fit LDS while n rows do (n = 129..196: cfg-5's 144, cfg-4's 196): pass 1 solves the top n x n
 * in LDS and logs every rotation, pass 2 replays the log on the riding rows in LDS -- the same rotations in the same
 * order as the one-kernel solver, without the block solver's trips through L2 / HBM.  workspace: device memory of
 * basd_jacobi_twopass_workspace_bytes() bytes, 8-byte aligned (0 bytes = shape not covered: BASD_EUNSUPPORTED, use
 * basd_jacobi_onesided). */
long basd_jacobi_twopass_workspace_bytes(int n, int batch, int max_sweeps);
int basd_jacobi_stacked_twopass(float* W, long batch_stride, int n, int batch, float* colnorm, int colnorm_stride,
                                int max_sweeps, float tol_cos, void* workspace, int* sweeps_out, hipStream_t stream);

/* Sort column norms descending; optionally emit the top-kmax normalised columns as rows
 * (`Vt[:k]` of layer_selector.py:37, :97). */
int basd_sort_extract(const float* W, long batch_stride, int rows, int rows_tot, int n, int batch,
                      const float* colnorm, int colnorm_stride, float* vals_desc, float* vecs, int kmax,
                      hipStream_t stream);

/* ---- tridiagonalisation-based symmetric eigen-solver (eigenvalues / leading eigenvectors only) ------- */

/* Householder tridiagonalisation A = Q T Q^T of `batch` symmetric n x n matrices (A destroyed):
 * first stage of the LAPACK path behind torch.linalg.eigvalsh (layer_selector.py:16) and the
 * Vt[:k] / S[:k] part of torch.linalg.svd (:36, :92).  d, e, tau: (batch, n); vh: (batch, n, n). */
long basd_tridiag_workspace_bytes(int n, int batch);

/* `work`: basd_tridiag_workspace_bytes(n, batch) bytes of 16-byte aligned device scratch.
 * Two stages: the trailing block of order <= 256 is factored in the registers of ONE CU per matrix (n <= 256: the
 * whole factorisation -- no workgroup waits for another); for n > 256 the first n - 256 steps run with the matrix
 * shared by up to 16 workgroups that exchange one 16-byte granule per row and step through `work` (all workgroups of
 * that launch must be resident together: at most half of what an occupancy query says the device holds of the kernel,
 * and never more than 128; beyond that the member count per matrix shrinks, down to 1 = no exchange).  Its last 32
 * bytes hold a status word that is non-zero afterwards if a workgroup of the shared stage gave up waiting for its
 * partners, and a trace of the first give-up (step + 1, row, member | matrix << 8, tag seen, tag wanted). */
int basd_tridiag(float* a, long a_batch_stride, int n, int batch, float* d, float* e, float* tau, float* vh,
                 void* work, hipStream_t stream);

/* basd_tridiag + the Marchenko-Pastur ranks (see basd_tridiag_mp_rank; layer_selector.py:16-19, :74) of the FIRST
 * rank_count matrices of the batch, computed by the workgroup that finishes each factorisation -- no separate launch on
 * the path the host waits for.  host_mirror (nullable): pinned host memory of rank_count + 8 ints that receives the
 * ranks and then the factorisation's 8 status words. */
int basd_tridiag_ranked(float* a, long a_batch_stride, int n, int batch, float* d, float* e, float* tau, float* vh,
                        void* work, int rank_count, double factor, int cap, int* rank_out, int* host_mirror,
                        void* mid_event /* nullable hipEvent_t: recorded behind the multi-workgroup stage */,
                        hipStream_t stream);

/* Test / tuning hook for basd_tridiag (the only process-wide setting of the library; its defaults come from the
 * BASD_TRIDIAG_{MEMBERS,PAD,LAG,THREADS,TAIL} environment variables, read ONCE when the library is loaded -- no
 * entry point calls getenv).  Negative = keep; reset != 0 restores the load-time values first.
 * members: workgroups per matrix in the shared stage; pad: workgroup-id padding between matrices; lag: member that
 * sleeps every step; threads: per member; tail: 0 = shared stage for the whole factorisation, 1 (default) = orders
 * 257..384 whole in the packed one-CU kernel, other orders shared stage + the register-resident tail kernel, 3 = shared
 * stage + tail kernel for every order.  Any other tail: BASD_EINVAL from the call (nothing changes), ignored in the
 * environment. */
int basd_tridiag_tuning(int members, int pad, int lag, int threads, int tail, int reset);

/* What basd_tridiag / _ranked / _ranked_gated would launch for that shape under the current tuning hooks (host only, no
 * HIP call).  flags: 1 = the matrices can be read as 16-byte quads (16-byte aligned base, a_batch_stride % 4 == 0),
 * 2 = ranks asked for, 4 = the gated entry point.  resident_budget: workgroups of the shared stage that may be resident
 * together (the entry points take it from an occupancy query); <= 0 = the cap of 128.
 * Returns what the entry point would: BASD_EINVAL (n < 2, batch < 1), BASD_EUNSUPPORTED (n > 4096; a gated call of a
 * shape the gate does not take), else BASD_OK with
 * out12: [0] front stage -- 0 none, 1 shared stage --, [1] back stage -- 0 none, 1 tail kernel, 2 packed kernel --,
 * [2] j_stop (steps of the front stage), [3] shared-stage kernel -- 0 scalar, 1 quads, 2 quads with n % 8 == 0 --,
 * [4] members per matrix, [5] workgroups of the shared stage, [6] its threads, [7] its dynamic LDS bytes ([3]..[7] are 0
 * without a front stage), [8] ranks -- 0 none, 1 by the back stage's workgroups, 2 by a separate launch --, [9] the
 * gated entry point takes the shape, [10] offset of the 8 status words in the workspace, [11]
 * basd_tridiag_workspace_bytes(n, batch). */
int basd_tridiag_plan_query(int n, int batch, int flags, int resident_budget, int* out12);

/* All eigenvalues (descending) of the tridiagonals by Sturm-sequence bisection. */
int basd_tridiag_eigenvalues(const float* d, const float* e, int n, int batch, float* vals_desc, hipStream_t stream);

/* The leading eigenvalues only (layer_selector.py:36-37, :92: S[:k] and Vh[:k] are all that is read of a spectrum once
 * the ranks are known): writes elements [0, min(n, 64 ceil(k / 64))) of every row of vals_desc (row stride n) with the
 * bits basd_tridiag_eigenvalues writes there, and leaves the rest of the row untouched.  k > 0; a k past n is taken as n. */
int basd_tridiag_eigenvalues_leading(const float* d, const float* e, int n, int k, int batch, float* vals_desc,
                                     hipStream_t stream);

/* out (batch, k_stride, n) rows = Q x (transpose = 0) or Q^T x (transpose = 1) for the rows of x (batch, k, n), Q the
 * product of the reflectors of basd_tridiag.  With basd_tridiag_shifted_solve this gives (A - lambda I)^{-1} on the
 * orthogonal complement of the leading eigenvectors: the part of the backward of `torch.linalg.svd(...).Vh[:k]`
 * (layer_selector.py:92 under autograd) that involves the eigenvectors NOT computed. */
int basd_tridiag_apply_q(const float* tau, const float* vh, int n, int k, int batch, const float* x, float* out,
                         int k_stride, int transpose, hipStream_t stream);

/* x[z][t] = (T_z - shifts[z][t] I)^{-1} rhs[z][t], t < k: LU with partial pivoting + one solve with perturbed tiny
 * pivots (shifts are eigenvalues; the caller projects the singular direction out).  rhs, x: (batch, k, n). */
int basd_tridiag_shifted_solve(const float* d, const float* e, const float* shifts, int shift_stride, int n, int k,
                               int batch, const float* rhs, float* x, hipStream_t stream);

/* Marchenko-Pastur rank of each tridiagonal without its spectrum: the lower median eigenvalue by 1025-section
 * Sturm counts, the threshold median * factor rounded to fp32, and one Sturm count at the threshold
 * (layer_selector.py:16-19; `factor` = (1 + sqrt(D/M))^2 in float64 from the host, `cap` as :74).
 * This is the quantity the host reads back every step: host_mirror (nullable) is device-visible pinned host memory
 * of batch + 8 ints; the kernel writes the ranks and the 8 words at `status` (nullable: the status area of
 * basd_tridiag's workspace) straight into it. */
int basd_tridiag_mp_rank(const float* d, const float* e, int n, int batch, double factor, int cap, int* rank_out,
                         float* thr_out, const int* status, int* host_mirror, hipStream_t stream);

/* Leading k eigenvectors of the original matrices (inverse iteration on T, cluster re-orthogonalisation,
 * back-transformation with the reflectors), written as rows of vecs (batch, k_stride, n).
 * z: batch*k*n floats of scratch. */
int basd_tridiag_eigenvectors(const float* d, const float* e, const float* tau, const float* vh,
                              const float* vals_desc, int n, int k, int batch, float* z, float* vecs, int k_stride,
                              hipStream_t stream);

/* ---- opt-in residual check of a tridiagonal factorisation ------------------------------------------------------
 * For a symmetric A of order n, its factorisation (d, e, tau, vh) and a probe vector x, with eps = 2^-24 and every sum
 * accumulated in fp64:
 *     rho_trace = |sum d_i - tr A| / (eps |A|_F)
 *     rho_fro   = |sum d_i^2 + 2 sum e_i^2 - |A|_F^2| / (eps |A|_F^2)
 *     rho_res   = |Q^T (A x) - T (Q^T x)|_2 / (eps |A|_F |x|_2),   Q the reflector product, T = tridiag(d, e).
 * A numerator of exactly 0 over a denominator of 0 (the zero matrix) is ratio 0; a ratio that is not <= its threshold
 * (any non-finite one included) fails.  The first two catch a wrong d or e, the third is a one-vector Freivalds test that
 * also covers tau and vh.  All three are NORMWISE: an error confined to directions whose eigenvalues lie far below
 * |A|_F is smaller than the rounding these bounds allow for and is not seen.
 *
 * The probe vector has no RNG state: element i of matrix index m (its position in the batch of the call) is
 *     h  = m * MUL_M + i * MUL_I + ADD;  h ^= h >> 15;  h *= MIX_1;  h ^= h >> 12;  h *= MIX_2;  h ^= h >> 15;
 *     x  = (h >> 31) ? -1 : +1                              (uint32 arithmetic; basd_tridiag_probe_sign below).
 *
 * Order of the calls on one stream: basd_tridiag_probe (reads A, which the factorisation destroys), basd_tridiag*,
 * basd_tridiag_apply_q(tau, vh, n, 2, batch, probe, work, 2, 1) on the two rows the probe leaves, basd_tridiag_check.
 * Three launches in all; no entry point allocates or synchronises. */
#define BASD_TRIDIAG_PROBE_MUL_M 0x9E3779B1u
#define BASD_TRIDIAG_PROBE_MUL_I 0x85EBCA77u
#define BASD_TRIDIAG_PROBE_ADD 0x27D4EB2Fu
#define BASD_TRIDIAG_PROBE_MIX_1 0x2C1B3C6Du
#define BASD_TRIDIAG_PROBE_MIX_2 0x297A2D39u
#define BASD_TRIDIAG_PROBE_ROWS 16          /* rows of A per workgroup of the probe launch */
#define BASD_TRIDIAG_CHECK_MAX_N 1024       /* largest order (that of basd_tridiag_apply_q) */
#define BASD_TRIDIAG_VERDICT_INTS 8
/* Default thresholds (thresholds == NULL): 8 x the worst value measured over fp32 LAPACK ssytrd and this library's own
 * factorisations, profiles/tridiag_check.txt.  The two sum tests grow like sqrt(n) (n rounded terms), the residual
 * test does not.  How far they sit below a single-entry corruption (same file): a d entry moved by 1e-3 max|d| gives
 * rho_trace 3.5 x its limit on a randn Gram of order 448, but only 16777 / sqrt(n) on a multiple of the identity -- 1.2 x
 * the limit at order 1024, and nothing from order 1261 on; an e entry moved likewise 3.1 x the rho_res limit; a tau or
 * vh entry of an active reflector moved by 1e-2 at least 13 x it on the matrices measured, about 2 x for the smallest
 * such effect known (rho_res 38).  Not the factor 4 one would like: pass tighter limits where the matrices allow it. */
#define BASD_TRIDIAG_CHECK_TRACE_PER_SQRT_N 13.3
#define BASD_TRIDIAG_CHECK_FRO_PER_SQRT_N 8.5
#define BASD_TRIDIAG_CHECK_RES 18.6
#define BASD_TRIDIAG_CHECK_BIT_TRACE 1
#define BASD_TRIDIAG_CHECK_BIT_FRO 2
#define BASD_TRIDIAG_CHECK_BIT_RES 4

#if defined(__HIPCC__)
#define BASD_TRIDIAG_PROBE_FN static __host__ __device__ __forceinline__
#else
#define BASD_TRIDIAG_PROBE_FN static inline
#endif
BASD_TRIDIAG_PROBE_FN float basd_tridiag_probe_sign(uint32_t m, uint32_t i) {
    uint32_t h = m * BASD_TRIDIAG_PROBE_MUL_M + i * BASD_TRIDIAG_PROBE_MUL_I + BASD_TRIDIAG_PROBE_ADD;
    h ^= h >> 15;
    h *= BASD_TRIDIAG_PROBE_MIX_1;
    h ^= h >> 12;
    h *= BASD_TRIDIAG_PROBE_MIX_2;
    h ^= h >> 15;
    return (h >> 31) ? -1.0f : 1.0f;
}

/* Bytes of the probe buffer of `batch` matrices of order n (16-byte aligned device memory; 0 = order not covered).
 * Layout: (batch, 2, n) fp32 -- row 0 = x, row 1 = y = A x accumulated in fp64 and rounded once --, then per matrix
 * ceil(n / BASD_TRIDIAG_PROBE_ROWS) pairs of fp64 (tr A, |A|_F^2 of that block of rows; basd_tridiag_check and
 * the callers fold them in index order), then the fp64 pair (tr A, |A|_F^2) of every matrix folded in that order by
 * basd_tridiag_check, then 8 control words for the verdict of basd_tridiag_check, which the probe launch clears. */
long basd_tridiag_probe_bytes(int n, int batch);

/* One pass over `batch` full row-major symmetric matrices (a_batch_stride elements apart), BEFORE basd_tridiag destroys
 * them: one workgroup per BASD_TRIDIAG_PROBE_ROWS rows, 16-byte loads where n, the stride and the base allow, every
 * reduction in a fixed order (two calls leave the same bits).  1 <= n <= BASD_TRIDIAG_CHECK_MAX_N, else
 * BASD_EUNSUPPORTED. */
int basd_tridiag_probe(const float* a, long a_batch_stride, int n, int batch, void* probe, hipStream_t stream);

/* The three ratios of every matrix -> ratios_out (batch, 3) fp32, and the verdict of the batch -> verdict_out
 * (BASD_TRIDIAG_VERDICT_INTS int32): [0] matrices that failed, [1] index of the first one (-1: none), [2] OR of their
 * BASD_TRIDIAG_CHECK_BIT_* masks, [3] matrices checked, [4..6] the fp32 bit patterns of the worst rho_trace, rho_fro,
 * rho_res of the batch (a NaN counts as worst), [7] 0.  host_mirror (nullable): pinned host memory that receives the same
 * 8 words.  One workgroup per matrix; the last one to finish writes the verdict.
 * work: (batch, 2, n) = Q^T of the probe's two rows (see above; NULL = Q is the identity, the rows are read from the
 * probe itself: n == 1, for which there is no reflector and basd_tridiag_apply_q takes no call).  tau and vh are
 * only checked for presence: they enter through `work`.  thresholds (host, nullable): rho_trace, rho_fro, rho_res
 * limits; NULL = the defaults above.  A probe serves one check at a time (the control words are shared), any number one
 * after another. */
int basd_tridiag_check(const float* d, const float* e, const float* tau, const float* vh, int n, int batch,
                       void* probe, const float* work, const float* thresholds, float* ratios_out, int* verdict_out,
                       int* host_mirror, hipStream_t stream);

/* ---- selector epilogues --------------------------------------------------------------------- */

/* rank = min(#{eig > fp32(median_lower(eig) * factor)}, cap).  layer_selector.py:17-19, :74.
 * factor = (1 + (D/M)**0.5)**2 evaluated by the HOST in float64 (layer_selector.py:11,18). */
int basd_mp_rank(const float* vals_desc, int n, int batch, double factor, int cap, int* rank_out, float* thr_out,
                 hipStream_t stream);

/* d = sum(sw * acos(min(sigma, 1-eps))^2) / sum(sw) per (student layer, teacher layer) item.
 * layer_selector.py:99-105. */
int basd_grassmann_distance(const float* colnorm, int stride, const int* k_arr, const float* sw, int sw_stride,
                            const int* sw_index, int items, float* d_out, float* theta_out, hipStream_t stream);

/* The same for matrices that were zero-padded to a common order n_valid (everything outside the leading k x k block zero,
 * basd_selector_chain_tail): colnorm holds n_valid values per item in any order, the k largest are the cosines. */
int basd_grassmann_distance_padded(const float* colnorm, int stride, int n_valid, const int* k_arr, const float* sw,
                                   int sw_stride, const int* sw_index, int items, float* d_out, hipStream_t stream);

int basd_sqrt_clamp(const float* in, float* out, long count, hipStream_t stream);

/* Both Grams of the projected teacher tokens z = tokens proj_t^T (layer_selector.py:72 -> :13 and :35) from the centred
 * Gram of the tokens in THEIR OWN space, for teachers about as wide as the student (D_t <~ 1.5 D_s: ViT teachers) -- z is
 * never formed: c (batch, n, n) = proj_t G_c proj_t^T (two basd_gemm_nt), zbar (batch, n) = proj_t tbar;
 * out_c (nullable: c is symmetric already) = sym(c) (the centred Gram of z), out_u (nullable: the rank-one route of the MP
 * rank, basd_tridiag_mp_rank_rank1, never forms it) = (sym(c) + M zbar zbar^T) / M (its uncentred Gram / M, M = m_rows).  Also the second Gram of basd_selector_chain: c = the centred Gram of the projected
 * tokens themselves, zbar their column means -- one symmetric launch per layer instead of two. */
int basd_gram_finish(const float* c, const float* zbar, int n, int batch, long m_rows, float* out_u, float* out_c,
                     hipStream_t stream);

/* Everything of the selector that follows the rank read-back, queued by one call (layer_selector.py:36-37, :92,
 * :95-105): leading kmax eigenvectors of the E student / L centred teacher Grams from their basd_tridiag
 * factorisations (t_* / s_*: d, e, tau, vh, vals), S[:k], the teacher bases rotated by proj_s^T, the E x L cosine
 * matrices, their singular values and d_grass_sq (E, L) -> d_out.  Scratch (floats unless noted): z_s, v_s
 * (E kmax d_s), z_t, u_t, u_rot (L kmax d_s), sw (L kmax), cos (E L kmax^2), k_arr (E L ints), sigma (E L kmax),
 * flags (basd_jacobi_workspace_ints(E L, 20) ints); sw_index: (E L) ints, item e*L+l -> l. */
int basd_selector_tail(const float* t_d, const float* t_e, const float* t_tau, const float* t_vh, const float* t_vals,
                       const float* s_d, const float* s_e, const float* s_tau, const float* s_vh, const float* s_vals,
                       int d_s, int E, int L, int kmax, const int* ranks, const float* proj_s_t, float* z_s,
                       float* v_s, float* z_t, float* u_t, float* u_rot, float* sw, float* cos, int* k_arr,
                       const int* sw_index, float* sigma, int* flags, float* d_out, hipStream_t stream);

/* Marchenko-Pastur ranks of the UNCENTRED Grams from the factorisations of the CENTRED ones (layer_selector.py:13-19 from
 * the matrices of :35): z^T z = G_c + M zbar zbar^T and G_c = Q T Q^T give z^T z = Q (T + M w w^T) Q^T with w = Q^T zbar
 * (basd_tridiag_apply_q, transposed), and the eigenvalues of a rank-one modification are COUNTED without another
 * factorisation: #{below x} = #{negative pivots of T - x I} + [-1/M - w^T (T - x I)^-1 w < 0] - 1, in one fp64 Sturm
 * recurrence.  A teacher layer then needs one factorisation instead of two.  d, e: (batch, n); w: (batch, n); rho = M;
 * factor, cap, rank_out, status, host_mirror as basd_tridiag_mp_rank. */
int basd_tridiag_mp_rank_rank1(const float* d, const float* e, const float* w, int n, int batch, double rho,
                               double factor, int cap, int* rank_out, const int* status, int* host_mirror,
                               hipStream_t stream);

/* basd_tridiag_ranked queued BEFORE its input exists (orders 257..384, the one-kernel factorisation; BASD_EUNSUPPORTED
 * otherwise): its whole-CU workgroups take their CUs while the chip is still quiet and wait, asleep and bounded, until
 * *go_flag == go_value; set that word with basd_flag_set on the stream that produces the matrices, behind them.  If the
 * word does not arrive within go_budget polls of ~1.7 us (e.g. a profiler serialising kernels) the workgroups give up:
 * status word 0 = 2 (also in host_mirror[rank_count]); queue the plain basd_tridiag_ranked then.
 * replaces: the same call sites as basd_tridiag_ranked (layer_selector.py:16-19, :72-74). */
int basd_tridiag_ranked_gated(float* a, long a_batch_stride, int n, int batch, float* d, float* e, float* tau, float* vh,
                              void* work, int rank_count, double factor, int cap, int* rank_out, int* host_mirror,
                              const unsigned* go_flag, unsigned go_value, int go_budget, hipStream_t stream);
int basd_flag_set(unsigned* flag, unsigned value, hipStream_t stream);

/* The selector of one loss step queued by ONE call over three streams (layer_selector.py:69-74 `_estimate_ranks`,
 * :131-138 teacher subspaces, :86-105 `_mix_for_student_layer` up to d_grass_sq): teacher projections z_l =
 * tokens_l proj_t^T, the centred Gram of every z_l and its uncentred Gram / M from it (+ M zbar zbar^T: an addition, no
 * second symmetric launch), centred Grams of the E student layers, the
 * Householder tridiagonalisation of all 2L + E matrices with the Marchenko-Pastur ranks of the L uncentred ones
 * written to `ranks` (device) and `host_mirror` (pinned host: L ranks + the 8 status words of basd_tridiag_ranked)
 * by the kernel that finishes the factorisation, then -- on tail_stream, with the ranks taken from DEVICE memory --
 * what basd_selector_tail does.  The host only waits for ev_ranks (basd_event_synchronize) to refresh
 * `subspace_ranks` and to raise on rank 0 like the reference.
 *   kmax: eigenvectors computed per matrix in the tail, a HINT (the previous step's largest rank); any value >= the
 *         largest rank of this step gives the same d_grass_sq; if the ranks read back exceed it, call
 *         basd_selector_chain_tail(args, larger kmax) again.  0: do not queue the tail (first step: no hint yet).
 *   mode: 0 = one factorisation launch over all 2L + E matrices (student Grams formed on student_stream beside the
 *             teacher's projections);
 *         1 = teacher matrices first; the student side (Grams + factorisation, student_stream != chain_stream) is
 *             held back until the ranks are out;   2 = the same, not held back;
 *         3 = the same, held back until the teacher's Grams are done (ev_tg0):
 *             the student Grams -- the largest MFMA launch of the step -- then run beside the teacher's
 *             factorisation (two CUs) instead of beside its projection and Grams.
 *   streams: main_stream = the caller's (inputs are ready there; NULL: the caller has recorded ev_fork on it already,
 *         e.g. before it queued other work the chain need not wait for); events are opaque handles of basd_event_create:
 *         ev_fork / ev_student / ev_ranks / ev_tail / ev_tgram / ev_tg0 are recorded by the call; ev_slot_free (nullable) is waited for
 *         before anything is written: the ev_tail of the call that used these buffers last.
 *   Every field is 8 bytes wide.  Device buffers (floats unless noted), n = d_s, M_t = B n_t, nt = ceil(M_t / 128):
 *         z (L, M_t, n); z_sums (L, nt, n); z_means (L, n); z_ptrs: device table of L pointers [z_0..z_{L-1}];
 *         t_slabs (L t_splits n n), t_splits = basd_syrk_splits(M_t, n, L);
 *         s_partial (E s_parts n), s_parts = basd_colmean_parts(B n_s); s_means (E, n); s_slabs (E s_splits n n);
 *         grams, vh (2L + E, n, n); d, e, tau, vals (2L + E, n); tri_work: basd_tridiag_workspace_bytes(n, 2L + E)
 *         bytes (modes 1, 2: (n, 2L) and tri_work_s (n, E)); ranks (L ints);
 *         tail, K = kmax_cap >= kmax: zv, vecs ((L + E) K n); u_rot (L K n); sw (L K); cos (E L K K); sigma (E L K);
 *         d_out (E L); k_arr (E L ints); sw_index (E L ints, item e L + l -> l);
 *         jflags (basd_jacobi_workspace_ints(E L, 20) ints).
 * Returns BASD_EUNSUPPORTED when B n_t < d_s (the reference then forms the token-side Gram, layer_selector.py:14-15):
 * take the per-kernel entry points. */
typedef struct BasdSelectorChain {
    const void* const* teacher_host_ptrs;  /* HOST array of L device pointers: (B, n_t, d_t) views with common strides */
    long t_dtype, t_sb, t_sn, t_sd;
    const void* const* student_ptrs;       /* device table of E pointers: (B, n_s, d_s) views with common strides */
    long s_dtype, s_sb, s_sn, s_sd, s_vec_ok;
    const float* proj_t;                   /* (d_s, d_t) fp32 row-major */
    const float* proj_s_t;                 /* (d_s, d_s) fp32: proj_s^T */
    long E, L, B, n_s, n_t, d_s, d_t;
    double mp_factor;                      /* (1 + sqrt(d_s / M_t))^2, float64 on the host as layer_selector.py:11,18 */
    long rank_cap;                         /* d_s - 1 (layer_selector.py:74) */
    long kmax, kmax_cap, mode;
    float* z; float* z_sums; const void* const* z_ptrs; float* z_means; float* t_slabs; long t_splits;
    float* s_partial; float* s_means; float* s_slabs; long s_splits, s_parts;
    float* grams; float* d; float* e; float* tau; float* vh; float* vals; void* tri_work; void* tri_work_s;
    int* ranks; int* host_mirror;          /* host_mirror: pinned host memory, L + 8 ints (nullable) */
    int* student_status_mirror;            /* modes 1, 2: pinned host memory, 8 ints (nullable) */
    float* zv; float* vecs; float* u_rot; float* sw; float* cos; float* sigma; float* d_out;
    int* k_arr; const int* sw_index; int* jflags;
    hipStream_t main_stream, chain_stream, student_stream, tail_stream;
    void* ev_fork; void* ev_student; void* ev_ranks; void* ev_tail; void* ev_slot_free; void* ev_tgram; void* ev_tg0;
    /* mode 3, nullable: the teacher's factorisation is queued FIRST, on fact_stream, and waits for go_flag (one device
     * word of the slot, set behind the teacher Grams to go_value != 0): see basd_tridiag_ranked_gated.  ev_ranks is then
     * recorded on fact_stream. */
    hipStream_t fact_stream; unsigned* go_flag; long go_value; long go_budget;
    /* measurement (all nullable; timed events of basd_event_create_timed, recorded on the stream of the launch they
     * bracket): tm_proj = behind the projections, tm_tgram = behind the teacher Grams, tm_scol0 / tm_scol1 = around the
     * student column means, tm_sgram = behind the student Grams, tm_tri0 = in front of the factorisation (ev_ranks ends
     * it), tm_mid = between its two stages, tm_spec = behind the spectra at the head of the tail */
    void* tm_proj; void* tm_tgram; void* tm_scol0; void* tm_scol1; void* tm_sgram; void* tm_tri0; void* tm_mid; void* tm_spec;
    /* Rank certificate (all four nullable together).  The reference raises inside forward when a teacher layer has MP
     * rank 0 (layer_selector.py:16-19 -> NaN weights -> torch.linalg.svd raises), which is what the host waits ~1.5 ms
     * for.  Behind the teacher Grams -- long before the factorisation -- one small kernel on cert_stream proves
     * "every rank >= 1" where it can: with eigenvalues l_1 >= ... >= l_n >= 0 of the uncentred Gram G = A + zbar zbar^T,
     *     l_1 >= max(|zbar|^2, ||G||_F^2 / tr G)   and   median <= min(tr G / c, tr A / (c - 1)),  c = n - (n-1)/2,
     * so "left > 1.5 factor right" (the 1.5: fp32 eigenvalue errors ~2e-5 l_1, entries slightly off PSD)
     * leaves no way for l_1 > fp32(median factor) to fail.  cert_mirror (pinned host, 1 int) = 1 if proven for ALL
     * layers, else 0 (flat spectra, NaN: the caller then waits for the ranks as before); ev_cert is recorded behind it.
     * cert_stream may be chain_stream (the kernel then sits between the Grams and the factorisation; measured best). */
    hipStream_t cert_stream; int* cert_mirror; void* ev_cert;
    double* cert_scratch;                  /* basd_rank_certificate_scratch_bytes(L) bytes, ZEROED once (the kernel leaves it zeroed) */
} BasdSelectorChain;
int basd_selector_chain(const BasdSelectorChain* args);
/* The certificate kernel of BasdSelectorChain.cert_mirror on its own: *flag (device or pinned host memory) = 1 iff
 *     max(|zbar|^2, ||G||_F^2 / tr G) > 1.5 factor min(tr G / c, (tr G - |zbar|^2) / (c - 1)),   c = n - (n-1)/2,
 * holds for every one of the `batch` symmetric n x n matrices G = A + zbar zbar^T (A PSD; zbar (batch, n) nullable = 0)
 * -- a sufficient condition for "every Marchenko-Pastur rank (layer_selector.py:16-19) is >= 1"; else 0. */
int basd_rank_certificate(const float* grams, const float* zbar, int n, int batch, double factor, double* scratch,
                          int* flag, hipStream_t stream);
/* scratch: basd_rank_certificate_scratch_bytes(batch) bytes of device memory, zeroed before the FIRST launch that uses
 * it (partial sums + a ticket; the launch leaves it zeroed again). */
long basd_rank_certificate_scratch_bytes(int batch);
/* Test hook: fills every CU's LDS with `pattern` (a NaN, say): no kernel may depend on what its CU's previous tenant left. */
int basd_debug_fill_lds(unsigned pattern, hipStream_t stream);
/* exact_k != 0: the caller has READ the ranks and every one of them equals kmax (one teacher layer): the principal-angle
 * matrices then have one common order and may leave LDS (orders past basd_jacobi_lds_square_fits; a speculative kmax
 * past it returns BASD_EUNSUPPORTED). */
int basd_selector_chain_tail(const BasdSelectorChain* args, int kmax, int exact_k);
int basd_jacobi_lds_square_fits(int n);

/* ---- attention-weighted Procrustes loss ------------------------------------------------------ */

/* Token weights from the layer-mixed attention.  relational.py:22-34 + layer_selector.py:112.
 * attn_ptrs: device array of L pointers to (B, H, A, A) tensors sharing strides (sb, sh, sq, sk),
 * A = n_a + has_cls.  atap*: weight interpolation n_a -> n_s; tap*: token interpolation n_t -> n_s
 * (both NULL when the grids coincide). */
int basd_token_weights(const void* const* attn_ptrs, int dtype, const float* mix, int L, long sb, long sh, long sq,
                       long sk, int B, int H, int A, int has_cls, int n_a, int n_t, int n_s, const int* atap0,
                       const int* atap1, const float* alam, const int* tap0, const int* tap1, const float* lam,
                       float* omega, float* omega_t, float* raw_out, hipStream_t stream);

/* Student half of relational.py:36-45 and the adjoint of combined.py:9-14:
 * mu = sum_n w_n x_n, tr_s = sum_n w_n |x_n - mu|^2 (as (B, ceil(D/64)) per-slab partials),
 * A' = I_interp^T diag(w) (X - 1 mu^T).  The general per-layer form: any row alignment, any number of tokens. */
int basd_student_project(const void* x, int dtype, long sb, long sn, int B, int n_s, int n_t, int D,
                         const float* omega, const int* tap0, const int* tap1, const float* lam, const int* range0,
                         const int* range1, float* mu, float* tr_s, float* a_prime, hipStream_t stream);

/* Teacher half: soft layer mixing (layer_selector.py:110-111), optional resampling to the core grid of
 * n tokens (combined.py:9-14, only when the teacher grid is finer than the student's; g0/g1/glam gather
 * taps, else NULL) and weighted centring (relational.py:37,39).  tok_ptrs: device array of L pointers. */
int basd_teacher_center(const void* const* tok_ptrs, int dtype, const float* mix, int L, long sb, long sn, long sd,
                        int B, int n, int D, const int* g0, const int* g1, const float* glam, const float* omega_t,
                        float* mu, float* tc, hipStream_t stream);
/* The same for G <= 4 groups of mixing weights (mix: (G, L); multi-layer teachers: one group per extraction layer) in
 * ONE pass over the teacher layers: omega_t (G, B, n), mu (G, B, D), tc (G, B, n, D).  Returns BASD_EUNSUPPORTED for
 * more groups or tiles past LDS: call basd_teacher_center per group. */
int basd_teacher_center_multi(const void* const* tok_ptrs, int dtype, const float* mix, int L, int G, long sb, long sn,
                              long sd, int B, int n, int D, const int* g0, const int* g1, const float* glam,
                              const float* omega_t, float* mu, float* tc, hipStream_t stream);
/* Streaming form of the same for row-major teacher tokens and many layers (no LDS tile: full rows are read; the mixed
 * tokens are written uncentred with per-chunk weighted column sums, a second pass folds the sums in a fixed order and
 * subtracts the mean in place).  scratch: basd_teacher_center_stream_scratch_floats() floats.  BASD_EUNSUPPORTED: more
 * than 4 groups or features not contiguous (sd != 1). */
long basd_teacher_center_stream_scratch_floats(int G, int B, int n, int D);
int basd_teacher_center_stream(const void* const* tok_ptrs, int dtype, const float* mix, int L, int G, long sb, long sn,
                               long sd, int B, int n, int D, const int* g0, const int* g1, const float* glam,
                               const float* omega_t, float* mu, float* tc, float* scratch, hipStream_t stream);

/* G[b] = P[b] P[b]^T accumulated in fp64 on v_mfma_f64_16x16x4_f64 (the bmm of relational.py:47,
 * reduced to the teacher grid). */
int basd_gram_f64(const float* p, long p_batch_stride, int n, int D, int batch, double* g, long g_batch_stride,
                  hipStream_t stream);

/* fp64 Cholesky of (possibly singular) PSD matrices; L full row-major. */
/* basd_gram_f64 with the contraction split over `splits` workgroups per matrix (few matrices, long feature axis);
 * slabs: splits * batch * n * n doubles of scratch, folded in a fixed order; g contiguous (batch, n, n). */
int basd_gram_f64_split(const float* p, long p_batch_stride, int n, int D, int batch, int splits, double* slabs,
                        double* g, hipStream_t stream);

int basd_chol_f64(const double* g, long g_batch_stride, int n, int batch, double* l, long l_batch_stride,
                  hipStream_t stream);

/* W[b] = [L_a^T L_b[b % lb_period] ; L_b[b % lb_period]]  (2n x n column-major fp32) -- the input of
 * basd_jacobi_onesided.  lb_period < batch: one teacher factor per sample shared by all extraction layers. */
int basd_stack_product(const double* la, const double* lb, long l_batch_stride, int n, int batch, int lb_period,
                       float* w, long w_batch_stride, hipStream_t stream);

/* Per sample: tr_t, nuclear norm (relational.py:48), loss_b = tr_s + tr_t - 2 nuc (relational.py:50),
 * and K' = Y Sigma^+ Y^T for the backward (nullable). */
int basd_procrustes_finalize(const float* w, long w_batch_stride, const float* sigma, int n, int n_s, int batch,
                             int t_period /* gb, omega indexed by b % t_period */,
                             const double* gb, long g_batch_stride, const float* omega, const int* tap0,
                             const int* tap1, const float* lam, const float* tr_s_part, int tr_slabs, float* tr_s,
                             float* tr_t, float* nuc, float* loss, float* k_prime, hipStream_t stream);

/* basd_student_project, and the student gradient dX = (*scale_ptr * scale_const) * w_s * ((x_s - mu) - interp(K' A')[s])
 * (autograd of relational.py:36-50 with respect to the student tokens), for all E extraction layers in ONE launch each.
 * x_ptrs: device table of E base pointers (common strides); omega + e * omega_e_stride (0 = one weight vector for all
 * layers); the other operands are laid out (E, B, ...); scale_ptr[e] = upstream gradient of layer e.
 * basd_student_project_multi returns BASD_EUNSUPPORTED where its vectorised LDS-staged kernel does not apply (rows not
 * 16-byte aligned, slab over 64 KB): fall back to basd_student_project per layer. */
int basd_student_project_multi(const void* const* x_ptrs, int dtype, long sb, long sn, int E, int B, int n_s, int n_t,
                               int D, int ptrs_16B_aligned, const float* omega, long omega_e_stride, const int* tap0,
                               const int* tap1, const float* lam, const int* range0, const int* range1, float* mu,
                               float* tr_s, float* a_prime, hipStream_t stream);
int basd_student_grad_multi(const void* const* x_ptrs, int dtype, long sb, long sn, int E, int B, int n_s, int n_t,
                            int D, const float* omega, long omega_e_stride, const float* mu, const float* h,
                            const int* tap0, const int* tap1, const float* lam, const float* scale_ptr,
                            float scale_const, float* dx, const float* tnorm2, float* gomega, hipStream_t stream);
/* H = K' A' (basd_gemm_tn) and basd_student_grad_multi in ONE launch for cores of n_t <= 64 tokens: each workgroup
 * forms its 64-feature slab of H in LDS (K' through the scalar cache) and streams the sample's token rows once, so H
 * never goes to memory.  k_prime (E, B, n_t, n_t) as basd_procrustes_finalize writes it (symmetric), a_prime
 * (E, B, n_t, D).  Returns BASD_EUNSUPPORTED for larger cores or rows that are not 16-byte aligned: use the two-call
 * form (autograd of relational.py:36-50 either way). */
int basd_student_grad_fused(const void* const* x_ptrs, int dtype, long sb, long sn, int E, int B, int n_s, int n_t,
                            int D, int ptrs_16B_aligned, const float* omega, long omega_e_stride, const float* mu,
                            const float* k_prime, const float* a_prime, const int* tap0, const int* tap1,
                            const float* lam, const float* scale_ptr, float scale_const, float* dx,
                            hipStream_t stream);

/* The whole forward of relational.py:22-50 for E extraction layers against the (mixed) teacher -- and, when `dx` is
 * set, the student-token gradients for the upstream gradients `grad_layers` -- queued by ONE call: the launches of
 * basd_token_weights, basd_teacher_center, basd_student_project(_multi), basd_gram_f64 x2, basd_chol_f64,
 * basd_stack_product, basd_jacobi_onesided, basd_procrustes_finalize (transposed cores of n <= 64 with k_prime set:
 * basd_procrustes_finish_transposed) [, basd_student_grad_fused or basd_gemm_tn + basd_student_grad_multi] in
 * that order (a dozen FFI calls from Python cost several times the launches themselves, and that host time sat in
 * front of the caller's stream).  All fields are 8 bytes wide; pointers are device memory except student_host_ptrs.
 *   G = 1: the teacher side is shared by all layers (one teacher layer: mixing weights exactly 1), else G = E.
 *   n = min(n_s, n_t): the core grid.  Arrays: omega (G,B,n_s), omega_t (G,B,n), raw (G,B,n_a) nullable,
 *   mu_t (G,B,d_t), tc (G,B,n,d_t), mu_s (E,B,d_s), tr_part (plan field 12; at most E*B*ceil(d_s/32)),
 *   tr_s/tr_t/nuc/loss_b (E,B),
 *   a_prime (E,B,n,d_s), g_all/l_all ((E+G)B,n,n) fp64, W (EB,n,2n), sigma (EB,n),
 *   jflags basd_jacobi_workspace_ints(EB, max_sweeps) ints, sweeps (EB) ints nullable, k_prime (EB,n,n) nullable,
 *   h (EB,n,d_s) + dx (E,B,n_s,d_s) + grad_layers (E): only for the gradients. */
typedef struct BasdProcrustesArgs {
    const void* const* student_ptrs;       /* device table of E pointers */
    const void* const* student_host_ptrs;  /* the same E pointers in host memory (per-layer fallback) */
    long s_dtype, s_sb, s_sn, s_aligned;
    const void* const* tok_ptrs;           /* device table of L pointers */
    long t_dtype, t_sb, t_sn, t_sd;
    const void* const* attn_ptrs;          /* device table of L pointers */
    long a_dtype, a_sb, a_sh, a_sq, a_sk;
    const float* mix;                      /* (G, L) */
    long E, L, G, B, n_s, n_t, d_s, d_t, H, A, has_cls, n_a, n, max_sweeps;
    const int* atap0; const int* atap1; const float* alam;                                  /* n_a -> n_s */
    const int* tap0; const int* tap1; const float* lam; const int* range0; const int* range1;   /* n -> n_s, student side */
    const int* g0; const int* g1; const float* glam;                                        /* teacher gather n_t -> n */
    float* omega; float* omega_t; float* raw; float* mu_t; float* tc; float* mu_s; float* tr_part; float* tr_s;
    float* a_prime;
    double* g_all; double* l_all;
    float* W; float* sigma; int* jflags; int* sweeps;
    float* tr_t; float* nuc; float* loss_b; float* k_prime;
    float* h; float* dx; const float* grad_layers;
    double* g_slabs; long g_splits;     /* nullable / <= 1: teacher Gram unsplit; else g_splits * G*B*n*n doubles of scratch */
    /* UW-SO combination (combined.py:76-85) inside the call, nullable: uw_ce = the base loss (one fp32 on the device);
     * uw_out (4 + 2 E floats) receives w_ce, w_geo, total, geo, then E x w_geo / E, then the E per-layer means.  The
     * student gradients (dx) are then those of `total` for a unit upstream gradient and grad_layers is ignored. */
    const float* uw_ce; float* uw_out;
    /* nullable: basd_jacobi_twopass_workspace_bytes(n, E*B, max_sweeps) bytes; offered, the SVD of stacked cores
     * takes basd_jacobi_stacked_twopass where that covers the shape (plan field 7) */
    void* jac_ws;
    /* nullable, only read when `raw` is set (gradients through the mixing weights): E*B * 2n*n floats.  Offered, the
     * planner may take the transposed cores for such a call and U Sigma is rebuilt here (basd_ustack_from_transposed);
     * sigma_u: E*B * n floats, the norms of its columns (what the backward pairs with w_stack).  Plan field 11 says
     * whether the backward finds U Sigma here or in W / sigma: when the stacked cores are taken, neither is written. */
    float* w_stack; float* sigma_u;
} BasdProcrustesArgs;
int basd_procrustes_forward_fused(const BasdProcrustesArgs* args, hipStream_t stream);
/* The routes basd_procrustes_forward_fused takes for `args` under the current hooks (host only: no HIP call, usable
 * without a GPU; pointers are tested for presence and 16-byte alignment, never dereferenced, so any non-null aligned
 * value stands for "offered").  One planner (csrc/procrustes_plan.h) answers here and in the call.  out20:
 *    0 teacher centring: 1 stream, four features per thread; 2 stream; 3 all groups in one launch; 4 per group;
 *      5 given (basd_procrustes_plan_query_cached only)
 *    1 student projection: 1 all layers in one launch, 2 per layer;  2 features per trace slab (32 / 64);  3 slabs
 *    4 teacher Gram split (0 / 1);  5 Cholesky: 1 in LDS, 2 blocked;  6 cores: 1 transposed, 2 stacked [M; L_b]
 *    7 SVD: 1 one-sided Jacobi on the transposed cores, 2 basd_jacobi_stacked_twopass with jac_ws (one-sided where
 *      that does not cover the order), 3 one-sided on the stacked cores
 *    8 finish: 1 basd_procrustes_finish_transposed, 2 basd_procrustes_finalize + basd_kprime_from_transposed,
 *      3 basd_procrustes_finalize, 4 the same with K' by its tiled kernel
 *    9 U Sigma rebuilt into w_stack (0 / 1);  10 student gradient: 0 none, 1 fused, 2 basd_gemm_tn + multi
 *   11 U Sigma afterwards in: 1 W (with sigma), 2 w_stack (with sigma_u)
 *   12 floats of tr_part the projection writes;  13 floats of W the stream centring borrows
 *   14..19 dynamic LDS bytes of the centring, projection, Gram, Cholesky, finish and fused-gradient kernels (0: none)
 * A stage with no route is 0 and the status BASD_EUNSUPPORTED; arguments the call rejects give BASD_EINVAL. */
int basd_procrustes_plan_query(const BasdProcrustesArgs* args, long* out20);

/* ---- the teacher side of a single-layer teacher, given instead of computed ------------------------------------
 * With one teacher layer (L == 1, G == 1) the mixing weight is exactly 1 (layer_selector.py:110-112: softmax over one
 * distance), so the teacher enters relational.py:22-39 only through three per-sample arrays that are a function of the
 * teacher's input image alone: the fp64 Gram of the centred, weighted teacher tokens on the core grid (the teacher
 * slot of g_all, rows E*B .. E*B + B), omega (B, n_s) and omega_t (B, n).
 *
 * basd_procrustes_forward_cached is basd_procrustes_forward_fused for G == 1 with those three as INPUTS: tok_ptrs,
 * attn_ptrs, mix, mu_t, tc and g_slabs are not read, basd_token_weights, basd_teacher_center* and the teacher's
 * basd_gram_f64(_split) are not queued, and everything from the student projection on -- student Grams, ONE Cholesky
 * launch over all (E + 1) B matrices, cores, SVD, finish, UW-SO, student gradient -- is queued in the same order by the
 * same routes, so with the same three arrays every output has the bits of the uncached call.  G != 1: BASD_EINVAL.
 * basd_procrustes_plan_query_cached answers for it from the same planner: field 0 is 5 ("given"), fields 4, 13 and 14
 * are 0, every other field is what basd_procrustes_plan_query answers for the same argument block. */
int basd_procrustes_forward_cached(const BasdProcrustesArgs* args, hipStream_t stream);
int basd_procrustes_plan_query_cached(const BasdProcrustesArgs* args, long* out20);
/* The other half: those three arrays computed BY THEMSELVES, for any set of images, without a student.
 * basd_procrustes_teacher_side queues the part of basd_procrustes_forward_fused ahead of its student projection and then
 * its teacher Gram, through the same code (fused.hip: teacher_weights_and_centring, teacher_gram): basd_token_weights,
 * the centring route of the plan (L == 1, G == 1: basd_teacher_center), and basd_gram_f64_split (g_slabs set and
 * g_splits > 1; g_slabs: g_splits * B*n*n doubles) or basd_gram_f64.  No projection, Cholesky, SVD or finish.
 *   read:    tok_ptrs, t_*, attn_ptrs, a_*, mix (one float, 1), L, G, B, n_s, n_t, d_t, H, A, has_cls, n_a, n, the
 *            taps (atap*, tap0 / tap1 / lam, g0 / g1 / glam), raw (nullable), g_slabs, g_splits
 *   written: omega (B, n_s), omega_t (B, n), scratch mu_t (B, d_t) and tc (B, n, d_t), and g_all, which for THIS call
 *            is the (B, n, n) fp64 teacher Gram itself (there are no student Grams ahead of it)
 *   not read: E, d_s and every student field; every array behind the Grams.
 * Row b of the three outputs depends on image b and on g_splits alone -- not on B, on b or on the other images: the
 * token weights and the centring work per sample, and the split Gram folds a matrix's g_splits slabs in a fixed order.
 * With the g_splits of an uncached call the rows are bit for bit those that call leaves in its teacher slot.
 * L != 1, G != 1, a core grid past the centring kernel's LDS (n > ~580) or past the Gram's: BASD_EUNSUPPORTED before
 * anything is queued.  basd_procrustes_plan_query_teacher_side answers for it from the same predicates: fields 0, 4,
 * 13, 14 and 16 are those of basd_procrustes_plan_query for the same teacher arguments, every student-side field is 0
 * ("none"), and the status is BASD_OK or BASD_EUNSUPPORTED by the teacher-side stages alone. */
int basd_procrustes_teacher_side(const BasdProcrustesArgs* args, hipStream_t stream);
int basd_procrustes_plan_query_teacher_side(const BasdProcrustesArgs* args, long* out20);
/* The cache of those arrays, one row per dataset image: cache_g (capacity, n, n) fp64, cache_omega (capacity, n_s),
 * cache_omega_t (capacity, n), all dense.  One launch each:
 *   basd_teacher_cache_store scatters the B rows a call has just produced (g (B, n, n), omega (B, n_s), omega_t (B, n),
 *     dense) into the cache rows index[b]; basd_teacher_cache_load gathers the cache rows index[b] into row b of the
 *     places the cached call reads.
 * index: (B) int64 on the device.  Offsets are formed in 64 bits (capacity * n * n * 8 passes 2^32 for real datasets).
 * The Grams move as 16-byte pairs where n * n is even and both Gram bases are 16-byte aligned, as doubles otherwise
 * (n = 49).  An index outside [0, capacity) copies nothing (callers check on the host).  A repeated index is legal in
 * load.  In store, launches with equal indices race on that row: hand over EQUAL rows for them (the teacher side is a
 * function of the image), then every interleaving leaves the same bytes.  B <= 65535. */
int basd_teacher_cache_store(const double* g, const float* omega, const float* omega_t, const long* index, int B, int n,
                             int n_s, long capacity, double* cache_g, float* cache_omega, float* cache_omega_t,
                             hipStream_t stream);
int basd_teacher_cache_load(const double* cache_g, const float* cache_omega, const float* cache_omega_t,
                            const long* index, int B, int n, int n_s, long capacity, double* g, float* omega,
                            float* omega_t, hipStream_t stream);
/* Test / tuning hook, read by the planner: 0 = always the stacked cores [M; L_b] (riding rows); 1 = the transposed
 * cores where they apply (default: >= 128 cores, basd_jacobi_plain4_fits(n), and -- with a gradient through the mixing
 * weights -- w_stack offered); 2 = the same for any batch; negative = keep.  Process-wide. */
int basd_procrustes_tuning(int transposed_cores);

/* The two pieces of the transposed route (relational.py:47-48 and its autograd): M = L_a^T L_b alone, row-major and
 * compact at w + b * w_batch_stride -- as a column-major matrix that is M^T, whose one-sided Jacobi leaves V Sigma in
 * the columns -- and K' = Y Sigma^+ Y^T with Y = L_b V formed from those columns (z: n x n floats of scratch per
 * matrix at z + b * z_batch_stride). */
int basd_stack_product_t(const double* la, const double* lb, long l_batch_stride, int n, int batch, int lb_period,
                         float* w, long w_batch_stride, hipStream_t stream);
int basd_kprime_from_transposed(const float* w, long w_batch_stride, const float* sigma, int n, int batch,
                                const double* lb, long l_batch_stride, int lb_period, float* z, long z_batch_stride,
                                float* k_prime, hipStream_t stream);
/* relational.py:47-50 behind the Jacobi of the transposed route for cores of n <= 64 tokens, in ONE launch: the
 * per-sample terms of basd_procrustes_finalize (called with k_prime == NULL) and the K' of basd_kprime_from_transposed,
 * bit for bit (same reduction order, every sum one fmaf per term in ascending order), with X = V Sigma and L_b read
 * once and Z kept on chip: no z buffer.  Arguments as in those two.  Returns BASD_EUNSUPPORTED without launching for
 * n > 64 or batch > 65535: call the two. */
int basd_procrustes_finish_transposed(const float* w, long w_batch_stride, const float* sigma, int n, int n_s,
                                      int batch, int t_period /* gb, omega indexed by b % t_period */,
                                      const double* gb, long g_batch_stride, const float* omega, const int* tap0,
                                      const int* tap1, const float* lam, const float* tr_s_part, int tr_slabs,
                                      float* tr_s, float* tr_t, float* nuc, float* loss, const double* lb,
                                      long l_batch_stride, int lb_period, float* k_prime, hipStream_t stream);
/* Test / measurement hook of basd_procrustes_forward_fused: 1 (default) = basd_procrustes_finish_transposed where it
 * applies, 0 = always basd_procrustes_finalize + basd_kprime_from_transposed; negative = query only.  Returns the
 * previous setting (not a status).  Process-wide. */
int basd_procrustes_finish_tuning(int fused);
/* The transposed route for steps whose backward goes through the mixing weights (multi-layer teachers; autograd of
 * relational.py:47-48 w.r.t. the teacher side reads U Sigma, the top half of the stacked cores: basd_teacher_factor*):
 * basd_ustack_stash, between basd_stack_product_t and the Jacobi, copies M (row-major, compact at wc) into the unused
 * bottom half of the stacked buffer w_stack (E*B x 2n*n floats); basd_ustack_from_transposed, behind the Jacobi, forms
 * M V from it and X = V Sigma (compact at x, what the Jacobi left) in `scratch` (n*n floats per core), makes its columns
 * orthogonal relative to their own norms with a short one-sided Jacobi (orthogonality was enforced on V Sigma: M V has
 * U Sigma's columns to tol sigma_max only; sigma_u receives their norms) and places them in the top half, stacked layout.
 * The backward reads w_stack with sigma_u. */
int basd_ustack_stash(const float* wc, long wc_batch_stride, int n, int batch, float* w_stack, long w_stack_stride,
                      hipStream_t stream);
int basd_ustack_from_transposed(const float* x, long x_batch_stride, const float* sigma, int n, int batch,
                                float* w_stack, long w_stack_stride, float* scratch, long scratch_batch_stride,
                                float* sigma_u, int max_sweeps, int* jflags, hipStream_t stream);

/* x *= num / den unless the ratio is exactly 1 (then the launch returns at once): the upstream gradient of a loss that
 * was differentiated for a unit one.  num, den: one fp32 each on the device, den nullable (= 1). */
int basd_scale_unless_one(float* x, long count, const float* num, const float* den, hipStream_t stream);

/* The base criterion of BASDLoss (combined.py:56) when it is the stock torch.nn.CrossEntropyLoss (mean reduction, no
 * class weights): per-row losses (already divided by the number of rows that are not ignored; loss = their sum) and
 * d loss / d logits in ONE launch.  Exactly one of labels (int64 class indices, B) / probs (fp32 soft targets (B, C),
 * row stride pld); label smoothing as in torch: t' = (1 - eps) t + eps / C. */
int basd_cross_entropy(const void* logits, int dtype, long ld, int B, int C, const long* labels, const float* probs,
                       long pld, float label_smoothing, long ignore_index, float* row_loss, float* dlogits,
                       hipStream_t stream);

/* ---- stream ordering helpers ----------------------------------------------------------------------- */

/* Events to order two streams from inside a library call (basd_tridiag_ranked's mid_event): opaque hipEvent_t handles. */
int basd_event_create(void** out);
int basd_event_destroy(void* event);
int basd_stream_wait_event(hipStream_t stream, void* event);
int basd_event_record(void* event, hipStream_t stream);
int basd_event_synchronize(void* event);      /* blocks the calling host thread */
/* A stream of priority level -1 (highest of the device's range), 0 (default) or +1 (lowest). */
int basd_stream_create_priority(void** out, int level);
/* diagnostics: events that carry a time stamp (basd_event_create makes them without), and the time between two */
int basd_event_create_timed(void** out);
int basd_event_elapsed_ms(void* from, void* to, float* ms_out);

/* ---- multi-layer teachers only: gradients through the mixing weights and the principal angles ------ */

/* Kt = Q - K'' with d loss_b / d T_c = 2 Kt T_c (autograd of relational.py:36-50 w.r.t. the mixed teacher
 * tokens of layer_selector.py:111), and |t_hat_c[s]|^2 per student token. */
int basd_teacher_factor(const float* w, long w_batch_stride, const float* sigma, int n, int n_s, int batch,
                        const double* la, const double* gb, long g_batch_stride, const float* omega,
                        const int* tap0, const int* tap1, const float* lam, const int* range0, const int* range1,
                        float* kt, float* tnorm2, hipStream_t stream);
/* The same for cores past LDS (basd_teacher_factor returns BASD_EUNSUPPORTED for n > 199): both contractions tiled,
 * Z = L_a U Sigma^-1/2 through z_scratch, (batch, n, n) floats of device scratch. */
int basd_teacher_factor_tiled(const float* w, long w_batch_stride, const float* sigma, int n, int n_s, int batch,
                              const double* la, const double* gb, long g_batch_stride, const float* omega,
                              const int* tap0, const int* tap1, const float* lam, const int* range0, const int* range1,
                              float* kt, float* tnorm2, float* z_scratch, hipStream_t stream);

/* partial[e][b][l] = <R[e][b], teacher layer l on the core grid>: d loss / d mix_l through the tokens
 * (layer_selector.py:111). */
int basd_mix_grad_tokens(const float* r, const void* const* tok_ptrs, int dtype, int L, long sb, long sn, long sd,
                         int E, int B, int n, int D, const int* g0, const int* g1, const float* glam, float* partial,
                         hipStream_t stream);

/* The same in ONE pass over the teacher layers for all E <= 4 extraction layers (BASD_EUNSUPPORTED beyond).  scratch:
 * basd_mix_grad_tokens_scratch_floats() floats of device memory; per-chunk sums are folded in a fixed order. */
long basd_mix_grad_tokens_scratch_floats(int E, int B, int L, int n);
int basd_mix_grad_tokens_onepass(const float* r, const void* const* tok_ptrs, int dtype, int L, long sb, long sn, long sd,
                                 int E, int B, int n, int D, const int* g0, const int* g1, const float* glam,
                                 float* partial, float* scratch, hipStream_t stream);

/* partial[e][b][l] = d loss / d mix_l through the attention-derived token weights
 * (layer_selector.py:112 + relational.py:22-34). */
int basd_token_weight_bwd(const float* gomega, const float* raw, int E, int B, int n_a, int n_s, const int* atap0,
                          const int* atap1, const float* alam, const int* arange0, const int* arange1,
                          const void* const* attn_ptrs, int dtype, int L, long sb, long sh, long sq, long sk, int H,
                          int A, int has_cls, float* partial,
                          float* graw_out /* nullable: (E, B, n_a) d loss_b / d raw attention-grid weights */,
                          hipStream_t stream);

/* [masked cosine matrix ; identity] stacks (2 kmax x kmax, column-major) for the principal-angle SVD with
 * right singular vectors (backward of layer_selector.py:99). */
int basd_build_angle_stack(const float* cos, int kmax, const int* k_arr, int items, float* out, hipStream_t stream);

/* gWt[item][j][i] = d (d_grass_sq[item]) / d W[i][j] * gd[item]  (backward of layer_selector.py:99-105). */
int basd_grassmann_distance_bwd(const float* stack, const float* colnorm, int kmax, const int* k_arr, const float* sw,
                                int sw_stride, const int* sw_index, const float* gd, int items, float* gwt,
                                hipStream_t stream);

/* K2[i][j] = (M[i][j] - M[j][i]) / (lam_j - lam_i): eigenvector perturbation of the student Gram
 * (backward of torch.linalg.svd at layer_selector.py:92). */
int basd_eigvec_k2(const float* m, const float* lam, int D, int kmax, int batch, float* k2, hipStream_t stream);

/* Stand-alone `_align_token_count` (combined.py:9-14): out (B, n_out, D) fp32 contiguous; and its adjoint. */
int basd_resample_tokens(const void* x, int dtype, long sb, long sn, long sd, int B, int n_in, int n_out, int D,
                         const int* tap0, const int* tap1, const float* lam, float* out, hipStream_t stream);
int basd_resample_tokens_adjoint(const float* dy, int B, int n_in, int n_out, int D, const int* tap0,
                                 const int* tap1, const float* lam, const int* range0, const int* range1, float* dx,
                                 hipStream_t stream);

/* ---- the optimizer: schedule-free AdamW over all parameters in one launch ---------------------------- */

/* One row per parameter tensor (device table).  y: the parameter itself (fp32, the `y` sequence in train mode);
 * z, v: the optimizer's state (`z`, `exp_avg_sq`); grad: NULL = no gradient this step, the tensor is skipped;
 * group: index into the per-group scalars.  Any pointer may be only 4-byte aligned (16-byte accesses are used
 * where y, z, v -- and, separately, grad -- allow them). */
typedef struct BasdSfAdamwTensor {
    float* y;
    float* z;
    float* v;
    float* grad;
    long numel;
    long group;
} BasdSfAdamwTensor;

/* Host-computed scalars of one parameter group for one step (HOST memory; they reach the kernel by value). */
typedef struct BasdSfAdamwGroup {
    double lr;                 /* group lr x warm-up factor (`scheduled_lr`) */
    double ckp1;               /* weight / weight_sum */
    double bias_correction2;   /* 1 - beta2^(k+1) */
    double beta1, beta2, eps, weight_decay;
} BasdSfAdamwGroup;

#define BASD_SFADAMW_MAX_GROUPS 8

/* Elements per chunk of the chunk lists below. */
int basd_sfadamw_chunk(void);

/* replaces: `self.optimizer.step()` + `self.optimizer.zero_grad()`  src/training/trainer.py:158-159 with the
 * `AdamWScheduleFree` of trainer.py:54-58 (incl. the second parameter group of :74-76).  Per element
 *   g = grad * grad_scale;  v = beta2 v + (1 - beta2) g g;  gn = g / (sqrt(v / bias_correction2) + eps) + weight_decay y;
 *   y = y + ckp1 (z - y);  y = y + lr (beta1 (1 - ckp1) - 1) gn;  z = z - lr gn;  grad = 0 if zero_grad.
 * chunks: n_chunks pairs (row of `table`, chunk index inside that tensor) on the device, covering every tensor.
 * groups: n_groups <= BASD_SFADAMW_MAX_GROUPS entries on the HOST.  ONE launch; n_chunks == 0 launches nothing. */
int basd_sfadamw_step(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, const BasdSfAdamwGroup* groups,
                      int n_groups, float grad_scale, int zero_grad, hipStream_t stream);

/* replaces: `self.optimizer.train()` / `self.optimizer.eval()`  src/training/trainer.py:180,:184:
 * y <- y + weights[group] (z - y) for every tensor of the table, ONE launch (grad is not read).
 * weights: n_groups <= BASD_SFADAMW_MAX_GROUPS floats on the HOST. */
int basd_sfadamw_swap(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, const float* weights,
                      int n_groups, hipStream_t stream);

/* What the clipped step decided, on the DEVICE (32 bytes, 8-byte aligned; zero it once).  norm_sq: the fp64 sum of
 * the squared raw gradients; norm = |grad_scale| sqrt(norm_sq): the 2-norm of the gradients as the update saw them;
 * (fp32: it reads inf past 3.4e38 while norm_sq, which the guard looks at, is still finite); coef: the clipping
 * coefficient that was applied; skipped: 1 if this step left y, z, v alone; skipped_total: the number of such steps
 * since the struct was zeroed. */
typedef struct BasdGradVerdict {
    double norm_sq;
    float norm;
    float coef;
    int skipped;
    int skipped_total;
    int pad[2];
} BasdGradVerdict;

/* Number of partial sums basd_grad_sqnorm writes for a chunk list of n_chunks entries: a pure function of n_chunks,
 * 1 <= value <= 1024.  It is the grid of the norm pass and thereby fixes the order of summation. */
int basd_grad_sqnorm_parts(int n_chunks);

/* replaces: the norm half of `torch.nn.utils.clip_grad_norm_` (the reference's trainer does not clip; a trainer on
 * `accelerate` would call `accelerator.clip_grad_norm_`) over the gradients of ALL tensors of the table, as n_partials
 * fp64 partial sums of squares.  Same table and chunk list as
 * basd_sfadamw_step; rows with grad == NULL are skipped.  n_partials (= basd_grad_sqnorm_parts(n_chunks)) workgroups
 * walk the chunk list with a grid stride; every lane squares its fp32 elements in fp64 (exact) and accumulates them
 * in fp64; lanes are combined in a fixed order (butterfly inside a wave, the waves in index order through LDS) and
 * workgroup b stores partials[b].  The same gradients give the same bits on every call.  16-byte loads where the
 * gradient pointer allows them, 4-byte loads for a misaligned gradient and the last numel % 4 elements.  No workgroup
 * reads what another wrote: the partials are summed by the kernel that consumes them (basd_sfadamw_step_clipped).
 * partials: n_partials doubles on the device, 8-byte aligned, all overwritten.  ONE launch; n_chunks == 0 launches
 * nothing. */
int basd_grad_sqnorm(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks, double* partials, int n_partials,
                     hipStream_t stream);

/* replaces: `clip_grad_norm_(params, max_norm)` + a non-finite guard + `optimizer.step()` + `optimizer.zero_grad()`.
 * basd_sfadamw_step behind a prologue: every workgroup sums the n_partials partials of basd_grad_sqnorm in one fixed
 * order (the same in every workgroup) and forms in fp64
 *   norm_sq = sum partials;  norm = |grad_scale| sqrt(norm_sq);
 *   coef = max_norm > 0 and max_norm / (norm + 1e-6) < 1 ? max_norm / (norm + 1e-6) : 1, rounded once to fp32
 *          (the `clip_grad_norm_` formula; a NaN norm clips nothing);
 *   skip = skip_nonfinite and norm_sq is not finite (one inf or NaN gradient element makes it so; finite fp32
 *          gradients cannot: 2^25 elements of 3.4e38^2 are far inside fp64).
 * Not skipped: the recurrence of basd_sfadamw_step with g = grad * fl32(grad_scale * coef) -- with coef == 1 the bytes
 * of y, z, v and grad are those of basd_sfadamw_step with grad_scale, else those with fl32(grad_scale * coef).
 * Skipped: y, z and v are not written; the gradients are still zeroed if zero_grad.
 * Lane 0 of workgroup 0 writes *verdict (skipped_total by a plain read-modify-write: launches are stream-ordered).
 * partials, verdict: on the device, non-null, 8-byte aligned; n_partials == basd_grad_sqnorm_parts(n_chunks).
 * max_norm <= 0 = no clipping.  ONE launch; n_chunks == 0 launches nothing (and leaves *verdict alone). */
int basd_sfadamw_step_clipped(const BasdSfAdamwTensor* table, const int* chunks, int n_chunks,
                              const BasdSfAdamwGroup* groups, int n_groups, float grad_scale, int zero_grad,
                              const double* partials, int n_partials, double max_norm, int skip_nonfinite,
                              BasdGradVerdict* verdict, hipStream_t stream);

/* diagnostics: kernel launches made by the entry points above (step, swap, norm pass, clipped step) since the
 * library was loaded (process-wide). */
long basd_sfadamw_launches(void);

/* ---- validation: loss, top-1 and top-k of one batch in one launch ------------------------------------ */

/* replaces: the body of the batch loop of `evaluate_model`  src/evaluation/metrics.py:19-55 -- the column gather
 * `outputs[:, valid_indices]`, `criterion(outputs, targets) * B`, and the two `MulticlassAccuracy.update` calls.
 * logits: (B, C) fp32 / bf16 read in place with row stride ld (elements); class_index: K columns of it on the device
 * (NULL with K == C: all classes in order); labels: B int64 positions in [0, K).  Per row b, with z_j the j-th selected
 * logit and y = labels[b]:
 *   loss_b = lse(z) - (1 - eps) z_y - eps / K sum_j z_j      (fp32, row maximum subtracted; not divided by a count;
 *                                                              the last term is left out when eps == 0)
 *   rank_b = #{j : z_j > z_y} + #{j < y : z_j == z_y}        (a tie goes to the lower class position)
 * and, all by 64-bit integer atomic adds (agent scope), so that the result does not depend on the order of arrival:
 *   state[0] += llrint(loss_b * 2^32);  state[1] += 1;  state[2] += rank_b == 0;  state[3] += rank_b < top_k.
 * A row that cannot be represented -- y outside [0, K), a NaN among its K logits, loss_b not finite or >= 2^24, a
 * class_index entry outside [0, C) (not read) -- is a miss at every k, adds 1 to state[4] and nothing to state[0].
 * state: 5 words on the device, accumulated into (zero them to start).  ONE launch, no memset, no workspace; B == 0
 * launches nothing.  1 <= top_k <= K. */
int basd_eval_batch(const void* logits, int dtype, long ld, int B, int C, const int* class_index, int K,
                    const long* labels, float label_smoothing, int top_k, long long* state, hipStream_t stream);

/* ---- batch preparation: MixUp / CutMix, soft targets and the uint8 conversion in one launch ------------ */

/* Channels that may carry their own mean / std (they travel in the kernel arguments). */
#define BASD_MIX_MAX_STAT_CHANNELS 4

/* replaces: `self.mixup_cutmix(images, targets)`  src/training/trainer.py:89-92, :141 (RandomChoice([MixUp, CutMix]) of
 * torchvision.transforms.v2 incl. the one-hot soft targets), and for uint8 sources the loader's
 * `ToDtype(float32, scale=True)` + `Normalize(mean, std)`.
 * src: dense NCHW (B, C, H, W), fp32 / bf16 / uint8 (BASD_DTYPE_U8); dst: dense NCHW of the same shape, fp32 / bf16,
 * not overlapping src (checked).  The partner of row i is row (i - 1) mod B (`roll(1, 0)`).  Every step below is ONE
 * fp32 operation rounded to nearest, nothing is contracted; a bf16 dst is rounded once, to nearest even, at the end.
 *   v(x) = float(x)  (fp32, bf16);   v(u) = ((float(u) / 255) - mean_c) / std_c  (uint8, two true divisions;
 *                                     mean = std = NULL: mean 0, std 1 for any C; otherwise C <= 4 floats each, HOST)
 *   kind 0 (none):    out = v(x_i)
 *   kind 1 (MixUp):   out = v(x_{i-1}) * fp32(1.0 - lam) + v(x_i) * fp32(lam)                (1.0 - lam in double)
 *   kind 2 (CutMix):  out = v(x_{i-1}) for y1 <= y < y2 and x1 <= x < x2, v(x_i) elsewhere   (an empty box: a copy)
 * labels (nullable; B int64 on the device) given: targets, dense (B, K) fp32, is written whole in the same launch,
 *   T[i][k] = [y_{i-1} == k] * fp32(1.0 - lam_targets) + [y_i == k] * fp32(lam_targets);
 * a label outside [0, K) in row i or in its partner makes row i of T NaN (nothing is read or written out of bounds).
 * ONE launch, no memset, no workspace, no host-to-device copy; B == 0 launches nothing.  16-byte accesses where the
 * rows' addresses allow, narrower ones for rows at other offsets and for the last C*H*W % width elements. */
int basd_mix_batch(const void* src, int src_dtype, void* dst, int dst_dtype, int B, int C, int H, int W, int kind,
                   double lam, int y1, int y2, int x1, int x2, const float* mean /* host */,
                   const float* std /* host */, const long* labels, int K, double lam_targets, float* targets,
                   hipStream_t stream);

/* ---- teacher attention importance from the qkv projection's output in one launch ----------------------- */

#define BASD_ATTN_CLS_ROW 0
#define BASD_ATTN_QUERY_MEAN 1

/* replaces: the attention hook `qkv = mod.qkv(x).reshape(B, N, 3, nh, hd).permute(2, 0, 3, 1, 4);
 *           attn = (q @ k.transpose(-2, -1)) * scale; attn.softmax(dim=-1)`  src/models/teacher.py:27-39, reduced to
 *           what the loss reads of it, `attn.mean(dim=1)[:, 0, 1:]` / `attn.mean(dim=1).mean(dim=1)`
 *           src/losses/relational.py:22-27 (the mean over heads stays with the loss: layer mixing comes first).
 * qkv: the OUTPUT of a fused projection, (B, N, 3 H hd) fp32 / bf16, last axis laid out [3][H][hd] with unit stride;
 * batch / token strides sb / sn (elements) are arbitrary: a view is read in place (16-byte loads where its address and
 * strides allow, element loads otherwise).  out: dense (B, H, N) fp32, written whole.
 *   mode BASD_ATTN_CLS_ROW:     out[b,h,j] = softmax_j(scale q[b,h,0] . k[b,h,j])          (all N columns)
 *   mode BASD_ATTN_QUERY_MEAN:  out[b,h,j] = (1/N) sum_i softmax_j(scale q[b,h,i] . k[b,h,j])
 * Q K^T runs on the matrix cores (bf16 input: v_mfma_f32_32x32x16_bf16, fp32 input: v_mfma_f32_32x32x2_f32, the
 * contraction padded with zeros), fp32 accumulation, fp32 softmax with the row maximum subtracted; the score tiles
 * are recomputed in a second pass over the keys, so nothing of size N^2 is written to memory.  Fixed-order
 * reductions, no atomics: the bits depend on the arguments only.  A NaN or +inf score makes out[b,h,:] of its own
 * (b, h) NaN and nothing else; large finite scores do not overflow.
 * Supported: 1 <= N <= 1025, hd a multiple of 8 up to 128, any B, H >= 1; anything else returns BASD_EUNSUPPORTED
 * before anything is launched.  ONE launch, no workspace, nothing the caller must zero. */
int basd_attn_importance(const void* qkv, int dtype, long sb, long sn, int B, int N, int H, int hd, int mode,
                         float scale, float* out, hipStream_t stream);

/* ---- dataset statistics: exact per-channel sums of uint8 pixels in one launch -------------------------- */

#define BASD_LAYOUT_HWC 0
#define BASD_LAYOUT_CHW 1

/* replaces: the body of the image loop of `get_channel_stats`  src/data/datasets.py:46-68 -- the conversion of every
 *           image to float64 on the host, its per-image `mean` / `var`, and the running merge of those.
 * src: uint8, dense, at ANY byte address (callers pass views):
 *   layout BASD_LAYOUT_HWC: images * pixels pixels of C interleaved bytes (`np.asarray(pil_image)`, a stack of such
 *                           arrays, or any concatenation of ragged images cut at pixel boundaries);
 *   layout BASD_LAYOUT_CHW: images * C planes of `pixels` bytes each (a dense NCHW batch).
 * 1 <= C <= 4.  state: 9 words on the device, ADDED to by 64-bit integer atomic adds (agent scope; zero them to start):
 *   state[0] += images * pixels;   state[1 + c] += sum of x over channel c;   state[5 + c] += sum of x^2 over channel c
 * for c < C; the words of channels >= C are not touched.  The sums are integers and are exact, so the state is the same
 * bits whatever the order of arrival, the launch geometry, the cutting of the data into calls or their number; per
 * channel there is room for 2^63 / 255^2 > 1.4e14 pixels.  Mean and standard deviation are the caller's to form
 * (basd_amd.stats.finish: exact rational arithmetic, rounded once).
 * 16-byte loads behind a head of single bytes up to the first 16-byte boundary (of every plane, in CHW); both sums of
 * a dword by v_dot4_u32_u8.  ONE launch, no memset, no workspace, no copy; at most nine atomic adds per workgroup.
 * images * pixels == 0 launches nothing and returns 0; C outside 1..4, an unknown layout, a negative size, more than
 * 2^40 pixels in one call or more than 2^31 tiles of 3 KiB return BASD_EINVAL before anything is launched.
 * max_blocks: test / tuning hook; 0 = the entry point chooses the grid, > 0 = a cap on its workgroups (the result does
 * not depend on it). */
int basd_channel_stats(const unsigned char* src, int layout, long images, int C, long pixels, long long* state,
                       int max_blocks, hipStream_t stream);

/* ---- TrivialAugmentWide and the horizontal flip of uint8 batches in one launch -------------------------- */

#define BASD_TAUG_IDENTITY 0
#define BASD_TAUG_SHEAR_X 1
#define BASD_TAUG_SHEAR_Y 2
#define BASD_TAUG_TRANSLATE_X 3
#define BASD_TAUG_TRANSLATE_Y 4
#define BASD_TAUG_ROTATE 5
#define BASD_TAUG_BRIGHTNESS 6
#define BASD_TAUG_COLOR 7
#define BASD_TAUG_CONTRAST 8
#define BASD_TAUG_SHARPNESS 9
#define BASD_TAUG_POSTERIZE 10
#define BASD_TAUG_SOLARIZE 11
#define BASD_TAUG_AUTOCONTRAST 12
#define BASD_TAUG_EQUALIZE 13

/* Images of C*H*W bytes up to this are staged in LDS (3 x 224 x 224); larger ones are read from memory twice. */
#define BASD_TAUG_STAGE_BYTES 150528

/* One row of the device table, one per image (64 bytes). */
typedef struct BasdTaugRecord {
    int op;        /* BASD_TAUG_* */
    int flip;      /* non-zero: every read of source pixel (y, x) below reads (y, W - 1 - x): the result is op(flip(image)) */
    int iarg;      /* Posterize: bits */
    float farg;    /* ops 6-9: f = 1 + m as fp32; Solarize: the threshold */
    double a[6];   /* ops 0-5: the inverse affine map, made on the host */
} BasdTaugRecord;

/* replaces: `v2.RandomHorizontalFlip(), v2.TrivialAugmentWide()` of the training transform  src/data/datasets.py:137-144
 *           (torchvision.transforms.v2; 31 magnitude bins, nearest interpolation, fill 0), which the reference runs per
 *           image in Pillow inside its loader's workers.  Which op, which magnitude and whether to flip are the host's
 *           draws (basd_amd.trivial_augment); they arrive as one BasdTaugRecord per image.
 * src: dense NCHW (B, C, H, W) uint8, C in {1, 3}, at any byte address; dst: the same shape, not overlapping src
 * (checked); table: B records on the device; status: one int on the device, OR-ed into (bit 0: a record with an op
 * code outside the table; its image is copied, flipped if the record says so).  This text is the specification; the
 * kernel equals it bit for bit, and it equals Pillow 12 (ImageEnhance, ImageOps, Image.transform, Image.rotate) bit for
 * bit except for rotations at source coordinates within 1/256 of an integer (Pillow walks them in 16.16 fixed point).
 *
 * Ops 0-5 (Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate): output pixel (x, y) takes the source pixel at
 *   sx = floor(a0 (x + 0.5) + a1 (y + 0.5) + a2),  sy = floor(a3 (x + 0.5) + a4 (y + 0.5) + a5),
 * evaluated in fp64 from left to right, every product and sum rounded on its own; 0 where (sx, sy) lies outside the
 * image.  The host's matrices: Identity (1, 0, 0, 0, 1, 0); ShearX by m (1, m, 0, 0, 1, 0) (about the top-left corner,
 * `center=[0, 0]`); ShearY by m (1, 0, 0, m, 1, 0); TranslateX by t = int(m) (1, 0, -t, 0, 1, 0); TranslateY by t
 * (1, 0, 0, 0, 1, -t); Rotate by m degrees as PIL.Image.rotate: angle = m mod 360, r = -radians(angle), the matrix
 * [cos r, sin r, 0, -sin r, cos r, 0] with every entry round(., 15), centre (W/2, H/2), a2 = (a0 (-cx) + a1 (-cy)) + cx
 * and a5 likewise with cy; angle 0 is the identity; 180 is (-1, 0, W, 0, -1, H); on square images 90 is
 * (0, -1, W, 1, 0, 0) and 270 is (0, 1, 0, -1, 0, H) (Pillow transposes in these cases: exact integer maps).
 *
 * Ops 6-9 (Brightness, Color, Contrast, Sharpness): out = blend(degenerate, image, f) per byte with a = the degenerate
 * byte and b = the image's: t = float(a) + f * float(b - a), one fp32 product and one fp32 sum; for 0 <= f <= 1 the
 * result is (uint8)(int)t, otherwise 0 for t <= 0, 255 for t >= 255, else (int)t.  The degenerate image: Brightness 0;
 * Color the grey (19595 R + 38470 G + 7471 B + 32768) >> 16 in all three channels (C = 1: the input is returned);
 * Contrast the constant floor(sum_grey / (H W) + 0.5) (C = 1: the grey is the channel itself); Sharpness Pillow's
 * SMOOTH: interior pixels floor(acc) clipped to 0..255, acc an fp32 that starts at 0.5 and adds float(p) * k_i over
 * the 3 x 3 window in row-major order, each step one product and one sum, k = (1, 1, 1, 1, 5, 1, 1, 1, 1) / 13 in fp32;
 * the one-pixel border is copied.
 *
 * Op 10 (Posterize): out = p & (0xFF << (8 - bits)), bits = iarg (the host: (8 - (arange(31) / (30 / 6))).round()).
 * Op 11 (Solarize): out = p if float(p) < farg else 255 - p (the host: farg = 255 * linspace(1, 0, 31)[bin]).
 * Op 12 (AutoContrast): per channel lo / hi = the minimum / maximum; hi <= lo: unchanged; otherwise
 *   lut[i] = clip(int(i * scale + offset), 0, 255) in fp64 with scale = 255.0 / (hi - lo), offset = -lo * scale.
 * Op 13 (Equalize): PIL.ImageOps.equalize per channel with the histogram h: fewer than two non-empty bins: unchanged;
 *   step = (sum(h) - last non-empty bin) div 255, step == 0: unchanged; otherwise n = step div 2 and for i = 0..255:
 *   lut[i] = min(n div step, 255); n += h[i].
 *
 * One workgroup per image, ONE launch per batch on `stream`; no allocation, no memset, no workspace, no wait for the
 * device.  B == 0 launches nothing; C outside {1, 3}, an empty image, C*H*W >= 2^30 or overlapping buffers return
 * BASD_EINVAL before anything is launched. */
int basd_trivial_augment(const unsigned char* src, unsigned char* dst, int B, int C, int H, int W,
                         const BasdTaugRecord* table, int* status, hipStream_t stream);

/* ---- Pillow-exact crops and resizes (bilinear, bicubic, box) of ragged uint8 images in one launch ------------ */

/* The horizontal pass of a band of output rows is staged in LDS as bytes: source rows x columns x C of one stage stay
 * inside this budget; a band whose rows need more is cut into shorter ones, a wide or strongly reduced image into
 * column chunks. */
#define BASD_RESIZE_STAGE_BYTES 40960
/* The largest reduction per axis: window size <= BASD_RESIZE_MAX_RATIO * resized size (at most 65 taps per pixel).
 * A filter of wider support admits less: ceil(S_f * in / out) <= BASD_RESIZE_MAX_RATIO, see the limits below. */
#define BASD_RESIZE_MAX_RATIO 32
/* Source and resized sides are at most this. */
#define BASD_RESIZE_MAX_SIDE 1048576

#define BASD_RESIZE_BAD_GEOMETRY 1   /* status bit 0: a window, rectangle, size or offset outside its bounds */
#define BASD_RESIZE_BAD_RATIO 2      /* status bit 1: a reduction above the filter's limit */
#define BASD_RESIZE_BAD_FILTER 4     /* status bit 2: a filter that is none of BASD_RESIZE_FILTER_* */

/* The resampling filter of a record: Pillow's Image.BILINEAR, Image.BICUBIC, Image.BOX. */
#define BASD_RESIZE_FILTER_BILINEAR 0
#define BASD_RESIZE_FILTER_BICUBIC 1
#define BASD_RESIZE_FILTER_BOX 2

/* One row of the device table, one per OUTPUT image (64 bytes).  Two records may name one source, with one filter or
 * with two. */
typedef struct BasdResizeRecord {
    long long src_offset;         /* byte offset of the source image in the packed buffer */
    int src_h, src_w;             /* the source: interleaved HWC, row pitch src_w * C bytes */
    int win_x, win_y, win_w, win_h;   /* the crop window inside the source */
    int res_w, res_h;             /* the size the window is resized to */
    int out_x, out_y;             /* top-left corner of the OH x OW output rectangle inside the resized image */
    int filter;                   /* BASD_RESIZE_FILTER_* (byte offset 48; 0, what a zeroed record holds: bilinear) */
    int pad[3];
} BasdResizeRecord;

/* replaces: `v2.RandomResizedCrop(image_size)` of the training transform and `v2.Resize(round(image_size / crop_ratio)),
 *           v2.CenterCrop(image_size)` of the clean and the validation transform  src/data/datasets.py:80-94,137-149,
 *           which the reference runs per image in Pillow inside its loader's workers (and twice per training image),
 *           with their `interpolation` argument (BILINEAR, the reference's default; BICUBIC; BOX) chosen per record.
 * src: one packed uint8 buffer of src_bytes bytes holding the decoded images (HWC, `np.asarray(img.convert("RGB"))`)
 * back to back at any byte address; dst: dense (n, C, OH, OW) uint8, planar, not overlapping src (checked);
 * table: n records on the device; status: one int on the device, OR-ed into (BASD_RESIZE_BAD_*).
 *   dst[i] = resize(window_i)[out_y : out_y + OH, out_x : out_x + OW]
 * This text is the specification; the kernel equals it byte for byte, and it equals Pillow 12's
 * `Image.crop((win_x, win_y, win_x + win_w, win_y + win_h)).resize((res_w, res_h), F)` byte for byte for F =
 * Image.BILINEAR, Image.BICUBIC, Image.BOX
 * (8-bit ImagingResample on the window as an image of its own: taps clamp at the window, not at the source).
 *
 * Per axis, with `in` the window size, `out` the resized size: scale = double(in) / out, fs = max(scale, 1.0),
 * support = S_f * fs with S_f = 1.0 (bilinear), 2.0 (bicubic), 0.5 (box), inv = 1.0 / fs.  For output index xx:
 * center = (xx + 0.5) * scale,
 *   xmin = max(int(center - support + 0.5), 0),  xmax = min(int(center + support + 0.5), in)     (int: towards zero),
 * for x = 0 .. xmax - xmin - 1 in increasing x: t = (x + xmin - center + 0.5) * inv, w_x = f(t) with
 *   bilinear: a = |t|, w_x = a < 1 ? 1 - a : 0;
 *   box:      -0.5 < t <= 0.5 ? 1 : 0  (of t itself, not of |t|: the asymmetry is Pillow's);
 *   bicubic:  a = -0.5, t = |t|:  t < 1: ((a + 2) * t - (a + 3)) * t * t + 1;  t < 2: (((t - 5) * t + 8) * t - 4) * a;
 *             otherwise 0  (evaluated in exactly this order);
 * ww = the running sum of the w_x; if ww != 0: w_x = w_x / ww;  k_x = int(0.5 + w_x * 2^22) for w_x >= 0 and
 * k_x = int(-0.5 + w_x * 2^22) for w_x < 0.  All of it fp64, from left to right, every operation rounded on its own
 * (no fused multiply-add).
 * A pass works on bytes: acc = 2^21 + sum_x k_x * p[xmin + x] in int32, result = clamp(acc >> 22, 0, 255) with an
 * arithmetic shift (bicubic's negative lobes take acc below 0 and above 255 << 22; sum |k_x| stays near 1.25 * 2^22,
 * so acc stays inside int32).  The horizontal pass runs first and is rounded to uint8; the vertical pass runs on those
 * bytes.  A pass with in == out is the identity under these formulas for all three filters (it is not special-cased).
 *
 * Limits, checked per record by the kernel (and by basd_amd.resize on the host): 1 <= src_h, src_w, res_h, res_w <=
 * BASD_RESIZE_MAX_SIDE; 0 <= src_offset and src_offset + src_h * src_w * C <= src_bytes; the window is not empty and
 * lies inside the source; the output rectangle lies inside the resized image (no padding: a centre crop of an image
 * smaller than the crop is refused); filter is one of BASD_RESIZE_FILTER_*; on both axes in <= BASD_RESIZE_MAX_RATIO *
 * out and ceil(S_f * max(in / out, 1)) <= BASD_RESIZE_MAX_RATIO, so that a pixel has at most 65 taps: reductions up to
 * 32 for bilinear and box, up to 16 for bicubic (a larger one is refused with BASD_RESIZE_BAD_RATIO, not resampled
 * another way).  A record that violates one gets an all-zero output image and its bit in the status word; nothing of
 * it is read.
 *
 * Grid: (bands of band_rows output rows) x records.  A workgroup makes the horizontal coefficients of its columns and
 * the vertical ones of its rows once, runs the horizontal pass for the source rows its rows' taps need into LDS, and
 * the vertical pass out of LDS, four output bytes of a row per lane and store.  The filter is a field of the record and
 * so uniform over a workgroup: records of different filters share a table and a launch.  band_rows: 0 = the entry point
 * chooses (32, halved down to 4 while the grid would have fewer than 1024 workgroups); 1..32 = a test / tuning hook (the
 * result does not depend on it).  ONE launch on `stream`; no allocation, no memset, no workspace, no wait for the device.
 * n == 0 launches nothing; C outside {1, 3}, OH or OW outside 1..BASD_RESIZE_MAX_SIDE, C*OH*OW >= 2^30, src_bytes < 0,
 * band_rows outside 0..32, more than 2^31 - 1 workgroups or overlapping buffers return BASD_EINVAL before anything is
 * launched.  The per-axis code (taps, tap count, record check) is csrc/resize_core.h, shared with a host program. */
int basd_resize_crop(const unsigned char* src, long src_bytes, unsigned char* dst, int n, int C, int OH, int OW,
                     const BasdResizeRecord* table, int* status, int band_rows, hipStream_t stream);

/* ---- Pillow-exact baseline JPEG decoding of a batch of streams in three launches --------------------------- */

/* Width and height of a stream the device decodes are at most this (larger ones go through the host fallback). */
#define BASD_JPEG_MAX_SIDE 16384
/* Images of one call (the image is the second grid axis of two of the launches). */
#define BASD_JPEG_MAX_BATCH 65535

#define BASD_JPEG_KIND_STREAM 0      /* a baseline JPEG stream, decoded on the device */
#define BASD_JPEG_KIND_RAW 1         /* width * height * 3 RGB bytes made by the host fallback, copied into place */
#define BASD_JPEG_KIND_PROGRESSIVE 2 /* a progressive JPEG stream: basd_jpeg_decode_progressive only (BAD_RECORD elsewhere) */

/* The per-image status word (0: decoded); the batch's status word is the OR of 1 << (code - 1). */
#define BASD_JPEG_BAD_RECORD 1       /* a field of the record outside its bounds (nothing of the image is read) */
#define BASD_JPEG_BAD_TABLE 2        /* a Huffman table that is not a prefix code, or reaches past the stream */
#define BASD_JPEG_TRUNCATED 3        /* the entropy-coded data of a segment ends before its last coefficient */
#define BASD_JPEG_BAD_CODE 4         /* a bit pattern that is no code of the table */
#define BASD_JPEG_BAD_RESTART 5      /* a missing or wrong RSTn marker, or a segment count that is not the frame's */
#define BASD_JPEG_BAD_INDEX 6        /* a coefficient index past 63 */
#define BASD_JPEG_BAD_VALUE 7        /* a DC value outside 16 bits */

/* One row of the device table, one per image (128 bytes).  Offsets into the stream are counted from src_offset. */
typedef struct BasdJpegRecord {
    long long src_offset;         /* byte offset of the stream (or of the raw pixels) in the byte buffer */
    long long out_offset;         /* byte offset of the image (HWC RGB, width * height * 3 bytes) in the output */
    long long coef_offset;        /* workspace: blocks (scan order) of 64 int16 in zigzag order (a multiple of 16) */
    long long plane_offset;       /* workspace: the component planes, blocks * 64 bytes (a multiple of 8) */
    long long seg_offset;         /* byte buffer: n_seg int32, the first entropy-coded byte of every segment */
    int src_len;                  /* bytes of the stream (< 2^31 - 16); of a raw record width * height * 3 */
    int kind;                     /* BASD_JPEG_KIND_* */
    int width, height;
    int ncomp;                    /* 1 or 3 */
    int hs, vs;                   /* sampling of component 0: (1,1), (2,1) or (2,2); the others are (1,1) */
    int restart;                  /* MCUs per restart interval (DRI), 0: none */
    int n_seg;                    /* entropy-coded segments: 1, or ceil(MCUs / restart) */
    int quant[3];                 /* per component: offset of the 64 bytes of its DQT table (zigzag order) */
    int dc[3], ac[3];             /* per component: offset of its DHT table (16 counts, then the values) */
    int n_scans;                  /* BASD_JPEG_KIND_PROGRESSIVE: scans, 1 .. BASD_JPEG_MAX_SCANS; else unused */
    int scan_offset;              /* ... the n_scans BasdJpegScan rows, counted from src_offset (8-byte aligned in the buffer) */
    int scan_segments;            /* ... the largest n_seg of a scan (the host's summary; the rows are what is checked) */
    int pad;
} BasdJpegRecord;

/* Bytes at the start of the workspace that hold the B per-image status words. */
long basd_jpeg_status_bytes(int B);

/* replaces: the `Image.open(...).convert("RGB")` of the reference loader's workers (src/data/datasets.py), the last
 *           per-image work of the host.
 * src: one uint8 buffer of src_bytes bytes (a multiple of 16, at a 16-byte aligned address) that holds the streams, the
 * raw pixels of the fallback's images and the int32 segment tables; out: out_bytes bytes, the images back to back as
 * interleaved HWC RGB (the layout of a RaggedBatch of 3 channels); table: B records on the device; ws: a workspace of
 * ws_bytes bytes (16-byte aligned) whose first basd_jpeg_status_bytes(B) bytes receive the per-image status words;
 * status: one int on the device, OR-ed into; max_blocks / max_pixels: the largest block and pixel count of an image
 * of the batch (they size the grids; an image with more is cut short, never written out of bounds).
 *
 * This text is the specification; basd_amd.jpeg.decode_reference restates it in numpy, the kernels equal it byte for
 * byte, and it equals Pillow 12 (libjpeg-turbo) `np.asarray(Image.open(f).convert("RGB"))` byte for byte on the
 * streams in scope: SOF0, 8 bits, 1 or 3 components, luma sampling (1,1), (2,1) or (2,2) with chroma (1,1) (one
 * component: any sampling, read as (1,1)), 8-bit quantisation tables, one interleaved scan, no Adobe APP14 segment,
 * three components only as YCbCr (a JFIF APP0 segment or the component ids 1, 2, 3), sides up to BASD_JPEG_MAX_SIDE.
 * The host parses the header (basd_amd.jpeg.parse_jpeg) and names the tables by their offsets; EXIF is ignored.
 *
 * Geometry.  hmax = hs, vmax = vs.  An MCU is hs * vs luma blocks (row-major) followed by one Cb and one Cr block and
 * covers 8 hs x 8 vs pixels; one component: one block, 8 x 8 pixels.  MCUs run row-major over ceil(W / (8 hs)) x
 * ceil(H / (8 vs)).  Component planes have ceil(W h / hmax) x ceil(H v / vmax) real samples (the rest of the blocks'
 * area is decoded and never shown).
 *
 * Entropy decode.  A Huffman table assigns canonical codes: code = 0; for each length l = 1..16 the next counts[l]
 * values get consecutive codes, then code <<= 1.  Bits are read MSB first; a byte FF followed by 00 is the data byte
 * FF, FF followed by anything else ends the segment's data.  Per block: the DC symbol s from the component's DC
 * table, diff = EXTEND(s bits), the component's predictor += diff is coefficient 0; then k = 1 and until k = 64: the AC
 * symbol rs, r = rs >> 4, s = rs & 15; s != 0: k += r, coefficient k = EXTEND(s bits), k += 1; s == 0 and r == 15:
 * k += 16; s == 0 otherwise: the block ends.  EXTEND(v of s bits) = v < 2^(s-1) ? v - 2^s + 1 : v.  Coefficient k sits
 * at zigzag position k and is multiplied by byte k of the component's table.  With DRI, every `restart` MCUs a new
 * segment begins: the rest of the byte is dropped, the marker RSTn (FF D0+n, n counting the markers modulo 8) is
 * expected, and the predictors return to 0.  A segment is decoded by one lane from its first byte (the host finds the
 * markers); it ends at the two bytes of the next segment's marker, the last one at the stream's end.
 *
 * IDCT: libjpeg's accurate integer one (CONST_BITS 13, PASS1_BITS 2) in 64-bit integers.  On 8 values c0..c7:
 *   z1 = (c2 + c6) * 4433, t2 = z1 - c6 * 15137, t3 = z1 + c2 * 6270, t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13,
 *   t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
 *   a0 = c7, a1 = c5, a2 = c3, a3 = c1; z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3, z5 = (z3 + z4) * 9633;
 *   a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299, z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5,
 *   z4 = z4 * -3196 + z5; a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
 *   outputs 0..7 = t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3.
 * Columns first, each output (x + 2^10) >> 11 kept as int32; then rows, (x + 2^17) >> 18; add 128, clamp to 0..255.
 *
 * Upsampling of Cb and Cr to the luma grid, with n the real width of the chroma plane.  n <= 2, or sampling (1,1):
 * replication, out(x, y) = s(x / hs, y / vs).  (2,1), n > 2 ("fancy"): out[2i] = (3 s[i] + s[i-1] + 1) >> 2,
 * out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2, out[0] = s[0], out[2n-1] = s[n-1].  (2,2), n > 2: for output row y the
 * chroma row r = y / 2 and its neighbour r - 1 (y even) or r + 1 (y odd), kept inside the real rows; cs = 3 * row r
 * + the neighbour; out[2i] = (3 cs[i] + cs[i-1] + 8) >> 4, out[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4,
 * out[0] = (4 cs[0] + 8) >> 4, out[2n-1] = (4 cs[n-1] + 7) >> 4.  The result is cropped to W x H.
 *
 * Colour.  One component: R = G = B = Y.  Three: F(x) = int(x * 65536 + 0.5), cb -= 128, cr -= 128,
 *   R = Y + ((F(1.402) cr + 32768) >> 16), B = Y + ((F(1.772) cb + 32768) >> 16),
 *   G = Y + ((-F(0.34414) cb + 32768 - F(0.71414) cr) >> 16), arithmetic shifts, each clamped to 0..255.
 *
 * Bad streams.  Every field of a record is checked against the byte buffer, the output and the workspace before it is
 * used; every read of a stream against the stream's (segment's) end; every write lands inside the image's own
 * regions.  An image that fails (BASD_JPEG_BAD_* above) has an all-zero output (nothing is written for it where its
 * output range itself is out of bounds), its code in its status word and the code's bit in `status`; the other images
 * are unaffected.
 *
 * Launches (THREE per batch, whatever B; no allocation, no memset, no wait for the device):
 *   entropy   one workgroup of 64 lanes per image: lanes 0 .. 2 ncomp - 1 build the look-ahead tables (9 bits) of the
 *             components' DHT tables in LDS, then lane l decodes segments l, l + 64, ...; a block is assembled in LDS
 *             and stored as 64 int16 in the stream's zigzag order;
 *   idct      one lane per block: dequantise, IDCT, 8 rows of 8 bytes into the block's place in its component plane;
 *   pixels    one lane per output pixel: upsampling taps, colour conversion, crop, 3 bytes; a raw record's pixels
 *             are copied, a failed image's are zero.
 * B == 0 launches nothing; B > BASD_JPEG_MAX_BATCH, misaligned or overlapping buffers, a workspace shorter than
 * basd_jpeg_status_bytes(B) or negative counts return BASD_EINVAL before anything is launched. */
int basd_jpeg_decode(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                     const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status, long max_blocks,
                     long max_pixels, hipStream_t stream);

/* The same decode with the entropy stage working INSIDE a segment in parallel (opt-in; basd_jpeg_decode above is the
 * default and stays as it is).  Arguments, checks, workspace layout, record, status words and output bytes are those
 * of basd_jpeg_decode: for every stream, intact or damaged, both give the same per-image status word and the same
 * bytes (that is the contract; what holds the code to it is listed in DESIGN.md section 8).  Still three launches: a different entropy kernel, then the same idct and pixels kernels.
 *
 * sub_bytes: 0 (the built-in default, 128) or a multiple of 8 in BASD_JPEG_SUB_BYTES_MIN .. BASD_JPEG_SUB_BYTES_MAX;
 * anything else returns BASD_EINVAL.
 *
 * Scheme.  One workgroup of 256 lanes per image.  An image of 64 segments or more is decoded a segment per lane as
 * above.  Otherwise its segments are taken one after the other by the whole workgroup: the segment's coefficient area
 * is zeroed, its bytes are cut into sub-sequences of sub_bytes, and these are worked through in chunks of 256 (one per
 * lane); the exact decoder state, the number of blocks begun and the three DC predictors are carried from chunk to
 * chunk.  In a chunk, (1) lane 0 decodes its sub-sequence from the carried state and every other lane from a guess (a
 * block of component slot 0 begins at the sub-sequence's first byte), up to the first symbol that begins at or behind
 * the sub-sequence's end, and keeps its exit state, the number of blocks that began and the sums of the DC differences
 * per component; a bad code, an index past 63 or the end of the data is no error here, it leaves "no state".  (2) In
 * rounds, each behind a barrier, a lane whose predecessor's exit state differs from the state it last entered with
 * decodes again from it (from its own guess where the predecessor left no state); the rounds end when no lane decoded.
 * After round n the first n + 1 sub-sequences are exact whatever the stream.  Huffman streams usually fall into step
 * a few symbols to a kilobyte behind a wrong start and a chunk then takes a few rounds, but a periodic stream (a flat
 * picture) can hold a wrong phase, and blocks without an end-of-block code hide the zigzag index, for ever.  So there
 * are at most 64 such rounds; a chunk that has not settled by then is finished by one lane, which walks once through
 * the sub-sequences behind the 65 exact ones while the other lanes wait.  A chunk thus takes AT MOST 66 rounds (the
 * first pass, 64 rounds, the walk), its time stays within that of 256 passes over a sub-sequence, and termination does
 * not rest on the stream.  (3) An exclusive prefix sum over the block counts and the DC sums, added to the carried
 * ones, gives every lane its first block and its predictors.  (4) Every lane decodes once more from its now exact state
 * and stores its coefficients one by one (a block that spans sub-sequences is filled by several lanes); no block at or
 * past the segment's block count is begun, so padding is never decoded.  The segment is done when its last block has
 * ENDED, not when it has begun: the handed-over state says so (more blocks begun than the segment has; or as many, and
 * the zigzag index 0 or no state); a last block that begins in a chunk's last sub-sequence and runs on is finished,
 * and an error in its rest is met, by the next chunk.  The last sub-sequence of a segment has no end
 * and runs to the block count or to the error the serial decoder meets.  Of several lanes that fail the first in
 * stream order gives the segment's code; an image's status is the largest of its segments' codes, as above.
 * The exit state is canonical: it names the first byte of the stream of which no bit was taken (a stuffed 00 counts to
 * its FF), the unread bits of the byte ahead of it, the block's slot in the MCU and the zigzag index, so two decoders
 * at the same bit hand over equal states whatever their refills were. */
#define BASD_JPEG_SUB_BYTES_MIN 8
#define BASD_JPEG_SUB_BYTES_MAX 1024
int basd_jpeg_decode_parallel(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                              const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status,
                              long max_blocks, long max_pixels, int sub_bytes, hipStream_t stream);

/* ---- progressive JPEG streams in the same batch (opt-in): one more launch ------------------------------------- */

#define BASD_JPEG_MAX_SCANS 64       /* scans of a progressive stream the device takes (more: the host fallback) */

/* One row of a progressive record's scan table (64 bytes; the table sits in the byte buffer at src_offset +
 * scan_offset).  Offsets are counted from src_offset. */
typedef struct BasdJpegScan {
    int seg_offset;               /* n_seg int32 (4-byte aligned in the buffer): the first entropy-coded byte of every segment */
    int n_seg;                    /* 1, or ceil(scan units / restart) */
    int data_end;                 /* where the scan's data ends: the marker behind it, or src_len */
    int restart;                  /* scan units per restart interval in force at this SOS, 0: none */
    int ncomp;                    /* 1 (a one-component scan), or the frame's (an interleaved DC scan) */
    int comp;                     /* the frame index of a one-component scan's component */
    int ss, se, ah, al;           /* the band and the successive approximation: ss = se = 0 or 1 <= ss <= se <= 63; al <= 13 */
    int level;                    /* 0, or 1 + the largest level of an earlier scan that shares a component and overlaps
                                     in ss .. se; below n_scans */
    int dc[3];                    /* DC first scans: per FRAME component of the scan the offset of its DHT table */
    int ac;                       /* AC scans: the offset of the DHT table */
    int pad;
} BasdJpegScan;

/* Decodes a batch that may hold records of kind BASD_JPEG_KIND_PROGRESSIVE next to baseline and raw ones.  Arguments,
 * checks, workspace layout (192 bytes per block of the MCU-padded frame), status words and BASD_EINVAL rules are those
 * of basd_jpeg_decode_parallel; `parallel` picks the baseline entropy stage (0: that of basd_jpeg_decode, 1: that of
 * basd_jpeg_decode_parallel with `sub_bytes`; sub_bytes must be 0 with parallel == 0); max_scans / max_segments: the
 * largest scan count of a progressive record and the largest segment count of a scan of the batch (0 .. BASD_JPEG_MAX_SCANS
 * and >= 0; a record or a scan that claims more is BASD_JPEG_BAD_RECORD).
 *
 * Scope: SOF2, Huffman coding, and everything else of the frame as above (8 bits, 1 or 3 components, the same sampling,
 * 8-bit DQT tables all ahead of the first SOS, no Adobe segment, the JFIF / component-id rule, no DNL); at most
 * BASD_JPEG_MAX_SCANS scans with only DHT, DRI, COM and APPn segments between them; a DC scan (ss = se = 0) of all
 * components in frame order or of one, an AC scan (1 <= ss <= se <= 63) of one, behind that component's first DC
 * scan; al <= 13; the first scan of a coefficient has ah = 0, every later one ah = the previous al and al = ah - 1;
 * and the progression is COMPLETE: at EOI every coefficient of every component has been coded down to al = 0 (libjpeg
 * smooths the blocks of an incomplete one, which this text does not describe).  The host decides all of this
 * (basd_amd.jpeg.parse_jpeg(data, progressive=True)) and sends every other file through the fallback.
 *
 * Specification.  Coefficients are int16, zero before the first scan; what is stored wraps to 16 bits.
 * Geometry: an interleaved scan walks the frame's MCUs as the baseline scan does.  A one-component scan walks that
 * component's own blocks in raster order over ceil(cw / 8) x ceil(ch / 8), cw = ceil(W h / hmax), ch = ceil(H v / vmax):
 * NOT the MCU-padded grid (a 17 x 33 4:2:0 file: 3 x 5 luma blocks, not 4 x 6).  A scan unit is an MCU or such a block.
 * Restart segments: with DRI in force at the scan's SOS a segment is `restart` scan units, RSTn as above; at a segment's
 * start the DC predictors and EOBRUN are 0.  Tables are the ones in force at the SOS.
 * DC first (ss = 0, ah = 0): the DC symbol s, pred += EXTEND(s bits), coefficient 0 = pred << al.
 * DC refinement (ss = 0, ah > 0): one bit; if it is 1, coefficient 0 |= 1 << al.
 * AC first (ah = 0): if EOBRUN > 0: EOBRUN -= 1, the block is done.  Else k = ss; while k <= se: the AC symbol rs,
 *   r = rs >> 4, s = rs & 15; s != 0: k += r, coefficient k = EXTEND(s bits) * 2^al, k += 1; s == 0 and r == 15:
 *   k += 16; otherwise EOBRUN = 2^r - 1, plus r more bits where r > 0, and the block is done.
 * AC refinement (ah > 0), p1 = 1 << al, m1 = -1 << al; "correct k": read one bit; if it is 1 and (coefficient k & p1)
 *   == 0, add p1 where the coefficient is >= 0, else m1.  k = ss.  If EOBRUN == 0, while k <= se: read rs; s != 0: s
 *   must be 1, one bit, the new value is p1 if it is 1, else m1; s == 0 and r != 15: EOBRUN = 2^r, plus r bits where
 *   r > 0, leave the loop; then walk: while k <= se: coefficient k non-zero: correct k; zero: r -= 1, stop the walk
 *   where r < 0; k += 1.  Behind the walk a new value is stored at k; k += 1.  Then, if EOBRUN > 0: every non-zero
 *   coefficient from k to se is corrected, EOBRUN -= 1.
 * Dequantisation, IDCT, upsampling and colour are the text above, unchanged.
 * Errors: a value to be stored at k > se is BASD_JPEG_BAD_INDEX; a refinement symbol with s > 1 BASD_JPEG_BAD_CODE; a
 * DC category above 15 or a DC predictor outside 16 bits BASD_JPEG_BAD_VALUE; a scan's segment count that is not its
 * grid's BASD_JPEG_BAD_RESTART; the codes above otherwise.  An image's status is the code of the FIRST SCAN IN STREAM
 * ORDER that has a failing segment, and where several segments of that scan fail the largest of their codes (every
 * segment of a scan that runs is decoded); scans behind it do not matter.  A failed image's output is all zero.
 *
 * Launches (FOUR, whatever B; no allocation, no memset, no wait):
 *   progressive  one workgroup of 512 lanes per image, which returns at once for the other kinds.  The record and EVERY
 *                scan row are checked against the buffers before anything they name is read; the coefficient area is
 *                zeroed; then the scans run by levels with a barrier between levels: scans of one level touch disjoint
 *                coefficients, the n-th of them goes to wave n mod 8 (scans of different kinds diverge, so they do not
 *                share a wave), and within a scan lane l of the wave decodes segments l, l + 64, ...  Coefficients are
 *                read and written in place, at the block's position in the INTERLEAVED order, which is what idct reads.
 *                Once a segment of scan j has failed, no scan behind j is begun; scans ahead of j still run.
 *   entropy      the chosen baseline stage; it passes over progressive records and leaves their status words alone;
 *   idct, pixels as above; they take a progressive record as they take a stream. */
int basd_jpeg_decode_progressive(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                                 const BasdJpegRecord* table, unsigned char* ws, long ws_bytes, int* status,
                                 long max_blocks, long max_pixels, int sub_bytes, int parallel, int max_scans,
                                 int max_segments, hipStream_t stream);

/* ---- Pillow-exact 8-bit PNG decoding of a batch of files in two launches ------------------------------------ */

#define BASD_PNG_MAX_SIDE 16384
#define BASD_PNG_MAX_BATCH 65535

#define BASD_PNG_KIND_STREAM 0       /* the IDAT payloads of a PNG file, inflated and unfiltered on the device */
#define BASD_PNG_KIND_RAW 1          /* width * height * 3 RGB bytes made by the host fallback, copied into place */

/* The per-image status word (0: decoded); the batch's status word is the OR of 1 << (code - 1). */
#define BASD_PNG_BAD_RECORD 1        /* a field of the record outside its bounds (nothing of the image is read) */
#define BASD_PNG_BAD_BLOCK 2         /* deflate block type 3 */
#define BASD_PNG_BAD_STORED 3        /* a stored block whose LEN is not ~NLEN */
#define BASD_PNG_BAD_LENGTHS 4       /* code lengths that are no prefix code (see below) */
#define BASD_PNG_BAD_CODE 5          /* a bit pattern or a symbol that is no code (see below) */
#define BASD_PNG_BAD_DISTANCE 6      /* a match that reaches back past the first byte produced */
#define BASD_PNG_TRUNCATED 7         /* the input ends before the final block, or before the 4 bytes behind it, do */
#define BASD_PNG_WRONG_LENGTH 8      /* the stream produces more or fewer bytes than the scanlines need */
#define BASD_PNG_BAD_FILTER 9        /* a scanline whose filter type is above 4 */
#define BASD_PNG_BAD_ADLER 10        /* the Adler-32 of the inflated bytes is not the one behind the final block */

/* One row of the device table, one per image (64 bytes). */
typedef struct BasdPngRecord {
    long long src_offset;         /* byte buffer: the concatenated IDAT payloads, zlib header first (or the raw pixels) */
    long long out_offset;         /* byte offset of the image (HWC RGB, width * height * 3 bytes) in the output */
    long long ws_offset;          /* workspace: the filtered scanlines, height * (width * bpp + 1) bytes (a multiple of 16) */
    long long plte_offset;        /* byte buffer: 768 bytes, PLTE padded with zeros (read for colour type 3 only) */
    int src_len;                  /* bytes at src_offset (< 2^31 - 16); of a raw record width * height * 3 */
    int kind;                     /* BASD_PNG_KIND_* */
    int width, height;
    int color_type;               /* 0, 2, 3, 4 or 6 */
    int pad[3];
} BasdPngRecord;

/* Bytes at the start of the workspace that the launches keep per batch: B int32 status words, then B int32 with the
 * offset (from src_offset) of the 4 Adler-32 bytes, i.e. of the first byte boundary behind the final block. */
long basd_png_status_bytes(int B);

/* replaces: the same `Image.open(...).convert("RGB")` of the reference loader's workers for the datasets that ship PNG
 *           files (configs/experiment/basd_cifar100.yaml: uoft-cs/cifar100).
 * The arguments are those of basd_jpeg_decode, with max_filtered the largest height * (width * bpp + 1) of a stream
 * record.  This text is the specification; basd_amd.png.inflate_reference / decode_reference restate it in Python, the
 * kernels equal them byte for byte and status for status, and they equal Pillow 12
 * `np.asarray(Image.open(f).convert("RGB"))` on the files in scope.
 *
 * Scope (the host's basd_amd.png.parse_png decides; everything else is a raw record made by the fallback): bit depth 8,
 * colour type 0 (gray), 2 (RGB), 3 (palette, PLTE present), 4 (gray + alpha) or 6 (RGBA), no interlace, compression and
 * filter method 0, sides 1 .. BASD_PNG_MAX_SIDE, a zlib header that says deflate, a window of at most 32 KiB, no preset
 * dictionary and passes its check (CMF * 256 + FLG divisible by 31).  Chunk CRCs are not checked (Pillow decodes a file
 * whose IDAT CRC is wrong); tRNS, gAMA, iCCP, bKGD, acTL and every other ancillary chunk are ignored.
 *
 * Output: bpp = 1, 3, 1, 2, 4 bytes per pixel for colour types 0, 2, 3, 4, 6.  Gray is written three times, alpha is
 * dropped (not composited), index i is bytes 3 i .. 3 i + 2 of the 768 palette bytes (entries past PLTE are 0, 0, 0).
 *
 * Inflate (RFC 1951) of src[2 .. src_len) -- the two header bytes are the host's -- into exactly
 * n = height * (width * bpp + 1) bytes.  Bits are taken from the least significant end of each byte; past the end of
 * the input the bits are zeros, and taking one of them is BASD_PNG_TRUNCATED, which is checked after every group of
 * bits taken and before what they say is looked at.  Per block: 1 bit final, 2 bits type.
 *   type 3: BASD_PNG_BAD_BLOCK.
 *   type 0: the rest of the byte is dropped; LEN, NLEN (16 bits each); LEN != ~NLEN: BASD_PNG_BAD_STORED; more than
 *           n bytes produced: BASD_PNG_WRONG_LENGTH; fewer than LEN bytes left: BASD_PNG_TRUNCATED; LEN bytes copied.
 *   type 1: literal/length lengths 8 (0..143), 9 (144..255), 7 (256..279), 8 (280..287); 32 distance lengths of 5.
 *   type 2: HLIT (5), HDIST (5), HCLEN (4); HLIT + 257 > 286 or HDIST + 1 > 30: BASD_PNG_BAD_LENGTHS; HCLEN + 4
 *           lengths of 3 bits in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15; then HLIT + 257 + HDIST + 1
 *           lengths by that code: 0..15 a length; 16: the previous length 3 + (2 bits) times (none before it:
 *           BASD_PNG_BAD_LENGTHS); 17: zero 3 + (3 bits) times; 18: zero 11 + (7 bits) times; a repeat that runs
 *           past the count, or no length for symbol 256: BASD_PNG_BAD_LENGTHS.
 * A set of lengths is a code when it is not over-subscribed (sum of 2^-len <= 1) and complete (= 1); as in zlib, the
 * literal/length and the distance set may also be incomplete when their longest code has 1 bit or they have no code at
 * all; the code-length set may not.  Anything else is BASD_PNG_BAD_LENGTHS.  Codes are canonical (per length in
 * symbol order, counting up, shorter lengths first), and are sent most significant bit first.  A symbol is found from
 * the next 15 bits; where they begin with no code, 15 bits are taken and the result is BASD_PNG_BAD_CODE.  Symbols of
 * a block, one at a time: < 256 a literal; 256 ends the block; 286, 287: BASD_PNG_BAD_CODE; else with i = symbol - 257:
 * length 3 + i (i < 8), 258 (i = 28), else e = i / 4 - 1 extra bits and length 3 + ((4 + i % 4) << e) + extra; then a
 * distance symbol d (30, 31: BASD_PNG_BAD_CODE): distance 1 + d (d < 4), else e = d / 2 - 1 extra bits and distance
 * 1 + ((2 + d % 2) << e) + extra.  A distance larger than the count of bytes produced: BASD_PNG_BAD_DISTANCE.  A
 * literal or a match that would produce byte n + 1: BASD_PNG_WRONG_LENGTH (checked after the distance).  Byte
 * pos + j of a match is byte pos - distance + j % distance.  After the final block: fewer than n bytes:
 * BASD_PNG_WRONG_LENGTH; the rest of the byte is dropped; fewer than 4 bytes left: BASD_PNG_TRUNCATED.  What follows
 * those 4 bytes is ignored.
 *
 * Adler-32 of the n bytes b_0 .. b_(n-1): A = (1 + sum b_i) mod 65521, B = (n + sum (n - i) b_i) mod 65521; the 4
 * bytes behind the final block, big-endian, must equal B * 65536 + A (else BASD_PNG_BAD_ADLER); then every scanline's
 * first byte must be at most 4 (else BASD_PNG_BAD_FILTER).
 *
 * Unfilter (PNG 1.2, section 6): per scanline the filter byte, then width * bpp bytes x; with a the reconstructed
 * byte bpp to the left, b the one above, c the one above a (0 outside the image), modulo 256: 0: x; 1: x + a; 2: x + b;
 * 3: x + floor((a + b) / 2); 4: x + Paeth, where p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c| and the
 * predictor is a if pa <= pb and pa <= pc, else b if pb <= pc, else c.
 *
 * Bad streams.  Every field of a record is checked against the byte buffer, the output and the workspace before it is
 * used, every read of a stream against src_len, every write lands in the image's own ranges.  An image that fails has
 * an all-zero output (nothing is written where its output range itself is out of bounds), its code in its status word
 * and the code's bit in `status`; the other images are unaffected.  Every loop of the inflate takes at least one bit or
 * produces at least one byte, and leaves at the first error, so a stream ends within 8 * src_len + n steps.
 *
 * Launches (TWO per batch, whatever B; no allocation, no memset, no wait for the device):
 *   inflate    one workgroup of one wave per image.  The decode state is the same in all 64 lanes.  The three Huffman
 *              tables live in LDS: lane 0 counts the lengths and assigns the codes, all lanes fill the 9-bit look-up
 *              (longer codes are found by counting through the lengths).  A match is copied by the lanes together
 *              out of a 32 KiB window of the output kept in LDS; every byte goes to the window and to the workspace.
 *   unfilter   one workgroup of one wave per image: the Adler-32 and the filter bytes (lanes stride over the bytes,
 *              64-bit sums), then bands of 64 scanlines as a skewed wavefront: lane l owns row r0 + l and
 *              reconstructs pixel t - l at step t, the pixel above comes from lane l - 1 by a lane shift, the last
 *              row of a band is written back for the next one; each pixel is written as RGB in the same step.  A
 *              raw record's pixels are copied, a failed image's are zero.
 * B == 0 launches nothing; the argument checks and BASD_EINVAL rules are those of basd_jpeg_decode (max_filtered and
 * max_pixels at most what BASD_PNG_MAX_SIDE allows, a workspace of at least basd_png_status_bytes(B)). */
int basd_png_decode(const unsigned char* src, long src_bytes, unsigned char* out, long out_bytes, int B,
                    const BasdPngRecord* records, unsigned char* ws, long ws_bytes, int* status, long max_filtered,
                    long max_pixels, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BASD_HIP_H */
