/* driftmi.h — C ABI of libdriftmi, the MI355X (gfx950) implementation of
 * driftscan's per-m hot path (beam-transfer generation, SVD compression,
 * KL / DoubleKL).  This is the drop-in boundary: plain pointers and sizes, no
 * torch / numpy types, `extern "C"`.  The reference has no FFI of its own (it is
 * Python + LAPACK); each entry point therefore cites the reference *call site*
 * whose arithmetic it replaces (paths relative to radiocosmology/driftscan).
 *
 * Conventions
 *   - complex128 = interleaved (double re, double im); matrices are row-major.
 *   - every pointer named *_dev is DEVICE memory owned by the caller (e.g. a
 *     torch tensor's data_ptr()); pointers named *_host are host memory.
 *   - every function returns int: 0 ok, <0 argument/runtime error (see
 *     dm_last_error), >0 numerical status mirroring LAPACK `info`.  0 is the ONLY
 *     success value: no entry point reports a count or a warning through its
 *     return value (the Python binding raises on every non-zero status, positive
 *     ones included — products behind a failed eigen-iteration are not usable).
 *   - a dm_ctx owns a device id, a HIP stream and a growable device workspace;
 *     one context per GPU, one host thread per context.  All work is enqueued on
 *     the context's stream; functions documented as "synchronises" block the
 *     host until their results are complete.
 *   - there is NO CPU fallback: without a GPU every compute entry point fails.
 */
#ifndef DRIFTMI_H
#define DRIFTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dm_ctx dm_ctx;

/* ---- context ----------------------------------------------------------- */
/* stream: an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)
 * or NULL to let the context create its own. */
int dm_ctx_create(int device, size_t workspace_bytes, void* stream, dm_ctx** out);
int dm_ctx_destroy(dm_ctx* ctx);
int dm_ctx_sync(dm_ctx* ctx);
size_t dm_ctx_workspace_bytes(dm_ctx* ctx);
/* Replace the (idle) workspace arena by one of exactly `bytes` (0: just give the memory back).  The arena
 * only ever grows on its own; a stage that needs most of the card in one piece (dm_eigh_gen at n = 32 576:
 * ~140 GB) calls this first so that the previous stage's arena is not in the way.  Synchronises.
 * No reference counterpart (numpy allocates per call). */
int dm_ctx_workspace_reset(dm_ctx* ctx, size_t bytes);
const char* dm_last_error(dm_ctx* ctx);
int dm_version(void);

/* dm_prof_trd_stride: the live measurement samples — every dm_prof_trd_stride()-th column of the tridiagonalisation
 * is bracketed by events, every launch of >= 2e9 work units of the other classes, and one in four of the smaller
 * ones; dm_prof_report weights the samples (by the stride / by four), so its figures estimate the totals over all
 * launches and `launches` the number of launches.  Event records cost a marker packet each. */
int dm_prof_trd_stride(void);

/* Per-kernel-class instrumentation for bench.py: when enabled (1) every launch of the MFMA / HBM-bound kernel
 * classes is bracketed by HIP events on the context's stream (sampled as dm_prof_trd_stride describes); with
 * enable = 2 every remaining kernel of the path is bracketed as well (the "extended" classes, time only).
 * dm_prof_report fills 24-entry arrays with summed event time [ms], algorithmic flops actually executed and launch
 * counts since the last reset:
 *   0 grouped ZGEMM, 1 real-B GEMM, 2 Jacobi Gram, 3 Jacobi inner solver, 4 Jacobi apply, 5 real GEMM of the D&C merges,
 *   6 / 7 the one-stage tridiagonalisation kernels [algorithmic BYTES], 8 panel QR, 9 bulge chase, 10 second-stage
 *   back-transformation of the two-stage tridiagonalisation, 11 gathered-B ZGEMM (the covariance projections);
 *   extended: 12 fused ring transform of BT-gen, 13 other BT-gen kernels, 14 LDS-resident small tridiagonalisation,
 *   15 divide & conquer (without its real GEMMs), 16 Cholesky panels + triangular diagonal solves, 17 transposes /
 *   copies / scans, 18 T factors / slice sums / gathers of the eigensolver, 19 Jacobi-engine and SVD-chain helpers,
 *   20 block-apply of stored product blocks to vectors [algorithmic BYTES of A], 21-23 unused. */
int dm_prof_reset(dm_ctx* ctx, int enable);
int dm_prof_report(dm_ctx* ctx, double* ms, double* flops, long long* launches);

/* ---- dense building blocks (exposed for the parity tests) --------------- */
/* C = alpha * op(A) diag(kscale) op(B) + beta C on the fp64 matrix cores.
 * A is viewed as (M x K) through element strides (rsA, csA), B as (K x N)
 * through (rsB, csB); conj* conjugate the elements.  `batch` problems at the
 * given element strides between consecutive A/B/C/kscale.
 * Replaces: np.dot at drift/core/beamtransfer.py:1186, :1226; doublekl.py:73-85. */
int dm_zgemm_strided_batched(dm_ctx* ctx, int M, int N, int K, double alpha, const void* A_dev, int rsA, int csA,
                             int conjA, int64_t strideA, const void* B_dev, int rsB, int csB, int conjB,
                             int64_t strideB, double beta, void* C_dev, int ldc, int64_t strideC,
                             const double* kscale_dev, int64_t stride_kscale, int batch);

/* The same product for a ragged group: `nprob` independent problems of different shapes in ONE launch
 * (every 64x64 output tile of every problem is a workgroup).  Used where the reference loops over m or
 * frequency with one np.dot per iteration.
 * Replaces: np.dot at drift/core/doublekl.py:73-74, :80, :85; drift/core/kltransform.py:124-143 (inv_gen,
 * formed here as N E^H from E N E^H = I). */
typedef struct dm_zgemm_problem {
  const void* A;  /* device c128, viewed (M x K) through element strides (rsA, csA) */
  const void* B;  /* device c128, viewed (K x N) through (rsB, csB) */
  void* C;        /* device c128, row-major, leading dimension ldc */
  int M, N, K;
  int rsA, csA, rsB, csB, ldc;
  int conjA, conjB;
  double alpha, beta;
} dm_zgemm_problem;
int dm_zgemm_grouped(dm_ctx* ctx, int nprob, const dm_zgemm_problem* probs_host);

/* The grouped product with every field of its internal descriptor.  Exposed for the parity tests: the drivers of the
 * library (Cholesky and triangular solves, the tridiagonalisations, BT-gen, sky synthesis, the covariance
 * projections) fill these fields themselves; the two entries below let a test reach each kernel class and flag
 * directly.  C(m, n) lives at C[m ldc + n csc]:
 *   C = (alpha + i alpha_im) op(A) diag(kscale) op(B) + beta C
 * flags (DM_ZGEMM_*):
 *   CONJ_A, CONJ_B  conjugate the elements as they are read
 *   B_REAL          B holds doubles (strides in doubles)
 *   ALL_REAL        A, B and C hold doubles; takes no kscale, csc != 1, alpha_im, conj flag, B_REAL or B_GATHER
 *   B_GATHER        B(k, n) = B[bgather[2n] + k rsB] * kscale[bgather[2n + 1] + k]; needs bgather and kscale, csB is
 *                   not read; not together with B_REAL
 *   LOWER / UPPER   only the 64 x 64 tiles on or below / above the block diagonal are computed, the rest of C is
 *                   left alone; UPPER | UPPER128 also computes the tile left of an odd diagonal tile.  Complex B only.
 * A combination listed as not taken is refused with DM_EARG before anything is launched. */
enum {
  DM_ZGEMM_CONJ_A = 1,
  DM_ZGEMM_CONJ_B = 2,
  DM_ZGEMM_B_REAL = 4,
  DM_ZGEMM_LOWER = 8,
  DM_ZGEMM_ALL_REAL = 16,
  DM_ZGEMM_UPPER = 32,
  DM_ZGEMM_B_GATHER = 64,
  DM_ZGEMM_UPPER128 = 128
};
typedef struct dm_zgemm_problem_ex {
  const void* A;
  const void* B;
  void* C;
  const double* kscale; /* K weights (applied to A), the weight runs of a gathered B, or NULL */
  const int* bgather;   /* B_GATHER: N pairs (element offset of the column's K-run in B, offset of its weights) */
  int M, N, K;
  int rsA, csA, rsB, csB, ldc, csc;
  int flags;
  double alpha, alpha_im, beta;
  int launch; /* problems with the same value share one grouped launch */
} dm_zgemm_problem_ex;
/* The problems of each `launch` value form one plan; all plans are built first, their host images travel to the
 * device in ONE copy, and the launches run in ascending `launch` order on the context's stream (the route of the
 * Cholesky, solve and tridiagonalisation chains), so a later launch may read what an earlier one wrote.  M, N, K >= 0;
 * a problem with M = 0 or N = 0 writes nothing, K = 0 gives C = beta C.  Returns when the work is queued. */
int dm_zgemm_grouped_ex(dm_ctx* ctx, int nprob, const dm_zgemm_problem_ex* probs_host);

/* What the planner decides for the same list, per launch in ascending `launch` order (exposed for the parity tests,
 * which assert their coverage of the kernels from it).  Host only: no context, no device, and no pointer of a problem
 * is followed (only NULL or not).  Classes are 0 complex, 1 real B, 2 all real, 3 gathered B.
 * cells[class][flat][ragged][rmw] counts the tiles: flat = a 32-row tile of the register-only kernel, ragged = the
 * tile reaches past M or N or its operands are scaled (kscale, gathered B) — the masked path of the kernels —, rmw =
 * beta != 0.  *nlaunch gets the number of launches; at most max_launch entries of out are written.  DM_EARG for a
 * flag combination the planner refuses. */
typedef struct dm_zgemm_launch_info {
  int launch;
  int use4;   /* register-only kernels (0: the LDS-staged ones) */
  int deep;   /* complex class on the deep-prefetch kernel */
  int wide_r; /* real-B class on 64 x 128 tiles */
  int tiles[4];
  int flat[4];
  int cells[4][2][2][2];
} dm_zgemm_launch_info;
int dm_zgemm_plan_info(int nprob, const dm_zgemm_problem_ex* probs_host, int max_launch, dm_zgemm_launch_info* out,
                       int* nlaunch);

/* Batched lower Cholesky A = L L^H in place (n x n, row-major, ld), `batch`
 * matrices `stride` elements apart.  info_host[i] = 0 or the order of the first
 * non-positive-definite leading minor.  Synchronises.
 * Replaces: the zpotrf inside scipy.linalg.eigh(A, B) at drift/core/kltransform.py:89. */
int dm_zpotrf_batched(dm_ctx* ctx, int n, void* A_dev, int ld, int64_t stride, int batch, int* info_host);

/* Batched triangular solve with the lower factor: L X = B (conjtrans = 0) or
 * L^H X = B (conjtrans = 1), X overwrites B (n x nrhs row-major).
 * Replaces: zhegst / ztrsm inside scipy.linalg.eigh(A, B), kltransform.py:89. */
int dm_ztrsm_left_lower_batched(dm_ctx* ctx, int n, int nrhs, const void* L_dev, int ldl, int64_t strideL,
                                void* B_dev, int ldb, int64_t strideB, int conjtrans, int batch);

/* The same two engines for a ragged list of problems, as dm_eigh_gen hands them (exposed for the parity tests):
 * every problem has its own address, size and leading dimensions, and all of them share each launch.
 * Factorisation: only the lower triangle of A is read (of the diagonal its real part); on return the lower triangle
 * holds L with a real positive diagonal, the strictly upper triangle of the n x n window is zero, and nothing outside
 * that window is written.  info_host[i] = 0, or the 1-based index of the first pivot that is not a positive finite
 * number (a NaN or an Inf counts as a failure there); the window of a failed problem holds no usable factor, the
 * other problems of the launch are not affected.  Synchronises. */
typedef struct dm_zpotrf_problem {
  void* A; /* device c128, row-major n x n, leading dimension ld >= n */
  int n, ld;
} dm_zpotrf_problem;
int dm_zpotrf_problems(dm_ctx* ctx, int nprob, const dm_zpotrf_problem* probs_host, int* info_host);

/* Solves: L X = B (conjtrans = 0) or L^H X = B (conjtrans = 1), X overwrites the n x nrhs window of B; of L only the
 * lower triangle is read (of its diagonal the real part), and nothing outside the window of B is written.
 * upper_only (forward solves with nrhs == n only): X is wanted on and above its diagonal only; the entries below it
 * come back undefined (they stay inside the window).  Returns when the work is queued. */
typedef struct dm_ztrsm_problem {
  const void* L; /* device c128, row-major n x n, leading dimension ldl >= n */
  int ldl, n;
  void* B;       /* device c128, row-major n x nrhs, leading dimension ldb >= nrhs */
  int ldb, nrhs;
} dm_ztrsm_problem;
int dm_ztrsm_problems(dm_ctx* ctx, int nprob, const dm_ztrsm_problem* probs_host, int conjtrans, int upper_only);

/* The argument checks of the two entries above on their own.  Host only: no context, no device, and no pointer of a
 * problem is followed (only NULL or not).  DM_EARG for a negative size, ld < n or ldl < n where n > 0, ldb < nrhs where
 * nrhs > 0, a NULL matrix of a problem that is not empty (n > 0; for a solve n > 0 and nrhs > 0), upper_only together
 * with conjtrans, or upper_only with nrhs != n; DM_OK otherwise. */
int dm_zpotrf_problems_check(int nprob, const dm_zpotrf_problem* probs_host);
int dm_ztrsm_problems_check(int nprob, const dm_ztrsm_problem* probs_host, int conjtrans, int upper_only);

/* One-sided block-Jacobi SVD of `batch` row-major matrices (rows x cols, ld,
 * `stride` elements apart): the rows of each matrix are unitarily mixed in place
 * until mutually orthogonal with respect to the columns [gc0, gc1) and sorted by
 * descending norm over those columns.  On return rows = diag(sigma) V^H padded
 * with the passenger columns; sigma_dev gets `rows` doubles per matrix.
 * Synchronises.  sweeps_host (optional) receives the sweep count.
 * Replaces: scipy.linalg.svd at drift/core/beamtransfer.py:74, :113. */
int dm_jacobi_rows_batched(dm_ctx* ctx, int rows, int cols, int gc0, int gc1, void* Z_dev, int ld, int64_t stride,
                           int batch, double* sigma_dev, int* sweeps_host);

/* The same engine for a ragged list of problems with its options (what the SVD chain hands it; exposed for the
 * parity tests).  Problem i mixes the rows [row0, row0 + nrows) of the row-major matrix at Z (device c128, leading
 * dimension ld) over its columns [0, ncols) until they are orthogonal with respect to the columns [gc0, gc1), and
 * sorts them by descending norm over those columns; nothing outside that row and column range is read or written.
 * Needs 0 <= gc0 <= gc1 <= ncols <= ld, row0 >= 0 and 0 <= nrows <= sigma_stride; Z may be NULL where nrows = 0.
 * sigma_dev gets the nrows row norms of problem i at i * sigma_stride (the rest of its stride is left alone).
 * Options (opts NULL: all defaults):
 *   unconverged      non-zero: the rows are known not to be orthogonal yet, the measuring pass is skipped
 *   drop_below       > 0: rows that end below drop_below * (largest row norm) are kept out of the sweeps
 *   one_stage_eig    non-zero: the Gram eigenproblems of the preconditioner on the one-stage tridiagonalisation
 *   subspace_cut     > 0: only split the rows at subspace_cut * (largest row norm), no order inside the two sides
 *   subspace_margin  how far above the cut the last preconditioner level may begin, in units of the cut
 *                    (0: the engine's default, 3.2e5)
 * The orthogonality reached is RELATIVE, |<y_i, y_j>| <= tol |y_i| |y_j|.  Synchronises.
 * sweeps_host (optional) receives the sweep count.
 * Exposed for the parity tests: this is the engine behind dm_svd_chain and dm_jacobi_rows_batched, as the chain calls
 * it.  On its own it is not a drop-in for a reference call site (matrix_image / matrix_nullspace of
 * drift/core/beamtransfer.py:68-143 also cut at rtol and take the null space from full_matrices: dm_svd_chain does
 * that around this engine). */
typedef struct dm_jacobi_problem_desc {
  void* Z;
  int ld, row0, nrows, ncols, gc0, gc1;
} dm_jacobi_problem_desc;
typedef struct dm_jacobi_options {
  int unconverged;
  double drop_below;
  int one_stage_eig;
  double subspace_cut;
  double subspace_margin;
} dm_jacobi_options;
int dm_jacobi_rows_problems(dm_ctx* ctx, int nprob, const dm_jacobi_problem_desc* probs_host, double* sigma_dev,
                            int sigma_stride, const dm_jacobi_options* opts /* may be NULL */, int* sweeps_host);

/* Two-sided block-Jacobi eigendecomposition of `batch` Hermitian n x n matrices:
 * on return C is diagonal (to working accuracy), W_dev (n x n per matrix, rows
 * are eigenvectors^H) holds the accumulated unitary, evals_dev the unsorted
 * diagonal.  Synchronises.
 * Replaces: the zheevd inside scipy.linalg.eigh, kltransform.py:89, :107. */
int dm_jacobi_herm_batched(dm_ctx* ctx, int n, void* C_dev, int ldc, int64_t strideC, void* W_dev, int ldw,
                           int64_t strideW, int batch, double* evals_dev, int* sweeps_host);

/* Hermitian eigendecomposition of `batch` n x n matrices by Householder
 * tridiagonalisation + implicit QL + blocked back-transformation (the production
 * path of dm_eigh_gen).  C is destroyed; W_dev rows are eigenvectors^H; evals_dev
 * (n per matrix) is NOT sorted.  Returns > 0 if the QL iteration fails.  Synchronises.
 * Replaces: the zheevd inside scipy.linalg.eigh, drift/core/kltransform.py:89, :107. */
int dm_herm_eig_batched(dm_ctx* ctx, int n, void* C_dev, int ldc, int64_t strideC, void* W_dev, int ldw,
                        int64_t strideW, int batch, double* evals_dev);

/* ---- SVD compression of beam-transfer blocks -------------------------------- */
/* Three-stage SVD chain + pseudo-inverse for nblk m-blocks x F frequencies.
 *   beam_m_dev   (nblk, F, T, P, L) c128   noise-unweighted beam_m blocks, T = 2*nbase
 *                                         (the reference's (2, nbase) axes flattened), zero for l < m
 *   noisew_dev   (F, T) f64               noisepower(b, f)^-1/2, duplicated for the two m signs
 *   beam_svd_dev (nblk, F, K, P, L) c128  out, K = min(L, T); rows >= nmodes are zero
 *   invbeam_svd_dev (nblk, F, P, L, K)    out or NULL (skip_svd_inv)
 *   beam_ut_dev  (nblk, F, K, T) c128     out
 *   sigma_dev    (nblk, F, K) f64         out
 *   nmodes_host  (nblk*F) int             out
 *   sweeps_host  optional int[4]: Jacobi sweeps used by SVD1, SVD2, SVD3, pinv
 * SVD1 hands its image and SVD2 its null space to the next SVD as orthonormal bases (:826, :844-848): a unitary change of
 * basis inside either subspace is undone by the next SVD, so on polarised blocks these two phases stop when the cut
 * (1e-10, polsvcut) is placed to the accuracy of a converged SVD and do not order the rows inside each side
 * (sweeps_host[0..1] = 0 then; DM_SVD_SUBSPACE=0 converges them).  sigma, nmodes and every product are those of the
 * reference chain (same spectra to 1e-13 sigma_max).
 * Synchronises.
 * Replaces: BeamTransfer._generate_svdfile_m, drift/core/beamtransfer.py:802-924
 * (matrix_image :68-104, matrix_nullspace :107-143, scipy.linalg.pinv :891). */
int dm_svd_chain(dm_ctx* ctx, int nblk, int F, int T, int P, int L, const void* beam_m_dev,
                 const double* noisew_dev, double polsvcut, void* beam_svd_dev, void* invbeam_svd_dev,
                 void* beam_ut_dev, double* sigma_dev, int* nmodes_host, int* sweeps_host);
/* The same chain for blocks whose columns l < lmin_host[blk] are exactly zero — block blk = the m-block of
 * m = lmin_host[blk], as `BeamTransfer.beam_m` returns it (beamtransfer.py:257-308: l padded from 0).  Zero columns add
 * nothing to an inner product and stay zero under row mixing, so every chain of block blk works on the
 * P * (L - lmin) columns that can be non-zero; products come back in the padded layout, zero for l < lmin.
 *   lmin_host    (nblk) int, 0 <= lmin < L; NULL = all zero (dm_svd_chain)
 * The caller guarantees the zeros (a non-zero entry at l < lmin would be dropped).  Same products as dm_svd_chain up to
 * the order of floating-point sums.  Replaces the same reference lines. */
int dm_svd_chain_lmin(dm_ctx* ctx, int nblk, int F, int T, int P, int L, const int* lmin_host,
                      const void* beam_m_dev, const double* noisew_dev, double polsvcut, void* beam_svd_dev,
                      void* invbeam_svd_dev, void* beam_ut_dev, double* sigma_dev, int* nmodes_host, int* sweeps_host);

/* ---- KL: covariance projection and generalised eigenproblem ---------------- */
/* Project a sky covariance into the SVD basis for nblk m-blocks.
 *   svnum_host   (nblk*F) int   kept modes per frequency (BeamTransfer._svd_num)
 *   l0_host      (nblk) int or NULL: first non-zero l of each block (= m), columns below are skipped
 *   cl_pfl_dev   (P, P, F, F, L) f64: the reference's (P,P,L,F,F) C_l array with l moved last
 *   npol         pol pairs looped: P, or 1 for `temponly`
 *   polmask_host (P*P) int or NULL: non-zero where cl[pi,pj] is not identically zero
 *   out_dev      c128, block b is (ndof_b x ndof_b) row-major at element offset out_off_host[b]
 *   zero_first   flag bits: 1 = clear the outputs before accumulating; 2 = the caller has checked that
 *                cl[pi,pj,f,f',l] == cl[pi,pj,f',f,l] for every pair it passes (the usual sky models): together
 *                with bit 1 and a pol mask without off-diagonal pairs the result is Hermitian block by block and
 *                only the frequency blocks f' >= f are formed, the others mirrored.  Without bit 2 every block
 *                is formed, as the reference does for an arbitrary array.
 * Replaces: BeamTransfer.project_matrix_sky_to_svd, drift/core/beamtransfer.py:1135-1188. */
int dm_project_cov(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev,
                   const int* svnum_host, const int* l0_host, const double* cl_pfl_dev, int npol,
                   const int* polmask_host, void* out_dev, const int64_t* out_off_host, int zero_first);

/* Block-diagonal projection of a diagonal telescope-basis matrix dmat (F, T):
 * block f (+)= alpha (U_f * d_f) U_f^H.
 * Replaces: project_matrix_diagonal_telescope_to_svd, drift/core/beamtransfer.py:1190-1231. */
int dm_project_diag(dm_ctx* ctx, int nblk, int F, int K, int T, const void* beam_ut_dev, const int* svnum_host,
                    const double* dmat_dev, double alpha, void* out_dev, const int64_t* out_off_host,
                    int accumulate);

/* diag(N_b) += reg * max(N_b), numpy's lexicographic complex max.
 * Replaces: drift/core/kltransform.py:289-290. */
int dm_regularise(dm_ctx* ctx, int nblk, const int* n_host, void* mats_dev, const int64_t* off_host, double reg);

/* Generalised Hermitian-definite eigenproblems A v = lambda B v (A, B destroyed).
 * evals (ALL of them) ascending at evals_dev + evoff_host[b]; evecs_dev + off_host[b] holds an
 * (n x n) matrix whose ROWS are the modes (the reference's evecs.T.conj()), row i belonging to
 * eigenvalue i.  add_const_host[b] = diagonal shift applied by the non-positive-definite rescue.
 * cut_mode selects which modes are formed at all (the back-transformation and the final
 * triangular solve are 2/3 of the vector work):
 *   0  all rows;
 *   1  only rows i >= i_ev, i_ev = first index with evals[i] >= cut_value (numpy searchsorted) —
 *      what KLTransform keeps with `subset` (kltransform.py:388-398);
 *   2  only rows i < i_ev — the foreground-clean modes DoubleKL keeps in its first stage (doublekl.py:54-60).
 * The other rows of the block are zero.  nkeep_host[b] (may be NULL) receives the number of rows formed.
 * Returns > 0 if a B stays indefinite after the rescue.  Synchronises.
 * Replaces: eigh_gen, drift/core/kltransform.py:55-121 (+ the threshold cuts cited above). */
int dm_eigh_gen(dm_ctx* ctx, int nblk, const int* n_host, void* A_dev, void* B_dev, const int64_t* off_host,
                double* evals_dev, const int64_t* evoff_host, void* evecs_dev, double* add_const_host,
                int* sweeps_host, int cut_mode, double cut_value, int* nkeep_host);

/* KLTransform._transform_m for nblk m-blocks in one call: S = B C_sg B^H, N = B C_fg B^H (cl_fg_dev NULL: zero) +
 * regulariser * max(N) on the diagonal + noise_scale * U diag(npower) U^H, then dm_eigh_gen with the given cut.
 *   beam_svd_dev (nblk, F, K, P, L), beam_ut_dev (nblk, F, K, T), svnum_host (nblk * F), l0_host (nblk) or NULL
 *   cl_*_dev (P, P, F, F, L) f64 with masks / symmetry flags as for dm_project_cov; npower_dev (F, T) f64
 *   noise_scale  1 with `use_thermal`, (1e-3 / Tsys)^2 without (kltransform.py:292-296)
 *   outputs as dm_eigh_gen (block b of the modes at evecs_dev + off_host[b], (ndof_b x ndof_b), rows = modes)
 * Synchronises.  Replaces: drift/core/kltransform.py:258-355 (sn_covariance + _transform_m). */
int dm_kl_m(dm_ctx* ctx, int nblk, int F, int K, int P, int L, int T, const void* beam_svd_dev, const void* beam_ut_dev,
            const int* svnum_host, const int* l0_host, const double* cl_sg_dev, const int* sg_mask_host, int sg_symmetric,
            const double* cl_fg_dev, const int* fg_mask_host, int fg_symmetric, const double* npower_dev, double noise_scale,
            double regulariser, int cut_mode, double cut_value, double* evals_dev, const int64_t* evoff_host, void* evecs_dev,
            const int64_t* off_host, double* add_const_host, int* nkeep_host);

/* DoubleKL._transform_m for nblk m-blocks in one call: stage 1 diagonalises S against N with the thermal term at
 * floor_scale = (1e-3 / Tsys)^2 and keeps the modes with eigenvalue > foreground_threshold; stage 2 diagonalises the full
 * S, N (thermal term at 1) inside that subspace; the composed modes E2 . E1[kept] are returned.
 *   f_evals_dev  ndof_b stage-1 eigenvalues at evoff_host[b]
 *   evals_dev    the nmodes_host[b] stage-2 eigenvalues at evoff_host[b]
 *   modes_dev    (nmodes_b x ndof_b) at off_host[b]; with cut_mode 1 the rows below the cut are zero and
 *                nkeep_host[b] (may be NULL) counts the rows formed
 *   add_const_host  the stage-1 rescue shift, the one the reference stores (doublekl.py:58)
 * Synchronises.  Replaces: drift/core/doublekl.py:30-87 (without `inverse`). */
int dm_doublekl_m(dm_ctx* ctx, int nblk, int F, int K, int P, int L, int T, const void* beam_svd_dev, const void* beam_ut_dev,
                  const int* svnum_host, const int* l0_host, const double* cl_sg_dev, const int* sg_mask_host, int sg_symmetric,
                  const double* cl_fg_dev, const int* fg_mask_host, int fg_symmetric, const double* npower_dev,
                  double floor_scale, double regulariser, double foreground_threshold, int cut_mode, double cut_value,
                  double* f_evals_dev, double* evals_dev, const int64_t* evoff_host, void* modes_dev, const int64_t* off_host,
                  int* nmodes_host, int* nkeep_host, double* add_const_host);

/* Exact per-m Fisher matrices of the band powers for nblk m-blocks:
 *   C_a = E (B C_l^a B^H) E^H,  F[a][b] = sum_ij C_a[i][j] C_b[j][i] / ((lam_i + 1)(lam_j + 1)).
 *   beam_svd_dev, svnum_host, l0_host   as for dm_project_cov
 *   cl_bands_dev (nbands, F, F, L) f64  band angular power spectra (temperature block), an INPUT
 *   evecs_dev + evecs_off_host[b]       (nmodes_host[b] x ndof_b) c128, rows = KL modes above the threshold
 *   evals_dev + evals_off_host[b]       their eigenvalues (f64)
 *   fisher_dev (nblk, nbands, nbands) c128  out (zero for blocks without modes)
 *   cl_symmetric  non-zero when cl_bands[a,f,f',l] == cl_bands[a,f',f,l] was checked by the caller (see dm_project_cov)
 * Synchronises.
 * Replaces: PSExact.makeproj + _work_fisher_bias_m, drift/core/psestimation.py:672-699, :775-815
 * (the bias of PSExact is identically zero, :797). */
int dm_fisher(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev, const int* svnum_host,
              const int* l0_host, int nbands, const double* cl_bands_dev, const void* evecs_dev,
              const int64_t* evecs_off_host, const int* nmodes_host, const double* evals_dev,
              const int64_t* evals_off_host, void* fisher_dev, int cl_symmetric);

/* Quadratic estimator of the band powers for R data columns per m-block, nblk m-blocks:
 *   x0 = X / (lam + 1),  x2 = B_T^H E^H x0 (temperature only),  q[a] = Re sum_{l >= l0} y2_l^H C^a_l x2_l
 * with y2 formed the same way from Y (or y2 = x2 without Y).
 *   beam_svd_dev, svnum_host, l0_host          as for dm_project_cov
 *   cl_bands_dev (nbands, F, F, L) f64         band angular power spectra (temperature block), as for dm_fisher
 *   evecs_dev + evecs_off_host[b]              (nmodes_host[b] x ndof_b) c128, rows = KL modes
 *   evals_dev + evals_off_host[b]              their eigenvalues (f64)
 *   x_dev + x_off_host[b]                      (nmodes_host[b] x R) c128 data columns (KL coefficients)
 *   y_dev + x_off_host[b]                      the second data set of a cross estimate, or NULL
 *   flags  DM_QEST_NOISE: append the noise term sum_i Re(x0_i conj(y0_i)) w_i, w = (DM_QEST_CROSSPOWER ? 0 : 1)
 *          + (DM_QEST_ZERO_MEAN ? lam_i : 0)
 *   q_dev (nblk, nbands [+1], R) f64           out (zero for blocks without modes)
 * F <= 256.  Fixed-order sums throughout: repeated calls are bit-identical.  Synchronises.
 * Replaces: PSEstimation.q_estimator, drift/core/psestimation.py:582-652 (with Y projected from Y). */
#define DM_QEST_NOISE 1
#define DM_QEST_CROSSPOWER 2
#define DM_QEST_ZERO_MEAN 4
int dm_qestimate(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev, const int* svnum_host,
                 const int* l0_host, int nbands, const double* cl_bands_dev, const void* evecs_dev,
                 const int64_t* evecs_off_host, const int* nmodes_host, const double* evals_dev,
                 const int64_t* evals_off_host, int R, const void* x_dev, const void* y_dev, const int64_t* x_off_host,
                 int flags, double* q_dev);

/* ---- Monte-Carlo Fisher estimators ------------------------------------------- */
/* dm_psmc_draw: sample columns for the Monte-Carlo estimators, drawn on the device.
 *   x_dev + x_off_host[b]  (nmodes_host[b] x R) c128 out: column r is sample s0 + r of m = m_host[b]
 * Draw (i, s) of block b is Philox4x32-10 with key = seed (low word first) and counter (i, s, m, stream):
 *   kind DM_PSMC_NORMAL      complex standard normal, E|z|^2 = 1: Box-Muller with |z| = sqrt(-log u1),
 *                            arg z = 2 pi u2, u1 / u2 the 53-bit uniforms in (0, 1] of words (0, 1) / (2, 3):
 *                            u = ((w_a >> 5) 2^26 + (w_b >> 6) + 1) 2^-53
 *   kind DM_PSMC_RADEMACHER  real -1 if the top bit of word 0 is set, else +1
 * scaled by (lam_i + 1)^(power / 2), power in {-1, 0, 1} (evals_dev + evals_off_host[b], unused for power 0).
 * A draw depends on (seed, m, s, i, stream) alone: the first k of n columns equal a k-column draw bit for bit.
 * Synchronises.
 * Replaces: PSMonteCarlo.gen_sample, drift/core/psmc.py:26-53 (cora's complex_std_normal), and the Z_2 draws of
 *           PSMonteCarloAlt.gen_vecs, drift/core/psmc.py:111-128. */
#define DM_PSMC_NORMAL 0
#define DM_PSMC_RADEMACHER 1
int dm_psmc_draw(dm_ctx* ctx, int nblk, const int* m_host, const int* nmodes_host, const double* evals_dev,
                 const int64_t* evals_off_host, uint64_t seed, int stream, int kind, int power, int s0, int R,
                 void* x_dev, const int64_t* x_off_host);

/* dm_psmc_moments: the sample moments of q (nblk, nq, ns) f64: mean_dev (nblk, nq) and the unbiased covariance
 * cov_dev (nblk, nq, nq) (np.cov, ddof = 1), two passes in a fixed order.  ns >= 2.  Synchronises.
 * Replaces: the np.cov / mean of PSMonteCarlo._work_fisher_bias_m, drift/core/psmc.py:72-89, and of
 *           CrossPower._work_fisher_bias_m, drift/core/crosspower.py:31-45. */
int dm_psmc_moments(dm_ctx* ctx, int nblk, int nq, int ns, const double* q_dev, double* mean_dev, double* cov_dev);

/* dm_psmc_alt: the stochastic-trace Fisher estimate of R sample columns per m-block:
 *   v_a = W E B_T C_a B_T^H E^H X,  W = diag((lam + 1)^-1/2),  F_ab = sum_{i, s} v_a[i, s] conj(v_b[i, s]) / nsamples
 *   beam_svd_dev ... evals_off_host            as for dm_qestimate
 *   x_dev + x_off_host[b]                      (nmodes_host[b] x R) c128 draws, already weighted by (lam + 1)^-1/2
 *   v_dev                                      NULL, or out (nbands, T) c128, T = sum_b nmodes_b R: v_a of block b
 *                                              is (nmodes_b x R) at a T + sum_{b' < b} nmodes_b' R
 *   fisher_dev (nblk, nbands, nbands) c128     out (zero for blocks without modes)
 * Z_a = C_a x2 (band_apply) is formed for every band on the matrix cores and projected back by grouped ZGEMMs; the
 * Gram sums are partial sums per chunk reduced in a fixed order.  F <= 256, nbands <= 128.  Synchronises.
 * Replaces: PSMonteCarloAlt.gen_vecs and _work_fisher_bias_m, drift/core/psmc.py:111-199. */
int dm_psmc_alt(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev, const int* svnum_host,
                const int* l0_host, int nbands, const double* cl_bands_dev, const void* evecs_dev,
                const int64_t* evecs_off_host, const int* nmodes_host, const double* evals_dev,
                const int64_t* evals_off_host, int R, const void* x_dev, const int64_t* x_off_host, int nsamples,
                void* v_dev, void* fisher_dev);

/* ---- Gaussian skies from the covariance models --------------------------------- */
/* dm_sky_draw: correlated draws of spherical-harmonic coefficients for one group of n components (pol, freq):
 *   a[r, i, l, m] = sum_j T_l[i, j] z[r, j, l, m],  rows i in [row0, row0 + nrows), l < L, m < M <= L, r < nreal
 *   T_dev         (L, n, n) f64: the symmetric square root of C_l of the group; row stride ldT, strideT between l
 *   jglobal_host  (n) pol * nfreq + freq of every component: counter word 0 of its draws, and its polarisation
 *   rowoff_host   (n) offset of component i in out_dev, in complex elements (read for the rows of the call)
 *   out_dev       c128: a[r, i, l, m] at rowoff[i] + r stride_real + l stride_l + m stride_m
 * z[r, j, l, m] is one Philox4x32-10 block with key = seed (low word first) and counter
 * (jglobal[j], (l << 16) | m, first + r, stream), mapped as DM_PSMC_NORMAL of dm_psmc_draw: complex with E|z|^2 = 1
 * for m > 0; for m = 0 real with E z^2 = 1 (sqrt(2) Re of that draw, imaginary part exactly 0).  Every element of the
 * range is written: 0 for m > l, and for l < 2 on the components of polarisation 1 and 2 (E, B).  The draws are made in
 * the kernel and multiplied on the matrix cores; the sum over j runs in an order set by n alone, so a coefficient has
 * the same bits whatever rows, M, first / nreal or grouping of calls produced it.  n <= 1024 and L <= 65536; beyond,
 * the call returns an error and launches nothing.  Synchronises.
 * Replaces: cora.core.skysim.mkfullsky (the Gaussian skies the reference's simulations are made from). */
int dm_sky_draw(dm_ctx* ctx, int n, int L, int M, const double* T_dev, int ldT, int64_t strideT,
                const int* jglobal_host, const int64_t* rowoff_host, int nfreq, int row0, int nrows, uint64_t seed,
                int stream, int first, int nreal, void* out_dev, int64_t stride_real, int64_t stride_l,
                int64_t stride_m);

/* dm_source_alm: the exact spherical-harmonic coefficients of nsrc point sources, band-limited at lmax:
 *   a^T_lm(f) = sum_s I_s(f) lambda_lm(z_s) e^{-i m phi_s}   (a^V alike with V_s)
 *   a^E_lm(f) = sum_s e^{-i m phi_s} (W_lm(s) Q_s(f) + i X_lm(s) U_s(f))
 *   a^B_lm(f) = sum_s e^{-i m phi_s} (W_lm(s) U_s(f) - i X_lm(s) Q_s(f))
 *   z_dev, sth_dev, phi_dev  (nsrc) f64: cos and sin of the colatitude, and the longitude reduced to [0, 2 pi)
 *   flux_dev                 (nf, npol, nsrc) f64: temperature x solid angle of (I) or (I, Q, U, V)
 *   alm_dev                  (nf, npol, lmax + 1, m_hi - m_lo + 1) c128, polarisations (T) or (T, E, B, V); every element is
 *                            written, 0 for l < m and for E, B at l < 2
 * lambda, W, X come from the recurrence of the ring tables (a column whose seed is a normal double has their bits), the
 * phases from sincos of the double product m * phi.  The sums over sources run as complex x real products on the matrix
 * cores, sources in chunks of 1024 in catalogue order and m in blocks of 8 aligned to multiples of 8; max_bytes bounds the
 * tables and phased fluxes alive at once (one m-block of one chunk at least) and has no influence on the bits.
 * Errors, with nothing launched: npol other than 1 or 4; m_hi > lmax; npol = 4 and a source with sin theta = 0 whose Q
 * or U is not zero at some frequency (an unpolarised source at a pole is fine).  Synchronises. */
int dm_source_alm(dm_ctx* ctx, int nsrc, const double* z_dev, const double* sth_dev, const double* phi_dev, int nf,
                  int npol, const double* flux_dev, int lmax, int m_lo, int m_hi, void* alm_dev, size_t max_bytes);

/* dm_alm_at_points: spherical-harmonic coefficients evaluated at npts points — the adjoint of dm_source_alm and the
 * synthesis of dm_sht_synth with (z, phi) of a point in the place of (ring, pixel).  With fac = 1 for m = 0, 2 otherwise:
 *   F^T_m(s) = sum_l a^T_lm lambda_lm(z_s)   (F^V alike)
 *   F^Q_m(s) = sum_l a^E_lm W_lm(s) + i a^B_lm X_lm(s),   F^U_m(s) = sum_l a^B_lm W_lm(s) - i a^E_lm X_lm(s)
 *   value_p(s, f) = sum_{j < nm} fac_m Re(F^p_m(s) e^{+i m phi_s}),  m = ms[j]
 *   z_dev, sth_dev, phi_dev  (npts) f64: cos and sin of the colatitude, and the longitude reduced to [0, 2 pi)
 *   ms_host                  (nm) the m of column j of the coefficients: distinct, 0 .. lmax, any order (nm = 0: no term)
 *   alm_dev                  c128: a^p_lm(f) at f stride_f + p stride_p + l stride_l + j stride_m complex elements,
 *                            p = (T) or (T, E, B, V); elements with l < m are not read
 *   out_dev                  (npts, npol, nf) f64, polarisations (T) or (T, Q, U, V): the layout of a spectrum per object
 *   accumulate               0: out = value; otherwise out += value (the sum over the m of the call is formed first)
 * A partial `ms` gives a partial sum; partial sums over disjoint subsets add up to the whole.  One fused kernel runs the
 * recurrence of the Legendre tables in registers, a lane per point and block of frequencies (8 for npol = 1, 4 for
 * npol = 4): no table is written.  A lane adds l ascending inside an m and the m in the order of ms, so the bits of a
 * value do not depend on the other points, on cutting the points or (in multiples of the block) the frequencies into
 * several calls, or on max_bytes, which bounds the re-ordered copy of the coefficients (one block of frequencies at
 * least; the recurrence coefficients, 32 bytes per (l, m), come on top).  The phase is sincos of the double product
 * m * phi.  Errors, with nothing launched or written: npol other than 1 or 4; npts or nf below 1; an m of ms outside
 * 0 .. lmax or repeated; npol = 4 and a point with sin theta = 0 (for npol = 1 a pole is fine).  Synchronises. */
int dm_alm_at_points(dm_ctx* ctx, int npts, const double* z_dev, const double* sth_dev, const double* phi_dev, int nm,
                     const int* ms_host, int lmax, int nf, int npol, const void* alm_dev, int64_t stride_f,
                     int64_t stride_p, int64_t stride_l, int64_t stride_m, double* out_dev, int accumulate,
                     size_t max_bytes);

/* ---- beam-transfer generation (cylinder telescopes) --------------------------- */
/* Host geometry shared by the three calls below: ring_cth_host / ring_sth_host hold
 * cos / sin of the colatitude of the 4*nside-1 HEALPix rings; frame_host (9 doubles)
 * holds xhat (East), yhat (North), zhat (zenith) in sky cartesian coordinates.
 *
 * dm_bt_beam_cyl: field pattern of one (frequency, beam class) on all pixel centres.
 *   kind 0: unpolarised amplitude, out (npix) f64; 1 / 2: X / Y dipole, out (npix, 2) f64
 *   tab_*_host (ntab): knots (x, y, y'') of the natural cubic spline of the E-W
 *   Fraunhofer pattern; fwhm_ns: FWHM of the exptan N-S pattern.
 * Replaces: cylbeam.beam_amp / beam_x / beam_y, drift/telescope/cylbeam.py:101-212,
 *           _fast_tools.beam_exptan, drift/util/_fast_tools.pyx:248-282. */
int dm_bt_beam_cyl(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host,
                   const double* frame_host, int kind, const double* tab_x_host, const double* tab_y_host,
                   const double* tab_y2_host, int ntab, double fwhm_ns, double* out_dev);

/* dm_bt_beams_cyl: nbeam patterns of dm_bt_beam_cyl in one call (one upload of the ring geometry and one of all spline
 * tables instead of eight staged copies per beam).  tab_off_host (nbeam + 1) delimits the knots of each beam in the
 * concatenated tab_x / tab_y / tab_y2 arrays; row b of the output starts at out_dev + b * out_stride (doubles). */
int dm_bt_beams_cyl(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host,
                    const double* frame_host, int nbeam, const int* kind_host, const double* tab_x_host,
                    const double* tab_y_host, const double* tab_y2_host, const int* tab_off_host,
                    const double* fwhm_ns_host, double* out_dev, size_t out_stride);

/* dm_bt_maps: complex visibility response maps for ncol (frequency, baseline) columns:
 * h * fringe * (b_i x b_j) / sqrt(Omega_i Omega_j) -> (ncol, P, npix) c128 with P = 4
 * (I, Q, U, V) if polarised else 1.  beams_dev: nbeam maps from dm_bt_beam_cyl;
 * uv_host (ncol, 2) = baseline / wavelength; bi_host / bj_host (ncol) beam indices.
 * Replaces: _fast_tools.fringe, _construct_pol_real (drift/util/_fast_tools.pyx:18-164),
 *           Unpolarised/PolarisedTelescope._beam_map_single (drift/core/telescope.py:1156-1176, :1268-1283). */
int dm_bt_maps(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host,
               const double* frame_host, int polarised, int nbeam, const double* beams_dev, int ncol,
               const double* uv_host, const int* bi_host, const int* bj_host, void* maps_dev);

/* dm_bt_maps_c: dm_bt_maps for COMPLEX field patterns — beams_dev holds nbeam maps of npix * ncomp complex128 (zero
 * below the horizon); the second beam of a pair enters conjugated and the solid angles are sums of |b|^2.
 * Replaces drift/util/_fast_tools.pyx:167-242 (_construct_pol_complex, reached from telescope.py:1278-1279) and the
 * complex case of UnpolarisedTelescope._beam_map_single (telescope.py:1156-1176). */
int dm_bt_maps_c(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host,
                 const double* frame_host, int polarised, int nbeam, const void* beams_dev, int ncol,
                 const double* uv_host, const int* bi_host, const int* bj_host, void* maps_dev);

/* dm_bt_sht: spherical-harmonic transform of the maps straight into the m-ordered
 * blocks beam_m_dev (mmax+1, F, 2, B, P, lside+1) c128 (the reference's beam_m layout
 * with l padded from 0): rows (f, :, b) of the given columns are overwritten, zero for
 * l < m and l > col_lmax.  lmax_grp = max(col_lmax) <= lside.  Synchronises.
 * Replaces: _transfer_single / transfer_matrices (drift/core/telescope.py:755-830,
 *           :1178-1193, :1287-1316, i.e. cora.util.hputil.sphtrans_complex[_pol]) and the
 *           +/-m fold of BeamTransfer._generate_mfiles (drift/core/beamtransfer.py:620-624). */
int dm_bt_sht(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised,
              int lside, int mmax, int lmax_grp, int F, int B, int ncol, const int* col_f_host,
              const int* col_b_host, const int* col_lmax_host, const void* maps_dev, void* beam_m_dev);

/* dm_sht_synth: spherical-harmonic synthesis of real sky maps, the inverse of the analysis of dm_bt_sht:
 *   maps[f, p, start_r + j] = sum_m c_m Re(F_m(z_r) exp(i m phi_rj)),  c_0 = 1, c_m = 2 (m < min(M, lmax + 1)),
 *   F_m = sum_l a_lm lambda_lm for T and V; F_Q = W a_E + i X a_B, F_U = W a_B - i X a_E (the HEALPix spin-2 functions).
 *   alm_dev   (ncol, P, lmax + 1, M) c128 (a[f, p, l, m], zero for l < m), P = 4 (T, E, B, V) if polarised else 1
 *   maps_dev  (ncol, P, 12 nside^2) f64 out (T or T, Q, U, V in RING order)
 * Needs 4 nside <= 8192.  The device workspace holds the Legendre tables of the call and the harmonic rings of a chunk of
 * columns (at most 1 GiB).  Returns when the work is queued on the context's stream.
 * Replaces: cora.util.hputil.sphtrans_inv_sky (drift/pipeline/timestream.py:262, :295, :451). */
int dm_sht_synth(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised, int lmax,
                 int M, int ncol, const void* alm_dev, void* maps_dev);

/* dm_bt_sht_range: the same for the m-blocks m_lo .. m_hi only; beam_m_dev is then
 * (m_hi - m_lo + 1, F, 2, B, P, L).  A rank that owns a range of m synthesises the maps
 * (replicated, a few per cent of the per-m cost) but transforms and stores only its own blocks —
 * this replaces the reference's (f, b) -> m all-to-all (drift/core/beamtransfer.py:626-640). */
int dm_bt_sht_range(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised,
                    int lside, int m_lo, int m_hi, int lmax_grp, int F, int B, int ncol, const int* col_f_host,
                    const int* col_b_host, const int* col_lmax_host, const void* maps_dev, void* beam_m_dev);

/* dm_bt_sht_opts: dm_bt_sht_range with the two knobs of healpy.map2alm that cora's sphtrans_* may set
 * (neither healpy nor cora is available here, so which values the reference ends up with is not verifiable;
 * the defaults of every other entry point are niter = 0 and equal weights):
 *   niter        Jacobi refinements: coefficients += analysis(map - synthesis(coefficients)), niter times
 *                (healpy's `iter`, default 3 there).  The synthesis uses every (l, m) of a column, whatever m-range
 *                is requested: with niter > 0 the call transforms all m <= lmax_grp into a private buffer first.
 *   ring_w_host  (4 nside - 1) factors on the equal-area quadrature weight of each ring, or NULL
 *                (healpy's `use_weights` multiplies by 1 + w_ring from its data files).
 * Replaces: the same call sites as dm_bt_sht (drift/core/telescope.py:1179-1191, :1288-1312). */
int dm_bt_sht_opts(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised,
                   int lside, int m_lo, int m_hi, int lmax_grp, int F, int B, int ncol, const int* col_f_host,
                   const int* col_b_host, const int* col_lmax_host, const void* maps_dev, void* beam_m_dev, int niter,
                   const double* ring_w_host);

/* dm_bt_columns: dm_bt_maps + dm_bt_sht_range in one call — the visibility response of every pixel is formed in
 * registers inside the ring transform (v_mfma_f64_4x4x4 over the pixels of a ring) and the (ncol, P, npix) Stokes
 * maps are never written to memory; pixels below the horizon are skipped.  Arguments as for those two calls.
 * Returns when the work is queued on the context's stream (host arrays are copied before it returns): call dm_ctx_sync
 * before reading beam_m_dev from the host or from another stream.
 * Replaces: _beam_map_single + _transfer_single + the +/-m fold (drift/core/telescope.py:1156-1193, :1268-1316;
 * drift/util/_fast_tools.pyx:18-164; drift/core/beamtransfer.py:620-624). */
int dm_bt_columns(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, const double* frame_host,
                  int polarised, int nbeam, const double* beams_dev, int ncol, const double* uv_host, const int* bi_host,
                  const int* bj_host, int lside, int m_lo, int m_hi, int lmax_grp, int F, int B, const int* col_f_host,
                  const int* col_b_host, const int* col_lmax_host, void* beam_m_dev, const double* ring_w_host);

/* dm_bt_columns_c: the same for COMPLEX field patterns — beams_dev holds nbeam maps of npix * ncomp complex128 (zero
 * below the horizon), the map values are formed as drift/util/_fast_tools.pyx:169-242 (_construct_pol_complex) and
 * drift/core/telescope.py:1156-1176 form them, inside the ring transform. */
int dm_bt_columns_c(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, const double* frame_host,
                    int polarised, int nbeam, const void* beams_dev, int ncol, const double* uv_host, const int* bi_host,
                    const int* bj_host, int lside, int m_lo, int m_hi, int lmax_grp, int F, int B, const int* col_f_host,
                    const int* col_b_host, const int* col_lmax_host, void* beam_m_dev, const double* ring_w_host);

/* dm_bt_columns_iter: dm_bt_columns / dm_bt_columns_c (complex_beams != 0) with healpy.map2alm's `iter`: after the plain
 * quadrature the coefficients are refined niter times,  a <- a_0 + a - (A o S) a  with A = map2alm(iter = 0), S = alm2map —
 * what healpy does with the residual map, carried out in harmonic space: per m one real Gram matrix of the ring functions
 * under the quadrature (the same for every column) plus the explicit alias terms of the few dozen polar rings with fewer
 * than 2 lmax + 1 pixels.  No Stokes map and no residual map is ever formed; blocks are bit-identical under any partition
 * of m.  healpy's documented default is iter = 3; what cora passes is not verifiable here.  niter = 0 is
 * dm_bt_columns.  Returns when the work is queued on the context's stream.
 * Replaces: the same call sites as dm_bt_columns (cora.util.hputil.sphtrans_complex[_pol] -> healpy.map2alm behind
 * drift/core/telescope.py:1179-1191, :1288-1312). */
int dm_bt_columns_iter(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, const double* frame_host,
                       int polarised, int nbeam, const void* beams_dev, int complex_beams, int ncol, const double* uv_host,
                       const int* bi_host, const int* bj_host, int lside, int m_lo, int m_hi, int lmax_grp, int F, int B,
                       const int* col_f_host, const int* col_b_host, const int* col_lmax_host, void* beam_m_dev,
                       const double* ring_w_host, int niter);

/* dm_bt_alias_info: which m the refinement of an nside group couples through the polar rings (host only, no GPU work):
 * n_alias_rings per cap and mcut (-1: none).  A refined call whose m-range starts at or below mcut transforms
 * m = 0 .. max(m_hi, mcut) internally; callers size their column chunks with it. */
int dm_bt_alias_info(int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised, int lmax_grp,
                     int* n_alias_rings, int* mcut);

/* dm_bt_ring_plan_info: what the fused ring transform of dm_bt_columns / dm_bt_columns_c launches for a call (host only,
 * no GPU work; the launch goes through the same function).  use_fft: the belt rings go by the LDS FFT, with fft_npt
 * pixels per thread and fft_cpw columns per workgroup (both 0 without FFT); nring_dft: rings left to the matrix form;
 * dft_row (4 ints): its kernel as (1 for the shared-synthesis form else 0, P, NMG, NCG), zeros where nring_dft is 0.
 * A call without content (m_lo > lmax_grp or ncol = 0) launches nothing and reports zeros.  DM_BT_FFT and
 * DM_BT_NARROW are honoured as by the launch (both read once per process). */
int dm_bt_ring_plan_info(int nside, int polarised, int m_lo, int m_hi, int lmax_grp, int complex_beams, int ncol,
                         int* use_fft, int* fft_npt, int* fft_cpw, int* nring_dft, int* dft_row);

/* ---- bit truncation of beam-transfer blocks before they are written ------------------------------- */
/* In place on `nrows` rows of `ncols` complex128 values (`ld` elements between rows): every real and
 * imaginary part is rounded to the coarsest multiple of a power of two that keeps its error below
 *   err = max(prec * |z|, prec_max_row * max_j |z_row,j|),
 * ties to even — trailing mantissa bits become zero and the byte planes compress.  Rows are the runs
 * over l of the m-ordered blocks (the reference truncates `m_array.reshape(-1, nl)`).
 * Replaces: caput.truncate.bit_truncate_max_complex at drift/core/beamtransfer.py:641-646 (caput is not
 * vendored with the reference; restated from its documented contract, see oracle/truncate.py). */
int dm_bit_truncate_max_complex(dm_ctx* ctx, void* data_dev, int64_t nrows, int ncols, int64_t ld, double prec,
                                double prec_max_row);

/* ---- the data side: m-mode chain of a timestream ----------------------------------------------------- */
/* dm_blockvec_grouped: y_p = alpha_p op(A_p) x_p for a ragged list of independent problems with FEW right-hand sides, one
 * launch.  Problems are dm_zgemm_problem descriptors read as: A (M x K) through (rsA, csA) with optional conjA, B = x
 * (K x N) through (rsB, csB) with optional conjB, C = y (M x N) row-major with leading dimension ldc; N = R is the same
 * for all problems of a call, 1 <= R <= 8, and beta must be 0.  A problem with M = 0 or K = 0 is skipped: nothing is
 * written.  Bound by the read of A (each element once, 16-byte loads along whichever of the two dimensions is
 * contiguous); every output element is summed by one wave in an order fixed by (K, strides), so the result of a problem
 * does not depend on the rest of the batch.  Returns when the work is queued on the context's stream.
 * Replaces: the np.dot per (m, frequency[, polarisation]) of drift/core/beamtransfer.py:1233-1271, :1366-1421 and
 * drift/core/kltransform.py:710-769 as drift/pipeline/timestream.py:191-231, :306-457 call them. */
int dm_blockvec_grouped(dm_ctx* ctx, int nprob, const dm_zgemm_problem* probs_host);

/* dm_mmode_twiddle: W[t, m] = exp(-2 pi i ((m t) mod ntime) / ntime) / ntime, t < ntime, m <= mmax, row-major
 * (ntime, mmax + 1) c128 — the table of the pruned time -> m transform (a product with dm_zgemm_strided_batched).
 * Replaces: np.fft.fft(timestream) / ntime at drift/pipeline/timestream.py:141-148. */
int dm_mmode_twiddle(dm_ctx* ctx, int ntime, int mmax, void* W_dev);

/* dm_ts_noise: receiver noise of simulated timestreams, drawn in the time domain:
 *   out[r, i, p, t] = sigma[i, p] z,  r < nreal, i < nf, p < npairs, t < ntime
 *   sigma_dev     (nf, npairs) f64 on the device
 *   fglobal_host  (nf) global frequency index of every row i (>= 0)
 *   out_dev       contiguous (nreal, nf, npairs, ntime) c128; every element is written (no memset needed)
 * z is the complex standard normal (E|z|^2 = 1) that dm_psmc_draw and dm_sky_draw map one Philox4x32-10 block to, with
 * key = seed (low word first) and counter (p, fglobal[i], t, ((first + r) << 8) | 24).  The low byte 24 keeps word 3 apart
 * from the Monte-Carlo streams 0, 1, 2 and the sky streams 16, 17 for every realisation.  A draw depends on (seed, pair,
 * global frequency, time sample, realisation) alone: not on the frequencies a call holds, its realisation range or how a
 * caller chunks the work.  first + nreal > 2^24 is refused (dm_last_error) and nothing is launched.  One draw and one
 * 16-byte store per lane, 64-bit element index.  Returns when the work is queued on the context's stream.
 * Replaces: the np.random.standard_normal noise of drift/pipeline/timestream.py:779-798 (same distribution in the time
 * domain at sigma^2 = ntime noisepower, not the same numbers). */
int dm_ts_noise(dm_ctx* ctx, int nreal, int nf, int npairs, int ntime, const double* sigma_dev, const int* fglobal_host,
                uint64_t seed, int first, void* out_dev);

/* ---- per-feed gain errors of simulated timestreams ---------------------------- */
/* dm_ts_gain_coeff: Fourier coefficients of one Gaussian component (amplitude or phase) of the feed gains,
 *   out[r, i, a, k] = sigma ck[k] sqrt(2) conj(z),  r < nreal, i < nf, a < nfeed, k < nk
 *   fglobal_host  (nf) global frequency index of every row i (>= 0); not read when broadband != 0
 *   ck_host       (nk) f64 weights c_k of the spectrum (sum of squares 1)
 *   out_dev       contiguous (nreal, nf, nfeed, nk) c128; every element is written
 * z is the complex normal of dm_ts_noise with key = seed and counter (a, fglobal[i], k, ((first + r) << 8) | stream);
 * broadband != 0 puts 0xFFFFFFFF in the frequency word: one gain per feed for all frequencies (every row i the same).
 * stream is 25 (amplitude) or 26 (phase), apart from 0, 1, 2, 16, 17 and 24.  Re sum_k out[.., k] e^{2 pi i k t / ntime}
 * is the series x(t) = sigma sum_k c_k (A_k cos + B_k sin), A + i B = sqrt(2) z: a product of dm_zgemm_strided_batched
 * with the table of dm_mmode_twiddle.  first + nreal > 2^24 is refused and nothing is launched.  One draw per lane,
 * 64-bit element index.  Returns when the work is queued on the context's stream.  No counterpart in the reference. */
int dm_ts_gain_coeff(dm_ctx* ctx, int nreal, int nf, int nfeed, int nk, const int* fglobal_host, int broadband,
                     const double* ck_host, double sigma, uint64_t seed, int first, int stream, void* out_dev);

/* dm_ts_gain_compose: g[e] = (1 + Re xamp[e]) exp(i Re xphase[e]) for e < n; three contiguous c128 device buffers. */
int dm_ts_gain_compose(dm_ctx* ctx, int64_t n, const void* xamp_dev, const void* xphase_dev, void* g_dev);

/* dm_ts_gain_tile: time samples per workgroup tile of dm_ts_gain_apply for nfeed feeds (host only): the largest power
 * of two <= 16 whose tile nfeed x tile x 16 B fits in 64 KiB, 1 up to the 160 KiB of a CU, 0 when not even one fits. */
int dm_ts_gain_tile(int nfeed);

/* dm_ts_gain_apply: per-feed gains on stacked (unique-baseline) visibilities,
 *   out[r, f, c, t] (+)= G sky[r, f, c, t],  G = (1 / n_c) sum_{(i, j) in class c} g[r, f, i, t] conj(g[r, f, j, t])
 *   class_off_host (npairs + 1), members_host (class_off[npairs], 2): the feed pairs of every class
 *   g_dev    contiguous (g_nreal, nf, nfeed, ntime) c128, g_nreal = 1 (one array for all realisations) or nreal
 *   sky_dev, out_dev (nreal, nf, npairs, ntime) c128, t fastest, distinct buffers; rstride elements lie between the
 *            realisations of both (0: contiguous, nf npairs ntime; larger for a frequency slice of a wider array)
 * accumulate != 0 adds to out (the noise dm_ts_noise drew there: gains multiply the sky part only, the noise level is
 * unchanged — the convention of this library).  The sum of a class runs in an order fixed by (n_c, nfeed) alone, so the
 * same (g, table) gives the same bits in any batch.  Refused before any launch (dm_last_error): an empty class, a feed
 * index outside [0, nfeed), nfeed whose single-sample tile does not fit in LDS.  Returns when the work is queued on the
 * context's stream.  No counterpart in the reference, which simulates a perfectly calibrated telescope. */
int dm_ts_gain_apply(dm_ctx* ctx, int nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                     const int* class_off_host, const int* members_host, const void* g_dev, const void* sky_dev,
                     void* out_dev, int64_t rstride, int accumulate);

/* ---- m-modes of flagged timestreams: batched Toeplitz systems --------------------- */
/* dm_toeplitz_solve: `batch` independent Hermitian positive-definite Toeplitz systems T_s x = b of order n, each given
 * by its first column, solved by the normalised Levinson recursion (2 n^2 complex multiply-adds per right-hand side,
 * n values of storage per system instead of n^2):
 *   col_dev   (batch, n) c128: c_0 .. c_{n-1}, T[k, k'] = c_{k-k'} for k >= k' and conj(c_{k'-k}) otherwise; Im c_0 ignored
 *   b_dev     (batch, nrhs, n) c128: the right-hand sides on entry, the solutions on return
 *   info_dev  (batch) int32 on the device: 0 solved; k in 1 .. n - 1: the system is not positive definite, found at step k
 *             of the recursion (beta <= 0 or not finite); n: c_0 <= 0 or not finite.  A system with info != 0 has every
 *             solution written as zeros; no other system is affected.
 * One system per workgroup (one wave for n <= 384, 256 threads beyond), all of it in LDS: (2 + nrhs) n 16 bytes plus
 * 80 (1 + nrhs) bytes of reduction scratch, at most the 160 KiB of a CU — dm_toeplitz_max_rhs(n) is the largest nrhs
 * that fits.  The order of every sum is a function of n alone: a system has the same bits alone, in any batch and at any
 * position.  batch may exceed 65535 (64-bit element offsets); batch = 0 is a no-op.  Refused before any launch
 * (dm_last_error): n < 1, nrhs < 1, nrhs > dm_toeplitz_max_rhs(n), batch < 0, a null pointer with batch > 0.  Returns
 * when the work is queued on the context's stream.  No counterpart in the reference, which transforms complete days. */
int dm_toeplitz_solve(dm_ctx* ctx, int n, int nrhs, int batch, const void* col_dev, void* b_dev, int* info_dev);

/* dm_toeplitz_max_rhs: the largest nrhs of dm_toeplitz_solve whose LDS need fits one CU for order n (host only), 0 if
 * not even one right-hand side fits (n > 3410) or n < 1.  No counterpart in the reference. */
int dm_toeplitz_max_rhs(int n);

/* dm_toeplitz_solve_diag: dm_toeplitz_solve (the same solutions and info, bit for bit) that also writes the diagonal of
 * the inverse of every system as given:
 *   diag_dev  (batch, n) f64: d_i = (T_s^-1)[i, i].  After the last step of the recursion f / (beta c_0) is the first
 *             column of the inverse, and the Gohberg-Semencul formula gives d_i = sum_{j <= i} (|f_j|^2 - |f_{n-j}|^2) /
 *             (beta c_0) with f_n := 0: one prefix sum over values kept in LDS, whose order is a function of n alone (the
 *             same bits alone, in any batch and at any position).  A system with info != 0 gets a diagonal of zeros.
 * nrhs = 0 is allowed and gives the diagonal alone; b_dev is then not looked at (null or not) and the LDS need is that of
 * r, f and the reduction rows, 32 n + 80 bytes.  Refused before any launch (dm_last_error): n < 1, nrhs < 0,
 * nrhs > dm_toeplitz_max_rhs(n), an order whose LDS need exceeds a CU, batch < 0, a null col, diag or info (or b with
 * nrhs > 0) with batch > 0.  With noise of per-sample variance ntime * noisepower on the data of a weighted m-mode
 * estimate, noisepower * d is the noise variance of the estimated modes.  No counterpart in the reference. */
int dm_toeplitz_solve_diag(dm_ctx* ctx, int n, int nrhs, int batch, const void* col_dev, void* b_dev, double* diag_dev,
                           int* info_dev);

/* ---- unstacked (per-feed-pair) visibilities --------------------------------------- */
/* dm_vis_stack: the weighted, optionally calibrated mean of the redundant feed pairs of every unique baseline.  With the
 * class table of TransitTelescope.redundant_pairs (class_off_host (npairs + 1), members_host (nmem, 2),
 * nmem = class_off[npairs]; row m of the unstacked data is the feed pair (i, j) = members[m]):
 *   N = sum_{m in c} w_m conj(g_i) g_j V_m,   D = sum_{m in c} w_m |g_i|^2 |g_j|^2,   w_m := w[m] fw[i] fw[j]
 *   out[r, f, c, t] = N / D,   wout[r, f, c, t] = D / n_c;   both 0 where D == 0
 *   vis_dev   (nreal, nf, nmem, ntime) c128, t fastest; vis_rstride elements between realisations (0: contiguous)
 *   w_dev     contiguous (w_nreal, nf, nmem, ntime) f64 >= 0, w_nreal = 1 or nreal; null: ones, and no weight is read
 *   g_dev     contiguous (g_nreal, nf, nfeed, ntime) c128 calibration gains, g_nreal = 1 or nreal; null: ones, and
 *             neither LDS nor the member table is touched by the kernel
 *   feed_weight_host (nfeed) f64 >= 0 (0: a dead feed), or null
 *   out_dev   (nreal, nf, npairs, ntime) c128 and wout_dev f64 of the same shape, out_rstride elements between the
 *             realisations of both (0: contiguous); every element is written
 * out is the inverse-variance mean of the calibrated pairs V_m / (g_i conj g_j) without a division per member; its noise
 * variance is the nominal one over wout, which is exactly 1.0 for a complete class with unit weights and no gains.  One
 * workgroup per (realisation, frequency, tile of time samples, chunk of classes); the gains of the tile are staged in LDS
 * (tile = dm_ts_gain_tile(nfeed) with gains, 16 samples without); every element of vis and w is loaded once, 16 bytes
 * per lane.  The order of both sums of a class is a function of (n_c, nfeed) alone: the same bits alone, in any batch, at
 * any position and for any realisation range.  Refused before any launch (dm_last_error): an empty class, class offsets
 * that do not start at 0 or decrease, a feed index outside [0, nfeed), with gains an nfeed whose single-sample tile does
 * not fit in LDS, negative sizes or feed weights, a null vis, out or wout with work to do, out or wout sharing an element
 * with vis (judged on whole spans) or with each other.  nreal, nf, npairs or ntime = 0 is a no-op.  Returns when the work
 * is queued on the context's stream.  No counterpart in the reference, whose data begins at stacked baselines. */
int dm_vis_stack(dm_ctx* ctx, int nreal, int w_nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                 const int* class_off_host, const int* members_host, const void* vis_dev, const double* w_dev,
                 const void* g_dev, const double* feed_weight_host, void* out_dev, double* wout_dev, int64_t vis_rstride,
                 int64_t out_rstride);

/* dm_vis_expand: a stacked sky spread over the feed pairs, with the per-feed gains on it,
 *   out[r, f, m, t] (+)= g[r, f, i, t] conj(g[r, f, j, t]) sky[r, f, c(m), t],  (i, j) = members[m]
 *   g_dev     contiguous (g_nreal, nf, nfeed, ntime) c128, g_nreal = 1 or nreal; null: the class row is copied
 *   sky_dev   (nreal, nf, npairs, ntime) c128, sky_rstride elements between realisations (0: contiguous)
 *   out_dev   (nreal, nf, nmem, ntime) c128, out_rstride elements between realisations (0: contiguous)
 * accumulate != 0 adds to out (the noise dm_ts_noise drew there at the per-member level: gains multiply the sky part
 * only).  Table, layout and refusals of dm_vis_stack; one 16-byte store per lane and member.  Returns when the work is
 * queued on the context's stream.  No counterpart in the reference. */
int dm_vis_expand(dm_ctx* ctx, int nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                  const int* class_off_host, const int* members_host, const void* g_dev, const void* sky_dev, void* out_dev,
                  int64_t sky_rstride, int64_t out_rstride, int accumulate);

/* ---- redundant-baseline calibration -------------------------------------------------- */
/* dm_redcal_solve: per-feed gains g and class visibilities y from the redundancy of the class table alone.  Every
 * (realisation, frequency, time sample) is a problem of its own: minimise
 *   chi^2 = sum_m omega_m |V_m - g_i conj(g_j) y_c|^2,   omega_m = w[m] fw[i] fw[j], but 0 for i == j and 0 on every
 *   member of a class with fewer than two members of i != j and fw[i] fw[j] > 0 (a rule of the table and fw alone)
 * by the damped alternating fixed point, from g0:
 *   y_c = sum omega' conj(g_i) g_j V / sum omega' |g_i|^2 |g_j|^2 (0 where the denominator is 0; omega' is omega without
 *         the second exclusion, so that a class that constrains nothing still gets its calibrated mean)
 *   gh_a = [sum_{m=(a,j)} omega V conj(z) + sum_{m=(i,a)} omega conj(V) conj(z')] / [sum omega |z|^2 + sum omega |z'|^2],
 *         z = conj(g_j) y_c, z' = conj(g_i y_c)  (g_a where the denominator is 0)
 *   g_a <- (1 - damping) g_a + damping gh_a;   step = max_a |delta g_a| / |g_a|  (|g_a| before the update)
 * A sample freezes after the first iteration whose step is below tol: its g no longer changes, its y is computed once
 * more from the final g, iters is that iteration and step its step.  A sample that reaches maxiter with step >= tol
 * keeps the y of its last iteration and reports iters = maxiter and that step: it is not converged, not refused.
 *   vis_dev   (nreal, nf, nmem, ntime) c128, vis_rstride elements between realisations (0: contiguous)
 *   w_dev     contiguous (w_nreal, nf, nmem, ntime) f64 >= 0, w_nreal = 1 or nreal; null: ones
 *   feed_weight_host (nfeed) f64 >= 0 or null;   g0_dev contiguous (nreal, nf, nfeed, ntime) c128 or null: ones
 *   g_dev (nreal, nf, nfeed, ntime) c128, y_dev (nreal, nf, npairs, ntime) c128, iters_dev i32, step_dev f64 and
 *   chi2_dev f64 (nreal, nf, ntime), all contiguous; chi2 is chi^2 at the returned g and y; every element is written
 * Two kernels per iteration on the context's stream: the y step with the arithmetic and summation order of dm_vis_stack,
 * and the gain step, feed-major over an incidence table, which writes the new gains to a second buffer.  The host never
 * waits inside the loop; every 16 iterations it asks, without waiting, whether a sample is left and stops launching
 * once none is.  No floating-point atomics: g, y, iters, step and chi2 of a sample are the same bits alone, in any batch,
 * at any position of a tile and beside any neighbours.  Refused before any launch (dm_last_error): everything
 * dm_vis_stack refuses with gains, damping outside (0, 1], tol negative or not finite, maxiter < 1, a null output (or
 * vis) with work to do, an output sharing an element with vis, w, g0 or another output.  nreal, nf or ntime = 0 is a
 * no-op.  Returns when the last launch is queued.  No counterpart in the reference, whose data begins at stacked
 * baselines. */
int dm_redcal_solve(dm_ctx* ctx, int nreal, int w_nreal, int nf, int nfeed, int npairs, int ntime,
                    const int* class_off_host, const int* members_host, const void* vis_dev, const double* w_dev,
                    const double* feed_weight_host, const void* g0_dev, double damping, double tol, int maxiter,
                    void* g_dev, void* y_dev, int* iters_dev, double* step_dev, double* chi2_dev, int64_t vis_rstride);

/* ---- sky-model gain calibration ---------------------------------------------------------- */
/* dm_modelcal_solve: per-feed gains against a given stacked model M, constant over a solution interval of `interval`
 * consecutive samples: interval q holds the samples q L <= t < min((q + 1) L, ntime), nint = ceil(ntime / L).  Every
 * (realisation, frequency, interval) is a problem of its own: minimise
 *   chi^2 = sum_{t in q} sum_m omega_m(t) |V_m(t) - g_i conj(g_j) M_c(m)(t)|^2,  omega = w[m, t] fw[i] fw[j], 0 for i == j
 * (a class of one member constrains its two feeds: the "fewer than two" rule of dm_redcal_solve does not apply) by the
 * damped StEFCal fixed point, from g0:
 *   gh_a = [sum_t sum_{m=(a,j)} omega V conj(z) + sum_t sum_{m=(i,a)} omega conj(V) conj(z')]
 *          / [sum omega |z|^2 + sum omega |z'|^2],   z = conj(g_j) M_c, z' = conj(g_i M_c)   (g_a where the denominator is 0)
 *   g_a <- (1 - damping) g_a + damping gh_a;   step = max_a |delta g_a| / |g_a|  (|g_a| before the update)
 * An interval freezes after the first iteration whose step is below tol: iters is that iteration and step its step.  One
 * that reaches maxiter with step >= tol reports iters = maxiter and that step: it is not converged, not refused.
 *   vis_dev    (nreal, nf, nmem, ntime) c128, vis_rstride elements between realisations (0: contiguous)
 *   model_dev  contiguous (m_nreal, nf, npairs, ntime) c128, m_nreal = 1 or nreal
 *   w_dev      contiguous (w_nreal, nf, nmem, ntime) f64 >= 0, w_nreal = 1 or nreal; null: ones
 *   feed_weight_host (nfeed) f64 >= 0 or null;   g0_dev contiguous (nreal, nf, nfeed, nint) c128 or null: ones
 *   active_dev contiguous (nf, nint) i32 or null: an interval whose entry is 0 is not solved and returns g0, iters 0,
 *              step 0, chi2 0 and gweight 0
 *   g_dev (nreal, nf, nfeed, nint) c128; iters_dev i32, step_dev f64 and chi2_dev f64 (nreal, nf, nint); gweight_dev
 *   (nreal, nf, nfeed, nint) f64, all contiguous; chi2 is chi^2 and gweight the denominator of every feed at the returned
 *   g (0: the gain is unconstrained); every element is written
 * One kernel per iteration on the context's stream, feed-major over an incidence table, which writes the new gains to a
 * second buffer; one closing kernel for chi2, gweight and g.  The host never waits inside the loop; every 16 iterations
 * it asks, without waiting, whether an interval is left and stops launching once none is.  No floating-point atomics: the
 * five outputs of an interval are the same bits alone, in any batch and beside any neighbours.  Refused before any launch
 * (dm_last_error): everything dm_vis_stack refuses with gains, an nfeed whose gains of one interval (16 nfeed + 64 bytes)
 * do not fit in 64 KiB of LDS, interval < 1, damping outside (0, 1], tol negative or not finite, maxiter < 1, w_nreal or
 * m_nreal neither 1 nor nreal, a null output (or vis, model) with work to do, an output sharing an element with vis,
 * model, w, g0, active or another output.  nreal, nf or ntime = 0 is a no-op.  Returns when the last launch is queued.
 * No counterpart in the reference, whose data begins at stacked, calibrated baselines. */
int dm_modelcal_solve(dm_ctx* ctx, int nreal, int w_nreal, int m_nreal, int nf, int nfeed, int npairs, int ntime,
                      int interval, const int* class_off_host, const int* members_host, const void* vis_dev,
                      const void* model_dev, const double* w_dev, const double* feed_weight_host, const void* g0_dev,
                      const int* active_dev, double damping, double tol, int maxiter, void* g_dev, int* iters_dev,
                      double* step_dev, double* chi2_dev, double* gweight_dev, int64_t vis_rstride);

/* ---- sidereal stacking ----------------------------------------------------------------- */
/* dm_sidereal_regrid: one day of every row, sampled at phi_j = phi0 + j dphi (j = 0 .. nt_in - 1, dphi > 0, less than
 * one turn), resampled onto the sidereal grid phi_k = 2 pi k / ntime and written to, or added to, the accumulators of
 * the stack.  With s = max(1, (2 pi / ntime) / dphi) and u = (phi_k + 2 pi n - phi0) / dphi in [0, 2 pi / dphi), the taps
 * of k are the j in [ceil(u - a s), floor(u + a s)] with c_j = L_a((u - j) / s) != 0, L_a(t) = sinc(t) sinc(t / a) inside
 * |t| < a; a tap outside [0, nt_in) exists and counts as flagged, as does one with w > 0 false (0, negative, NaN), whose
 * data value reaches nothing.  With A, S = sum |c_j|, sum c_j over the unflagged taps and A_all, S_all over all, the
 * sample is valid iff an unflagged tap exists, A >= min_share A_all (for min_share = 1: no tap is missing, decided by
 * the count) and S >= S_all / 2; then xh = sum (c_j / S) x_j, W = 1 / sum ((c_j / S)^2 / w_j) and
 *   sum += W xh,  wsum += W,  sq += W |xh|^2,  hits += 1;
 * else W = 0 and nothing is added.  A u within 1e-9 of an integer is that integer and a cadence ratio within 1e-9 of 1
 * is 1, so on-grid data at equal cadence has one tap of coefficient 1 and is copied whatever its neighbours' flags.
 *   x_dev    (nf, nrow, nt_in) c128, contiguous, t fastest;   w_dev f64 of that shape or null: ones, no weight is read
 *   sum_dev  (nf, nrow, ntime) c128, wsum_dev f64 of that shape; sq_dev f64 and hits_dev i32 of that shape, each may be
 *            null and is then not kept
 *   accumulate == 0: every element of every output given is written, zeros where the sample is not valid;
 *   accumulate != 0: valid samples are added, all others are left bit for bit as they were
 * The tap geometry depends on the day alone: it is made on the host in long double, rounded to double and uploaded once
 * per call.  One workgroup per (frequency, tile of up to 16 rows, tile of up to 64 grid samples) stages the input span
 * of its taps in LDS once, 16 bytes of x and 8 of w per lane with t contiguous across the lanes, so every element comes
 * from HBM once up to the halo of a tile; a lane then owns one grid sample of up to 4 rows.  The tap sum of a sample runs
 * in tap order whatever the row, batch or tile: the same bits alone, in any batch of rows or frequencies and at any
 * position of a tile.  No atomics.  W is the diagonal weight only: neighbouring regridded samples share taps and are
 * correlated.  Refused before any launch (dm_last_error): a outside 1..8, phi0 or dphi not finite or dphi <= 0,
 * (nt_in - 1) dphi >= 2 pi, min_share outside (0, 1], ntime < 1, negative sizes, more than dm_sidereal_max_taps() taps
 * (2 a s + 1), a null x, sum or wsum with work to do, an output sharing an element with x, w or another output.  nf, nrow
 * or nt_in = 0 is a no-op, except that with accumulate == 0 the outputs are zeroed.  Returns when the work is queued on
 * the context's stream.  No counterpart in the reference, whose data begins at the finished sidereal stream. */
int dm_sidereal_regrid(dm_ctx* ctx, int nf, int nrow, int nt_in, int ntime, int a, double phi0, double dphi,
                       double min_share, const void* x_dev, const double* w_dev, void* sum_dev, double* wsum_dev,
                       double* sq_dev, int* hits_dev, int accumulate);
/* the cap on 2 a s + 1, the taps of one grid sample (host only) */
int dm_sidereal_max_taps(void);

/* ---- RFI flagging along time ---------------------------------------------------------- */
/* dm_rfi_flag: an iterated SumThreshold (Offringa et al. 2010) on every (frequency, row) series of one day, and the
 * weights of the day with the flagged samples at 0.  x (nf, nrow, nt) complex128 and w (nf, nrow, nt) float64 or null
 * (ones), contiguous; a sample with w > 0 false (0, negative, NaN) is input flagged (the set I) and its data value, NaN
 * included, reaches nothing.  A series is cut into nseg = ceil(nt / segment) balanced segments
 * [floor(s nt / nseg), floor((s + 1) nt / nseg)), which are independent; windows are truncated at their edges.
 * Tables, made on the host in long double and rounded to double once: g_d = exp(-d^2 / (2 kernel_sigma^2)), d = 0 .. H,
 * H = ceil(3 kernel_sigma); t[it][M] = alpha + chi1 rho^(-log2 M) base^(niter - 1 - it) beta with
 * alpha = sqrt(pi / (4 ln 2)), beta = sqrt((1 - pi / 4) / ln 2), the mean and the standard deviation of a Rayleigh
 * amplitude in units of its median.  Per segment, with B = I at the start, for it = 0 .. niter - 1: (1) fewer than
 * min_good samples outside B: the whole segment is flagged, its noise is 0, stop; (2) for j outside I the background
 * b_j = sum g_|d| x_{j+d} / sum g_|d| over d = -H .. H ascending, over the samples inside the segment and outside B, one
 * FMA per component and term, and a_j = sqrt(re(r)^2 + im(r)^2), r = x_j - b_j; a sample with no usable sample in its
 * window is unjudgeable; (3) m = the lower median of a_j over j outside B (rank (c - 1) / 2 of c), an exact order
 * statistic; (4) D = I and the unjudgeable samples; for every window length M <= n in ascending order, every window
 * [j, j + M) of the segment: over its samples outside D as D stood at the start of the pass, c their count and S the sum
 * of a_k in ascending k; the window hits iff c >= 1 and S > c (m t[it][M]); after the pass all samples of hitting
 * windows join D; (5) B = D.  The flags of the segment are the last B and noise = m / sqrt(ln 2).
 * Occupancy: with n_in the rows of a frequency where sample j is outside I and n_new the rows where detection flagged
 * it anew, j is flagged in every row of the frequency when n_in > 0 and n_new > row_share n_in (row_share = 1: never).
 * Outputs: w_out (nf, nrow, nt) = w (or 1) where kept, bit for bit, and 0 where flagged, and it may be w itself;
 * noise (nf, nrow, nseg); nflag (nf, nrow) int32, the new flags of detection in the row; occupancy (nf, nt) int32, n_new.
 * A row has the same bits in w_out and noise alone, in any batch, at any row index and with any other frequency.  No
 * floating-point atomics.  Refused before any launch (dm_last_error): negative sizes, segment outside
 * 1 .. dm_rfi_max_segment(), kernel_sigma not finite or <= 0 or H > 32, nwin outside 1..7 or windows that are not
 * ascending powers of two <= 64, chi1 <= 0, rho < 1, base < 1 or any of them not finite, niter outside 1..8,
 * min_good < 1, row_share outside (0, 1], a null x or output with work to do, an output sharing an element with x, w
 * (other than w_out == w) or another output.  nf, nrow or nt = 0 is a no-op.  Returns when the work is queued on the
 * context's stream.  No counterpart in the reference, whose data begins at the finished sidereal stream. */
int dm_rfi_flag(dm_ctx* ctx, int nf, int nrow, int nt, int segment, double kernel_sigma, int nwin,
                const int* windows_host, double chi1, double rho, int niter, double base, int min_good, double row_share,
                const void* x_dev, const double* w_dev, double* wout_dev, double* noise_dev, int* nflag_dev,
                int* occupancy_dev);
/* the cap on `segment`, set by the LDS layout of the row kernel (host only) */
int dm_rfi_max_segment(void);

/* ---- RFI flagging along frequency and the dilation of flags ---------------------------- */
/* dm_rfi_flag_freq: the method of dm_rfi_flag, word for word, on the series x[:, row, j] of every (row, j): nf takes
 * the place of nt in the segments (nseg = ceil(nf / segment) balanced segments over the frequencies), in the
 * background, the median, the window passes and min_good; the occupancy rule runs over the rows of a (f, j) as it does
 * there.  With xt = x transposed to (nt, nrow, nf) and wt likewise, the outputs are those of dm_rfi_flag(xt, wt)
 * transposed back, bit for bit: w_out (nf, nrow, nt), which may be w itself; noise (nseg, nrow, nt); nflag (nrow, nt)
 * int32, the new flags of every series; occupancy (nf, nt) int32.  No floating-point atomics.  Refused before any launch
 * (dm_last_error): what dm_rfi_flag refuses, with nf in the place of nt.  nf, nrow or nt = 0 is a no-op.  Returns when
 * the work is queued on the context's stream.  No counterpart in the reference. */
int dm_rfi_flag_freq(dm_ctx* ctx, int nf, int nrow, int nt, int segment, double kernel_sigma, int nwin,
                     const int* windows_host, double chi1, double rho, int niter, double base, int min_good,
                     double row_share, const void* x_dev, const double* w_dev, double* wout_dev, double* noise_dev,
                     int* nflag_dev, int* occupancy_dev);
/* the series of consecutive j that one workgroup of dm_rfi_flag_freq takes when the longest balanced segment,
 * ceil(nf / nseg), has segment_len samples: 8 up to 512, 4 up to 1024, 2 up to dm_rfi_max_segment(); 0 for a length it
 * does not take (host only) */
int dm_rfi_freq_tile(int segment_len);
/* dm_rfi_dilate: the scale-invariant rank operator (Offringa, van de Gronde & Roerdink 2012) in exact integers on every
 * series of w (nf, nrow, nt) float64 along axis 0 (time: the series w[f, row, :]) or 1 (frequency: w[:, row, j]).  F =
 * the samples where w > 0 is false; I = those where w_ref > 0 is false (w_ref of the shape of w, or null: none): they
 * are missing, stay as they are and count neither as flags nor as length.  kappa = rint((1 - eta) 65536), in double;
 * psi_i = 0 on I, 65536 - kappa on F \ I, -kappa elsewhere; P_0 = 0, P_{k+1} = P_k + psi_k; a sample j outside I is
 * flagged iff max_{b > j} P_b >= min_{a <= j} P_a: some window holding j has at least the share kappa / 65536 of its
 * present samples flagged.  The whole series is one unit.  w_out = w bit for bit where kept and 0 where newly flagged,
 * and it may be w itself; nadded int32, the newly flagged samples of every series: (nf, nrow) along time, (nrow, nt)
 * along frequency.  Refused before any launch (dm_last_error): negative sizes, another axis, eta not finite or outside
 * [0, 1), kappa < 1, a series longer than dm_rfi_dilate_max_length(axis), a null w, w_out or nadded with work to do, an
 * output sharing an element with w or w_ref (other than w_out == w) or with the other output.  nf, nrow or nt = 0 is a
 * no-op.  Returns when the work is queued on the context's stream.  No counterpart in the reference. */
int dm_rfi_dilate(dm_ctx* ctx, int nf, int nrow, int nt, int axis, double eta, const double* w_dev,
                  const double* wref_dev, double* wout_dev, int* nadded_dev);
/* the longest series dm_rfi_dilate takes along the axis: 16384 along time (0), dm_rfi_max_segment() along frequency
 * (1); 0 for another axis (host only) */
int dm_rfi_dilate_max_length(int axis);

/* ---- the delay fit along frequency ------------------------------------------------------ */
/* dm_delay_fit: one weighted least-squares fit of a band-limited basis per series x[:, row, t] of x (nf, nrow, nt)
 * complex128.  w (nf, nrow, nt) float64 or null (ones); a sample is kept iff w > 0 (false for 0, negatives and NaN),
 * omega_f = w_f on kept samples and 0 elsewhere, and x of a sample that is not kept is never read into arithmetic.
 * nbasis real bases, basis k of rank rank_host[k] stored (r_k, nf) row-major from nf sum_{j<k} r_j doubles of basis_dev;
 * basis_of_dev (nrow,) int32 names the basis of a row.  With A the basis of the row, a_f its row f and r its rank:
 * nvalid = the kept samples, s = sum_f omega_f / nf; nvalid < min_valid (min_valid <= 0: r) or nvalid = 0 gives
 * info = -1; G = sum_f omega_f a_f a_f^T + ridge s I = L L^T, a pivot that is not finite or not > 0 at column j gives
 * info = j + 1; c = G^-1 sum_f omega_f a_f x_f, model_f = a_f^T c, v_f = |L^-1 a_f|^2.  mode 0 (model): x_out = model
 * everywhere, w_out = w on kept samples and 0 on flagged ones; 1 (filter): x_out = x - model on kept samples and 0 on
 * flagged, w_out as before; 2 (inpaint): x_out = x bit for bit on kept samples and model on flagged, w_out = w on kept
 * and 1 / v_f on flagged (0 where v_f is not finite and positive).  A series that is not solved (info != 0) gives
 * x_out = x on kept samples (0 in mode 0) and 0 on flagged, w_out = w on kept and 0 on flagged.  A basis_of entry
 * outside [0, nbasis) gives info = -2 for the series of its row, which are handled as not solved.  info (nrow, nt) int32.
 * x_out may be x and w_out may be w.  No floating-point atomics; the bits of a (row, t) depend on nothing else in the
 * launch; the accumulation orders are those of section 4.23.  Refused before any launch (dm_last_error): negative sizes,
 * another mode, a ridge that is not finite or negative, and with work to do: nf > dm_delay_max_nf(), nbasis < 1 or
 * > 256, a rank < 1, > nf or > dm_delay_max_rank(), a null pointer other than w, an output sharing an element with an
 * input (other than x_out == x, w_out == w) or with another output.  nf, nrow or nt = 0 is a no-op.  Returns when the
 * work is queued on the context's stream.  No counterpart in the reference. */
int dm_delay_fit(dm_ctx* ctx, int nf, int nrow, int nt, int mode, double ridge, int min_valid, int nbasis,
                 const int* rank_host, const double* basis_dev, const int* basis_of_dev, const void* x_dev,
                 const double* w_dev, void* xout_dev, double* wout_dev, int* info_dev);
/* the most frequencies and the largest rank dm_delay_fit takes (host only) */
int dm_delay_max_nf(void);
int dm_delay_max_rank(void);
/* the series of consecutive t that one workgroup of dm_delay_fit takes for nf frequencies and a largest rank max_rank
 * in the table; 0 for a pair it does not take (host only) */
int dm_delay_tile(int nf, int max_rank);

/* ---- ring maps: the north-south beamformer of stacked visibilities ---------------------- */
/* dm_ringmap: for every frequency f, group g, elevation e and sample t
 *   map[f, g, 0, e, t] = sum_b x_b(t) Re(V_b(t) exp(-2 pi i tau_be)) / D(t),   map[f, g, 1, e, t] the same with Im
 *   (parts = 2 only),   x_b(t) = taper_b w_b(t),   D(t) = sum_b x_b(t),   D2(t) = sum_b taper_b x_b(t),
 *   tau_be = (scale[f] v_b) sinza[e] in turns, taken as tau - rint(tau) into sincospi,
 * the sums over the members b of the group: group g lists the rows members[group_off[g] .. group_off[g + 1]) of vis
 * (nf, nrow, nt) complex128; a row may sit in several groups and the rows of a group need not be contiguous.
 * group_off (ngroup + 1) and members (group_off[ngroup]) int32 are HOST tables; v and taper (per member, float64,
 * taper null: ones), scale (nf) and sinza (nel, any values) are on the device.  w (nf, nrow, nt) float64 or null
 * (ones): a sample is kept iff w > 0 (false for 0, negatives and NaN), and vis and w of a sample that is not kept
 * reach no arithmetic.  map (nf, ngroup, parts, nel, nt), norm = D and norm2 = D2 (nf, ngroup, nt) float64, either of
 * the two null: not written.  Where D(t) = 0 the map, D and D2 are exactly 0.  An output is one fp64 MFMA accumulator
 * walked through the members in list order, four at a time; D and D2 are sequential sums in list order: the bits of
 * (f, g, ., e, t) depend on nothing else in the launch, and plane 0 of parts = 2 is the parts = 1 result.  No table in
 * memory, no weighted copy, no atomics; no limit on the group size or nel.  Refused before any launch (dm_last_error):
 * negative sizes, parts outside {1, 2}, and with work to do: a null group_off, scale, sinza or map, null members, v or
 * vis with members listed, group_off[0] < 0, a decreasing group_off, a member outside [0, nrow), an output sharing an
 * element with an input or another output, more than 2^31 - 1 workgroups (128 elevations x 128 samples each).
 * nf, nt, ngroup or nel = 0 is a no-op.  Returns when the work is queued on the context's stream.  No counterpart in
 * the reference. */
int dm_ringmap(dm_ctx* ctx, int nf, int nrow, int nt, int ngroup, const int* group_off_host, const int* members_host,
               const double* v_dev, const double* taper_dev, const double* scale_dev, int nel, const double* sinza_dev,
               int parts, const void* vis_dev, const double* w_dev, double* map_dev, double* norm_dev, double* norm2_dev);

/* ---- formed beams: tracking beams on catalogue positions from stacked visibilities ------ */
/* dm_formed_beam: for every frequency f, group p and source s, over the samples k = k0[s] + j (mod nt), j = -half[s] ..
 * half[s], and the members b of the group
 *   D = turn[s] - k / nt reduced to [-1/2, 1/2],   x = sinth[s] sin(2 pi D),   y = yc0[s] - yc1[s] cos(2 pi D),
 *   A = exp(-env[f] x x)  (1 where env[f] = 0),   x_b(k) = taper_b w_b(k),
 *   tau = (scale[f] u_b) x + (scale[f] v_b) y in turns, each product taken as t - rint(t) into sincospi,
 *   beam[f, p, 0, s] = sum_k sum_b A x_b(k) Re(V_b(k) exp(-2 pi i tau)) / D,   beam[f, p, 1, s] the same with Im
 *   (parts = 2 only),   D = sum_k sum_b A x_b(k),   D2 = sum_k sum_b A A x_b(k).
 * Group p lists the rows members[group_off[p] .. group_off[p + 1]) of vis (nf, nrow, nt) complex128; member m has
 * u = uvals[iu[m]] and v = vvals[iv[m]] (m).  group_off (ngroup + 1), members, iu, iv (group_off[ngroup]), k0 and half
 * (nsrc) int32 and env (nf) float64 are HOST tables; uvals (nu), vvals (nv), taper (per member, null: ones), scale (nf),
 * turn, sinth, yc0 and yc1 (nsrc) float64 are on the device.  w (nf, nrow, nt) float64 or null (ones): a sample is kept
 * iff w > 0 (false for 0, negatives and NaN), and vis and w of a sample that is not kept reach no arithmetic.  half[s] =
 * -1 drops the source.  beam (nf, ngroup, parts, nsrc), norm = D and norm2 = D2 (nf, ngroup, nsrc) float64, either of the
 * two null: not written; where D = 0 all three are exactly 0.  A workgroup takes one (f, p) and dm_formedbeam_block()
 * sources of the catalogue sorted by k0 (the sort is made here) and walks the union of their windows; a tile of x V is
 * staged in LDS once for all of them.  A group with at most dm_formedbeam_max_nu() distinct u takes the factorised path
 * (cos / sin once per distinct u and per run of equal v, a complex multiply per member), any other the direct one (one
 * sincospi per member).  The result of (f, p, ., s) is summed in a fixed order that depends on the window of s and the
 * member list of p only: its bits do not depend on the other sources, their order, the other
 * groups or frequencies of the launch, or on norm / norm2 being null, and plane 0 of parts = 2 is the parts = 1 result.
 * No phase table and no weighted copy in memory, no floating-point atomics.  Refused before any launch (dm_last_error):
 * negative sizes, parts outside {1, 2}, and with work to do: a null group_off, scale, env, k0, half, turn, sinth, yc0,
 * yc1 or beam, a negative or non-finite env, half < -1 or 2 half + 1 > nt, k0 outside [0, nt), null members, iu, iv,
 * uvals, vvals or vis with members listed, group_off[0] < 0, a decreasing group_off, a member outside [0, nrow), iu or iv
 * outside its table, an output sharing an element with an input or another output, more than 2^31 - 1 workgroups.
 * nf, nt, ngroup or nsrc = 0 is a no-op.  Returns when the work is queued on the context's stream.  No counterpart in
 * the reference. */
int dm_formed_beam(dm_ctx* ctx, int nf, int nrow, int nt, int ngroup, const int* group_off_host, const int* members_host,
                   const int* iu_host, const int* iv_host, int nu, const double* uvals_dev, int nv, const double* vvals_dev,
                   const double* taper_dev, const double* scale_dev, const double* env_host, int nsrc, const int* k0_host,
                   const int* half_host, const double* turn_dev, const double* sinth_dev, const double* yc0_dev,
                   const double* yc1_dev, int parts, const void* vis_dev, const double* w_dev, double* beam_dev,
                   double* norm_dev, double* norm2_dev);
/* the sources of a workgroup of dm_formed_beam, and the distinct u of a group up to which it takes the factorised path
 * (host only) */
int dm_formedbeam_block(void);
int dm_formedbeam_max_nu(void);

/* ---- delay power spectra of stacked visibilities with their window function ------------- */
/* dm_delay_spectrum: for every row r, sample t, delay a = 0 .. nd - 1 and lag d = 0 .. nd - 1
 *   y_f = T_f omega_f,   omega_f = 1 (weighting 0) or w_f (weighting 1) on kept samples and 0 elsewhere,
 *   phi_fk = step_f k, one rounded product, reduced as phi - rint(phi) (exact) into sincospi,
 *   D_a(t) = sum_f y_f x_f exp(2 pi i phi_f,(a - a0)),
 *   W_d(t) = sum_f y_f exp(2 pi i phi_f,d),
 * and for every bin b of samples, over its used series (those with at least min_valid >= 1 kept channels)
 *   q[r, b, a] = sum_t |D_a(t)|^2,   h[r, b, d] = sum_t |W_d(t)|^2,
 *   s1[r, b] = sum_t sum_f T_f^2 omega_f,   s2[r, b] = sum_t sum_f T_f^2 omega_f^2,   count[r, b] = the used series.
 * x (nf, nrow, nt) complex128; w (nf, nrow, nt) float64 or null (ones): a sample is kept iff w > 0 (false for 0,
 * negatives and NaN), and x and w of a sample that is not kept reach no arithmetic.  taper (nf, null: ones) and step
 * (nf, turns per delay step of every channel: (nu_f - nu_ref) dtau) float64 are on the device.  bin_off (nbin + 1) int32
 * is a HOST table: bin b holds the samples bin_off[b] .. bin_off[b + 1] - 1, ascending and within [0, nt]; the samples
 * outside every bin are not used.  q and h (nrow, nbin, nd), s1 and s2 (nrow, nbin) float64, count (nrow, nbin) int32;
 * h, s1, s2 and count may be null: not written.  A bin with no used series gives exact zeros everywhere.  With real
 * weights the window matrix of q, F_ab = sum_t |W_(a - b)(t)|^2, depends on |a - b| alone: h is the first column of
 * that symmetric Toeplitz matrix, and s1 (inverse-variance weights) or s2 (unit weights, uniform variance) the noise
 * bias of q.
 * The products run on the fp64 MFMA with the phases made in registers and the weighting on the way into LDS: no phase
 * table, no weighted copy and no transformed cube in memory, no floating-point atomics.  The order of every sum is a
 * function of nf and of the bin's sample range alone (dm_delayspec.hip states it; a bin of more than 128 samples is cut
 * into dm_delayspec_segments() segments whose partial sums a second kernel adds in ascending order from scratch memory
 * of at most 4 (2 nd + 2) doubles per (row, bin)): the bits of (r, b, .) do not depend on the other rows and bins, on nd
 * (a smaller nd gives a prefix of h, and of q for the same a0) or on which optional outputs are null.  Refused before
 * any launch (dm_last_error): negative sizes, weighting outside {0, 1}, nf > dm_delayspec_max_nf(), nd >
 * dm_delayspec_max_nd(), min_valid < 1, a0 outside [0, nd) (for nd > 0), and with work to do: a null x, step, bin_off
 * or q, a bin_off that decreases or leaves [0, nt], an output sharing an element with an input or another output, nrow
 * or nbin > 65535.  nf, nrow, nt, nbin or nd = 0 is a no-op.  Returns when the work is queued on the context's stream.
 * No counterpart in the reference. */
int dm_delay_spectrum(dm_ctx* ctx, int nf, int nrow, int nt, int nd, int a0, int weighting, int min_valid,
                      const double* taper_dev, const double* step_dev, int nbin, const int* bin_off_host,
                      const void* x_dev, const double* w_dev, double* q_dev, double* h_dev, double* s1_dev,
                      double* s2_dev, int* count_dev);
/* the most frequencies and delays dm_delay_spectrum takes (host only) */
int dm_delayspec_max_nf(void);
int dm_delayspec_max_nd(void);
/* the segments that dm_delay_spectrum cuts a bin of nsamples samples into, and in *length (may be null) the samples of
 * each but the last (host only; 0 for nsamples <= 0) */
int dm_delayspec_segments(int nsamples, int* length);

#ifdef __cplusplus
}
#endif
#endif /* DRIFTMI_H */
