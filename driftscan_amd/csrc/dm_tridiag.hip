// dm_tridiag.hip — batched Hermitian eigensolver: Householder tridiagonalisation, divide & conquer
// on the real tridiagonal, and compact-WY back-transformation.
//
// This is the zheevd step of scipy.linalg.eigh(A, B) (drift/core/kltransform.py:89)
// for every m-block at once.  All matrices of the batch advance in lock-step, so a
// launch always carries (#matrices x #row tiles) workgroups:
//
//   T1  tridiagonalisation (LAPACK zhetrd/zlatrd recurrences, panels of 32 or 64 reflectors, upper triangle only):
//         trd_symv  p = A v reading each stored element once + Householder scalars  (HBM-bound: the roofline of T1)
//         trd_wx    w = tau p - (tau/2)(p^H v) v and the next column, one pass over the panel
//         her2k     A -= [V W][W V]^H once per panel, K = 2 x panel width           (grouped ZGEMM, MFMA)
//       or, for the batches trd_policy_of sends there, the two-stage reduction of dm_sbr_impl.h
//       (dense -> band on MFMA, band -> tridiagonal by bulge chasing)
//   T2  divide & conquer (LAPACK dstedc): leaves of at most 32 rows by implicit QL with the rotations
//       applied in LDS, merges by the secular equation and a ZGEMM per node.  A batch of at most
//       32 rows (or DM_EIG_QL) takes the implicit QL instead: ql_kernel, one wave (lane 0) per matrix,
//       records the Givens rotations sweep by sweep, and
//   T3  rot_apply   applies them to Z = I, one thread per ROW of Z, sixteen consecutive sweeps
//                   pipelined through a register window (HBM-bound / 16)
//   T4  back-transformation X = H_0 ... H_{n-2} Z in compact-WY blocks             (grouped ZGEMM, MFMA)
//
// Flop count ~ (16/3 + 8 + ...) n^3 against the ~1400 n^3 the two-sided block-Jacobi
// solver needs on the graded spectra of KL problems; accuracy is LAPACK's (backward
// stable, |d lambda| ~ eps |lambda_max|).
#include "dm_common.h"
#include "dm_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <thread>

// The panel width is a compile-time constant of the kernels (LDS arrays, T-factor layout): the body is
// compiled twice.  Narrow panels halve the traffic on the panel vectors V, W (a third of what trd_symv and
// trd_wx move once the trailing matrices are a few hundred rows) and win up to n ~ 2000 — the Gram matrices
// of the SVD preconditioner, the KL problems of config 2: 864 x 512 matrices 0.465 -> 0.409 s; wide panels
// keep the her2k updates at K = 128 where the MFMA products dominate (n = 12 000: 2.23 s against 2.34 s).
#define DM_TNB 32
#define DM_TRD_NS dm_trd32
#include "dm_tridiag_impl.h"
#undef DM_TNB
#undef DM_TRD_NS
#define DM_TNB 64
#define DM_TRD_NS dm_trd64
#include "dm_tridiag_impl.h"
#undef DM_TNB
#undef DM_TRD_NS

namespace {
struct trd_policy {
  int width;       // panel width of the one-stage reduction; the two-stage reduction exists in the 32-wide build only
  bool two_stage;  // wanted; herm_eig_tridiag takes it where the batch allows it (D&C path, n_max > TSM)
};

// `mode` is DM_TRD_TWOSTAGE or ctx->trd_mode_override: 1 forces the two-stage reduction, 0 forbids it, anything else
// leaves the choice to the measurements below.
//
// One stage: narrow panels up to n_max = 2048, wide ones above (see the panel width above).
//
// Two stages where they were measured faster than the one-stage reduction with ALL eigenvectors wanted (with a selection
// they gain more).  The bulge chase needs n / 64 sweeps in flight per matrix to be busy, so either many matrices of a few
// hundred rows or a few large ones:
//   111 x <= 1218 (configs[1]) 1.08 x, 512 x 864 1.15 x, 8 x 4000 1.17 x, 8 x 6000 1.19 x, 1 x 16384 1.03 x;
//   32 x 1200 0.89 x, 8 x 2000 0.81 x, 1 x 8192 0.75 x stay on the one-stage path.
// After the launch chains were planned once per panel: 512 x 300 1.05 x, 512 x 432 1.12 x, 256 x 600 1.14 x,
// 256 x 700 1.17 x, 512 x 864 1.19 x; 64 x 432 0.94 x, 64 x 700 0.96 x, 32 x 600 0.84 x, 16 x 1000 0.86 x.
// Round 5: the levels of the SVD preconditioner of a configs[4] slice are 23 matrices of n = 2500 .. 3552, on the
// one-stage path at 0.45 of the HBM roofline for 13 of the 44 s of that stage: n_max >= 2400 with sum n >= 48 000 joins.
// Round 6, after the chase by band position: 200 x 128 1.15 x, 300 x 64 1.04, 432 x 64 1.08, 700 x 64 1.05,
// 700 x 16 1.02, 1000 x 16 1.02, 1200 x 32 1.06, 2000 x 8 1.04, 16384 x 1 1.26; 300 x 16 0.93, 432 x 16 0.95,
// 600 x 8 0.90, 1200 x 8 0.96, 2000 x 2 0.83, 3000 x 4 0.97, 4000 x 2 0.88, 8192 x 1 0.96
// (profiles/r06e_twostage_sweep.txt).
// The batch rules apply up to n_max = 2048, where the narrow panels are the one-stage choice anyway; the size rules take
// larger batches to the two-stage reduction, and so to the 32-wide build, whatever the one-stage width would be.
trd_policy trd_policy_of(int maxn, int np, size_t totn, int mode) {
  const int width = maxn <= 2048 ? 32 : 64;
  if (mode == 1) return {32, true};
  if (mode == 0) return {width, false};
  const bool many = maxn <= 2048 && ((maxn >= 700 && np >= 16) || (maxn >= 200 && np >= 64) || (maxn >= 2000 && np >= 8) ||
                                     (maxn >= 300 && totn >= 120000));
  const bool large = (maxn >= 3500 && totn >= 24000) || (maxn >= 2400 && totn >= 48000) || maxn >= 14000;
  if (many || large) return {32, true};
  return {width, false};
}
}  // namespace

int dm_herm_eig_tridiag(dm_ctx* ctx, const std::vector<dm_jac_herm_problem>& probs, double* evals, int evals_stride,
                        dm_eig_select* sel) {
  int maxn = 0;
  size_t totn = 0;
  for (const auto& p : probs) {
    maxn = std::max(maxn, p.n);
    totn += p.n;
  }
  if (getenv("DM_TRD_SIZES")) {  // debugging aid: the batch composition
    fprintf(stderr, "[dm_herm_eig_tridiag] %zu problems, n =", probs.size());
    for (const auto& p : probs) fprintf(stderr, " %d", p.n);
    fprintf(stderr, "\n");
  }
  const char* e = getenv("DM_TRD_TWOSTAGE");
  const int mode = ctx->trd_mode_override >= 0 ? ctx->trd_mode_override : (e ? atoi(e) : -1);
  trd_policy pol = trd_policy_of(maxn, (int)probs.size(), totn, mode);
  if (const char* w = getenv("DM_TRD_PANEL")) pol.width = atoi(w) == 64 ? 64 : 32;
  return pol.width == 32 ? dm_trd32::herm_eig_tridiag(ctx, probs, evals, evals_stride, sel, pol.two_stage)
                         : dm_trd64::herm_eig_tridiag(ctx, probs, evals, evals_stride, sel, false);
}
