// dm_api.hip — extern "C" entry points of libdriftmi (see include/driftmi.h).
#include "dm_common.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <algorithm>

extern "C" {

int dm_zgemm_strided_batched(dm_ctx* ctx, int M, int N, int K, double alpha, const void* A, int rsA, int csA,
                             int conjA, int64_t strideA, const void* B, int rsB, int csB, int conjB,
                             int64_t strideB, double beta, void* C, int ldc, int64_t strideC,
                             const double* kscale, int64_t stride_kscale, int batch) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, M >= 0 && N >= 0 && K >= 0 && batch >= 0 && A && B && C);
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  const size_t mark = ws_scope__.mark;
  std::vector<dm_gemm_desc> g;
  g.reserve(batch);
  for (int b = 0; b < batch; ++b) {
    g.push_back(dm_gemm_make(reinterpret_cast<const cplx*>(A) + b * strideA, rsA, csA, conjA != 0,
                             reinterpret_cast<const cplx*>(B) + b * strideB, rsB, csB, conjB != 0,
                             reinterpret_cast<cplx*>(C) + b * strideC, ldc, M, N, K, alpha, beta,
                             kscale ? kscale + b * stride_kscale : nullptr));
  }
  int rc = dm_gemm_grouped_launch(ctx, g);
  dm_ws_release(ctx, mark);
  return rc;
}

int dm_zgemm_grouped(dm_ctx* ctx, int nprob, const dm_zgemm_problem* probs) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nprob >= 0 && (nprob == 0 || probs));
  dm_ws_scope ws_scope__(ctx);
  std::vector<dm_gemm_desc> g;
  g.reserve(nprob);
  for (int i = 0; i < nprob; ++i) {
    const dm_zgemm_problem& p = probs[i];
    DM_ARG(ctx, p.M >= 0 && p.N >= 0 && p.K >= 0);
    if (p.M == 0 || p.N == 0) continue;
    DM_ARG(ctx, p.A && p.B && p.C);
    g.push_back(dm_gemm_make(reinterpret_cast<const cplx*>(p.A), p.rsA, p.csA, p.conjA != 0, p.B, p.rsB, p.csB,
                             p.conjB != 0, reinterpret_cast<cplx*>(p.C), p.ldc, p.M, p.N, p.K, p.alpha, p.beta));
  }
  return dm_gemm_grouped_launch(ctx, g);
}

// ---- the grouped product with its whole descriptor (exposed for the parity tests) ----
static_assert(DM_ZGEMM_CONJ_A == DM_GEMM_CONJ_A && DM_ZGEMM_CONJ_B == DM_GEMM_CONJ_B && DM_ZGEMM_B_REAL == DM_GEMM_B_REAL &&
                  DM_ZGEMM_LOWER == DM_GEMM_LOWER && DM_ZGEMM_ALL_REAL == DM_GEMM_ALL_REAL &&
                  DM_ZGEMM_UPPER == DM_GEMM_UPPER && DM_ZGEMM_B_GATHER == DM_GEMM_B_GATHER &&
                  DM_ZGEMM_UPPER128 == DM_GEMM_UPPER128,
              "the public DM_ZGEMM_* flags are the planner's DM_GEMM_* flags");
static_assert(sizeof(int2) == 2 * sizeof(int), "bgather travels as pairs of int");

}  // extern "C"

namespace {

constexpr int kZgemmFlags = DM_GEMM_CONJ_A | DM_GEMM_CONJ_B | DM_GEMM_B_REAL | DM_GEMM_LOWER | DM_GEMM_ALL_REAL |
                            DM_GEMM_UPPER | DM_GEMM_B_GATHER | DM_GEMM_UPPER128;

// The problems sorted into launches (ascending `launch`, the order of the list kept inside one).  Looks at no memory
// behind the pointers.  false: a negative size, unknown flag bits, or a missing operand.
bool zgemm_ex_launches(int nprob, const dm_zgemm_problem_ex* probs, std::vector<int>& ids,
                       std::vector<std::vector<dm_gemm_desc>>& launches) {
  ids.clear();
  launches.clear();
  for (int i = 0; i < nprob; ++i) ids.push_back(probs[i].launch);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  launches.resize(ids.size());
  for (int i = 0; i < nprob; ++i) {
    const dm_zgemm_problem_ex& p = probs[i];
    if (p.M < 0 || p.N < 0 || p.K < 0 || (p.flags & ~kZgemmFlags)) return false;
    if (p.M > 0 && p.N > 0 && (!p.C || (p.K > 0 && (!p.A || !p.B)))) return false;
    dm_gemm_desc d;
    d.A = p.A; d.B = p.B; d.C = p.C; d.kscale = p.kscale;
    d.bgather = reinterpret_cast<const int2*>(p.bgather);
    d.M = p.M; d.N = p.N; d.K = p.K;
    d.rsA = p.rsA; d.csA = p.csA; d.rsB = p.rsB; d.csB = p.csB; d.ldc = p.ldc; d.csc = p.csc;
    d.flags = p.flags;
    d.alpha = p.alpha; d.beta = p.beta; d.alpha_im = p.alpha_im;
    launches[std::lower_bound(ids.begin(), ids.end(), p.launch) - ids.begin()].push_back(d);
  }
  return true;
}

}  // namespace

extern "C" {

int dm_zgemm_grouped_ex(dm_ctx* ctx, int nprob, const dm_zgemm_problem_ex* probs) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nprob >= 0 && (nprob == 0 || probs));
  std::vector<int> ids;
  std::vector<std::vector<dm_gemm_desc>> launches;
  DM_ARG(ctx, zgemm_ex_launches(nprob, probs, ids, launches));
  dm_ws_scope ws_scope__(ctx);
  if (launches.size() == 1) {
    const int rc = dm_gemm_grouped_launch(ctx, launches[0]);
    if (rc == DM_EARG) ctx->err = "bad argument: a flag combination the grouped product does not take";
    return rc;
  }
  // a chain: every plan first, one copy of all their host images, then the launches in turn
  std::vector<dm_gemm_plan> plans(launches.size());
  for (size_t l = 0; l < launches.size(); ++l) {
    const int rc = dm_gemm_plan_build(launches[l], plans[l]);
    if (rc == DM_EARG) ctx->err = "bad argument: a flag combination the grouped product does not take";
    if (rc != DM_OK) return rc;
  }
  std::vector<const dm_gemm_plan*> pp;
  for (const auto& pl : plans) pp.push_back(&pl);
  std::vector<const char*> dev;
  DM_TRY(dm_gemm_plans_upload(ctx, pp, dev));
  for (size_t l = 0; l < plans.size(); ++l) DM_TRY(dm_gemm_plan_run(ctx, plans[l], dev[l]));
  return DM_OK;
}

int dm_zgemm_plan_info(int nprob, const dm_zgemm_problem_ex* probs, int max_launch, dm_zgemm_launch_info* out,
                       int* nlaunch) {
  if (nprob < 0 || (nprob > 0 && !probs) || max_launch < 0 || (max_launch > 0 && !out) || !nlaunch) return DM_EARG;
  std::vector<int> ids;
  std::vector<std::vector<dm_gemm_desc>> launches;
  if (!zgemm_ex_launches(nprob, probs, ids, launches)) return DM_EARG;
  *nlaunch = (int)launches.size();
  for (size_t l = 0; l < launches.size(); ++l) {
    dm_gemm_plan plan;
    DM_TRY(dm_gemm_plan_build(launches[l], plan));
    if ((int)l >= max_launch) continue;  // still planned: a refused combination is reported wherever it sits
    dm_zgemm_launch_info& o = out[l];
    std::memset(&o, 0, sizeof(o));
    o.launch = ids[l];
    o.use4 = plan.use4;
    o.deep = plan.deep;
    o.wide_r = plan.wide_r;
    if (plan.blob.empty()) continue;
    const dm_gemm_tile* t = reinterpret_cast<const dm_gemm_tile*>(plan.blob.data() + plan.desc_bytes);
    const size_t cnt[4] = {plan.n0, plan.n1, plan.n2, plan.n3};
    for (int c = 0; c < 4; ++c)
      for (size_t i = 0; i < cnt[c]; ++i, ++t) {
        const dm_gemm_desc& d = launches[l][t->desc];
        // the extent of the tile as the kernel of its class cuts it
        const bool flat = t->tm < 0, wide = c == 1 && plan.wide_r;
        const int rows = flat ? 32 : 64, cols = (flat ? 128 : 64) * (wide ? 2 : 1);
        const int m0 = flat ? (-t->tm - 1) * 32 : t->tm * 64, n0 = t->tn * cols;
        const bool ragged = m0 + rows > d.M || n0 + cols > d.N || d.kscale != nullptr || c == 3;
        o.tiles[c] += 1;
        o.flat[c] += flat;
        o.cells[c][flat][ragged][d.beta != 0.0] += 1;
      }
  }
  return DM_OK;
}

int dm_zpotrf_batched(dm_ctx* ctx, int n, void* A, int ld, int64_t stride, int batch, int* info_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 0 && batch >= 0 && A && info_host);
  DM_ARG(ctx, ld >= n);  // a shorter row would put the factor outside the matrix
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  const size_t mark = ws_scope__.mark;
  std::vector<dm_mat> mats(batch);
  for (int b = 0; b < batch; ++b) mats[b] = dm_mat{reinterpret_cast<cplx*>(A) + b * stride, ld, n};
  int* info_dev = dm_ws_alloc_t<int>(ctx, batch > 0 ? batch : 1);
  if (!info_dev) return DM_ENOMEM;
  int rc = dm_potrf_batched(ctx, mats, info_dev);
  if (rc == DM_OK) rc = dm_download(ctx, info_host, info_dev, sizeof(int) * batch);
  dm_ws_release(ctx, mark);
  return rc;
}

int dm_ztrsm_left_lower_batched(dm_ctx* ctx, int n, int nrhs, const void* L, int ldl, int64_t strideL, void* B,
                                int ldb, int64_t strideB, int conjtrans, int batch) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 0 && nrhs >= 0 && batch >= 0 && L && B);
  DM_ARG(ctx, ldl >= n && ldb >= nrhs);
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  const size_t mark = ws_scope__.mark;
  std::vector<dm_trsm_problem> ps(batch);
  for (int b = 0; b < batch; ++b)
    ps[b] = dm_trsm_problem{reinterpret_cast<const cplx*>(L) + b * strideL, ldl, n,
                            reinterpret_cast<cplx*>(B) + b * strideB, ldb, nrhs};
  int rc = dm_trsm_left_lower_batched(ctx, ps, conjtrans != 0);
  dm_ws_release(ctx, mark);
  return rc;
}

// ---- Cholesky and triangular solves for a ragged list of problems (exposed for the parity tests) ----
int dm_zpotrf_problems_check(int nprob, const dm_zpotrf_problem* probs) {
  if (nprob < 0 || (nprob > 0 && !probs)) return DM_EARG;
  for (int i = 0; i < nprob; ++i) {
    const dm_zpotrf_problem& p = probs[i];
    if (p.n < 0 || p.ld < 0) return DM_EARG;
    if (p.n > 0 && (p.ld < p.n || !p.A)) return DM_EARG;
  }
  return DM_OK;
}

int dm_ztrsm_problems_check(int nprob, const dm_ztrsm_problem* probs, int conjtrans, int upper_only) {
  if (nprob < 0 || (nprob > 0 && !probs)) return DM_EARG;
  if (upper_only && conjtrans) return DM_EARG;
  for (int i = 0; i < nprob; ++i) {
    const dm_ztrsm_problem& p = probs[i];
    if (p.n < 0 || p.nrhs < 0 || p.ldl < 0 || p.ldb < 0) return DM_EARG;
    if (p.n > 0 && p.ldl < p.n) return DM_EARG;
    if (p.nrhs > 0 && p.ldb < p.nrhs) return DM_EARG;
    if (p.n > 0 && p.nrhs > 0 && (!p.L || !p.B)) return DM_EARG;
    if (upper_only && p.nrhs != p.n) return DM_EARG;
  }
  return DM_OK;
}

int dm_zpotrf_problems(dm_ctx* ctx, int nprob, const dm_zpotrf_problem* probs, int* info_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, dm_zpotrf_problems_check(nprob, probs) == DM_OK);
  DM_ARG(ctx, nprob == 0 || info_host);
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  std::vector<dm_mat> mats(nprob);
  for (int i = 0; i < nprob; ++i) mats[i] = dm_mat{reinterpret_cast<cplx*>(probs[i].A), probs[i].ld, probs[i].n};
  int* info_dev = dm_ws_alloc_t<int>(ctx, nprob > 0 ? nprob : 1);
  if (!info_dev) return DM_ENOMEM;
  DM_TRY(dm_potrf_batched(ctx, mats, info_dev));
  return dm_download(ctx, info_host, info_dev, sizeof(int) * nprob);
}

int dm_ztrsm_problems(dm_ctx* ctx, int nprob, const dm_ztrsm_problem* probs, int conjtrans, int upper_only) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, dm_ztrsm_problems_check(nprob, probs, conjtrans, upper_only) == DM_OK);
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  std::vector<dm_trsm_problem> ps(nprob);
  for (int i = 0; i < nprob; ++i)
    ps[i] = dm_trsm_problem{reinterpret_cast<const cplx*>(probs[i].L), probs[i].ldl, probs[i].n,
                            reinterpret_cast<cplx*>(probs[i].B), probs[i].ldb, probs[i].nrhs};
  return dm_trsm_left_lower_batched(ctx, ps, conjtrans != 0, upper_only != 0);
}

int dm_jacobi_rows_batched(dm_ctx* ctx, int rows, int cols, int gc0, int gc1, void* Z, int ld, int64_t stride,
                           int batch, double* sigma_dev, int* sweeps_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, rows >= 0 && cols >= 0 && gc0 >= 0 && gc1 <= cols && gc0 <= gc1 && Z && sigma_dev && batch >= 0);
  std::vector<dm_jac_problem> ps(batch);
  for (int b = 0; b < batch; ++b)
    ps[b] = dm_jac_problem{reinterpret_cast<cplx*>(Z) + b * stride, ld, 0, rows, cols, gc0, gc1};
  return dm_jacobi_rows(ctx, ps, sigma_dev, rows > 0 ? rows : 1, sweeps_host);
}

int dm_jacobi_rows_problems(dm_ctx* ctx, int nprob, const dm_jacobi_problem_desc* probs, double* sigma_dev,
                            int sigma_stride, const dm_jacobi_options* opts, int* sweeps_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nprob >= 0 && (nprob == 0 || (probs && sigma_dev)) && sigma_stride >= 0);
  std::vector<dm_jac_problem> ps(nprob);
  for (int i = 0; i < nprob; ++i) {
    const dm_jacobi_problem_desc& p = probs[i];
    DM_ARG(ctx, 0 <= p.gc0 && p.gc0 <= p.gc1 && p.gc1 <= p.ncols && p.ncols <= p.ld);
    DM_ARG(ctx, p.row0 >= 0 && p.nrows >= 0 && p.nrows <= sigma_stride && (p.nrows == 0 || p.Z));
    ps[i] = dm_jac_problem{reinterpret_cast<cplx*>(p.Z), p.ld, p.row0, p.nrows, p.ncols, p.gc0, p.gc1};
  }
  dm_jac_rows_opts o;
  if (opts) {
    DM_ARG(ctx, opts->drop_below >= 0.0 && opts->subspace_cut >= 0.0 && opts->subspace_margin >= 0.0);
    o.unconverged = opts->unconverged != 0;
    o.drop_below = opts->drop_below;
    o.one_stage_eig = opts->one_stage_eig != 0;
    o.subspace_cut = opts->subspace_cut;
    if (opts->subspace_margin > 0.0) o.subspace_margin = opts->subspace_margin;
  }
  return dm_jacobi_rows(ctx, ps, sigma_dev, sigma_stride, sweeps_host, &o);
}

int dm_jacobi_herm_batched(dm_ctx* ctx, int n, void* C, int ldc, int64_t strideC, void* W, int ldw,
                           int64_t strideW, int batch, double* evals_dev, int* sweeps_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 0 && C && W && evals_dev && batch >= 0);
  for (int b = 0; b < batch; ++b) DM_TRY(dm_set_identity(ctx, reinterpret_cast<cplx*>(W) + b * strideW, ldw, n));
  std::vector<dm_jac_herm_problem> ps(batch);
  for (int b = 0; b < batch; ++b)
    ps[b] = dm_jac_herm_problem{reinterpret_cast<cplx*>(C) + b * strideC, ldc,
                                reinterpret_cast<cplx*>(W) + b * strideW, ldw, n};
  return dm_jacobi_herm(ctx, ps, evals_dev, n > 0 ? n : 1, sweeps_host);
}

int dm_herm_eig_batched(dm_ctx* ctx, int n, void* C, int ldc, int64_t strideC, void* W, int ldw, int64_t strideW,
                        int batch, double* evals_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 0 && C && W && evals_dev && batch >= 0);
  std::vector<dm_jac_herm_problem> ps(batch);
  for (int b = 0; b < batch; ++b)
    ps[b] = dm_jac_herm_problem{reinterpret_cast<cplx*>(C) + b * strideC, ldc,
                                reinterpret_cast<cplx*>(W) + b * strideW, ldw, n};
  return dm_herm_eig_tridiag(ctx, ps, evals_dev, n > 0 ? n : 1);
}

}  // extern "C"
