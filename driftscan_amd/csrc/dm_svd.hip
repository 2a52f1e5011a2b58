// dm_svd.hip — the three-stage SVD compression of every (m, frequency) beam
// block, batched over all blocks handed in (drift/core/beamtransfer.py:802-924,
// BeamTransfer._generate_svdfile_m).
//
// The reference runs SVD1 -> project -> SVD2 (null space) -> project -> SVD3 ->
// project -> pinv, each a LAPACK call plus numpy GEMMs.  Here the whole chain is
// three phases of the one-sided block-Jacobi engine on ONE augmented matrix per
// (m, f):
//
//        Z = [ noisew * beam_m(f)  |  I_T ]        (T rows, P*L + T columns)
//
//   phase 1  rows 0..T      orthogonalised over all P*L sky columns   (SVD1, rtol 1e-10)
//   phase 2  rows 0..r1     orthogonalised over the polarised columns (SVD2, null space: rows cut2..r1)
//   phase 3  rows cut2..r1  orthogonalised over the T (pol 0) columns (SVD3, rtol 0)
//
// Because the unitary row mixing is applied to every column, after phase 3 the
// sky part of the surviving rows IS `beam = ut3 . bfr` (beamtransfer.py:877) and
// the identity part IS `ut3` (:866) — the projection GEMMs of the reference
// (:831, :850-851, :866, :877) disappear.  For unpolarised telescopes only
// phase 3 runs (:821-823).
//
// The pseudo-inverse (:887-921, scipy.linalg.pinv) is one more one-sided pass on
// [beam | I]: W beam = S V^H, so pinv(beam) = V S^-1 W = (S V^H)^H S^-2 W, a
// single grouped ZGEMM with the 1/s^2 weights on the contraction index.
#include "dm_common.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

// Per-chain geometry of the augmented matrices.  The blocks of an m carry exact zeros in the columns l < m (beam_m is
// stored with l padded from 0, beamtransfer.py:257-308): those columns add nothing to any inner product and stay zero
// under any row mixing, so a chain works on the COMPACT sky columns (p, l >= lmin) only — Lc = L - lmin per
// polarisation — and the products are scattered back into the padded layout at the end.
struct svd_geom {
  size_t zoff;   // element offset of the chain's Z (T rows x ldz)
  int lmin;      // first l kept
  int Lc;        // L - lmin
  int ldz;       // P * Lc + T
};

// Z[c] = [ nw[f] .* beam[c][:, (p, l >= lmin)] | I ]
__global__ void svd_build_z_kernel(const cplx* __restrict__ beam, const double* __restrict__ noisew,
                                   cplx* __restrict__ Z, const svd_geom* __restrict__ geo, int F, int T, int P, int L) {
  const int c = blockIdx.z;        // chain = blk * F + f
  const int f = c % F;
  const svd_geom g = geo[c];
  const int row = blockIdx.y;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= g.ldz) return;
  const int PLc = P * g.Lc;
  cplx v;
  if (col < PLc) {
    const int p = col / g.Lc, l = g.lmin + (col - p * g.Lc);
    const double w = noisew[(size_t)f * T + row];
    cplx b = beam[((size_t)c * T + row) * ((size_t)P * L) + (size_t)p * L + l];
    v = make_double2(b.x * w, b.y * w);
  } else {
    v = make_double2((col - PLc) == row ? 1.0 : 0.0, 0.0);
  }
  Z[g.zoff + (size_t)row * g.ldz + col] = v;
}

// scatter the surviving rows into the (zero-initialised) output products
__global__ void svd_extract_kernel(const cplx* __restrict__ Z, const svd_geom* __restrict__ geo,
                                   const int* __restrict__ row0, const int* __restrict__ nmodes,
                                   const double* __restrict__ noisew, const double* __restrict__ sig3,
                                   cplx* __restrict__ beam_svd, cplx* __restrict__ beam_ut, double* __restrict__ sigma,
                                   int F, int T, int P, int L, int K) {
  const int c = blockIdx.z;
  const int f = c % F;
  const int i = blockIdx.y;  // mode index
  if (i >= nmodes[c]) return;
  const svd_geom g = geo[c];
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int PLc = P * g.Lc;
  const cplx* z = Z + g.zoff + (size_t)(row0[c] + i) * g.ldz;
  if (col < PLc) {
    const int p = col / g.Lc, l = g.lmin + (col - p * g.Lc);   // the columns l < lmin of the (zero-filled) output stay zero
    beam_svd[((size_t)c * K + i) * ((size_t)P * L) + (size_t)p * L + l] = z[col];
  } else if (col < PLc + T) {
    const int t = col - PLc;
    const double w = noisew[(size_t)f * T + t];
    cplx u = z[col];
    beam_ut[((size_t)c * K + i) * T + t] = make_double2(u.x * w, u.y * w);
  }
  if (col == 0) sigma[(size_t)c * K + i] = sig3[(size_t)c * T + i];
}

// TALL chains (P (L - lmin) < T: more rows than sky columns — every m-block above m = L - T / P), SVD1: the T x T Gram
// eigenproblem of the row-side preconditioner has rank <= P Lc, and rounds 1-4 paid for all of it (864^3 against 452^3 at
// m = 400 of configs[2]).  The same singular triplets come out of the TRANSPOSED matrix: Yt = (w B)^H is P Lc x T, its
// rows are mixed until orthogonal over all T columns — Yt' = Sigma U^H: row i is sigma_i u_i^H — and the rows of the
// chain's Z follow as  [ u_i^H (w B) | u_i^H ]  (one product per polarisation); only r1 <= P Lc rows ever exist.
// Yt[c][k = p Lc + j][t] = conj( nw[f][t] beam[c][t][p][lmin + j] ), through a 32 x 32 LDS tile (both sides coalesced)
__global__ __launch_bounds__(256) void svd_build_yt_kernel(const cplx* __restrict__ beam, const double* __restrict__ noisew,
                                                           cplx* __restrict__ Yt, const svd_geom* __restrict__ geo,
                                                           const size_t* __restrict__ yoff, const int* __restrict__ tall,
                                                           int F, int T, int P, int L) {
  __shared__ cplx tile[32][33];
  const int c = blockIdx.z;
  if (!tall[c]) return;
  const svd_geom g = geo[c];
  const int f = c % F;
  const int Kc = P * g.Lc;
  const int k0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
  if (k0 >= Kc || t0 >= T) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int t = t0 + j, k = k0 + tx;
    cplx v = make_double2(0.0, 0.0);
    if (t < T && k < Kc) {
      const int p = k / g.Lc, l = g.lmin + (k - p * g.Lc);
      const double w = noisew[(size_t)f * T + t];
      const cplx b = beam[((size_t)c * T + t) * ((size_t)P * L) + (size_t)p * L + l];
      v = make_double2(b.x * w, -b.y * w);
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int k = k0 + j, t = t0 + tx;
    if (k < Kc && t < T) Yt[yoff[c] + (size_t)k * T + t] = tile[tx][j];
  }
}

// identity part of the rows of a tall chain: Z[c][i][P Lc + t] = Yt'[c][i][t] / sigma_i = u_i^H   (i < r1)
__global__ void svd_tall_rows_kernel(const cplx* __restrict__ Yt, const size_t* __restrict__ yoff,
                                     const int* __restrict__ tall, const int* __restrict__ r1,
                                     const double* __restrict__ sigt, cplx* __restrict__ Z,
                                     const svd_geom* __restrict__ geo, int T, int P) {
  const int c = blockIdx.z;
  if (!tall[c]) return;
  const int i = blockIdx.y;
  if (i >= r1[c]) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const svd_geom g = geo[c];
  const double s = sigt[(size_t)c * T + i];
  const double inv = s > 0.0 ? 1.0 / s : 0.0;
  const cplx y = Yt[yoff[c] + (size_t)i * T + t];
  Z[g.zoff + (size_t)i * g.ldz + (size_t)P * g.Lc + t] = make_double2(y.x * inv, y.y * inv);
}

// unpolarised tall chains (SVD3 through the transposed matrix): rows of Yt' = Sigma U^H -> u_i^H in place, beam_ut, sigma
__global__ void svd_tall3_products_kernel(cplx* __restrict__ Yt, const size_t* __restrict__ yoff,
                                          const int* __restrict__ tall, const int* __restrict__ nmodes,
                                          const double* __restrict__ sigt, const double* __restrict__ noisew,
                                          cplx* __restrict__ beam_ut, double* __restrict__ sigma, int F, int T, int K) {
  const int c = blockIdx.z;
  if (!tall[c]) return;
  const int i = blockIdx.y;
  if (i >= nmodes[c]) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int f = c % F;
  const double s = sigt[(size_t)c * T + i];
  const double inv = s > 0.0 ? 1.0 / s : 0.0;
  cplx y = Yt[yoff[c] + (size_t)i * T + t];
  y = make_double2(y.x * inv, y.y * inv);
  Yt[yoff[c] + (size_t)i * T + t] = y;
  const double w = noisew[(size_t)f * T + t];
  beam_ut[((size_t)c * K + i) * T + t] = make_double2(y.x * w, y.y * w);
  if (t == 0) sigma[(size_t)c * K + i] = s;
}

// Polarised telescopes, round 5: SVD3 runs on a matrix of its own, Z3[c] = [ U^H (w B_T) | U^H ] — the rows cut2 .. r1 of
// the accumulated row mixing (the identity part of Z after SVD2) and their total-intensity columns, recomputed from the
// input block by one product — instead of dragging the 3 (L - lmin) polarised passenger columns through every level
// product and rotation of the phase; the polarised part of `beam` is one product at the end, `ut3 . bfr` as the
// reference writes it (beamtransfer.py:877).  geo3: r3 rows x (Lc + T) columns per chain.
__global__ void svd_build_z3_kernel(const cplx* __restrict__ Z, const svd_geom* __restrict__ geo,
                                    const svd_geom* __restrict__ geo3, const int* __restrict__ row0,
                                    const int* __restrict__ nrow3, cplx* __restrict__ Z3, int T, int P) {
  const int c = blockIdx.z;
  const int i = blockIdx.y;
  if (i >= nrow3[c]) return;
  const svd_geom g = geo[c], g3 = geo3[c];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  Z3[g3.zoff + (size_t)i * g3.ldz + g.Lc + t] = Z[g.zoff + (size_t)(row0[c] + i) * g.ldz + (size_t)P * g.Lc + t];
}

// products of a polarised chain from Z3 (rows sorted by descending sigma): total-intensity part of beam_svd, beam_ut, sigma
__global__ void svd_extract3_kernel(const cplx* __restrict__ Z3, const svd_geom* __restrict__ geo3,
                                    const int* __restrict__ nmodes, const double* __restrict__ noisew,
                                    const double* __restrict__ sig3, cplx* __restrict__ beam_svd,
                                    cplx* __restrict__ beam_ut, double* __restrict__ sigma, int F, int T, int P, int L,
                                    int K) {
  const int c = blockIdx.z;
  const int f = c % F;
  const int i = blockIdx.y;
  if (i >= nmodes[c]) return;
  const svd_geom g = geo3[c];
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const cplx* z = Z3 + g.zoff + (size_t)i * g.ldz;
  if (col < g.Lc) {
    beam_svd[((size_t)c * K + i) * ((size_t)P * L) + g.lmin + col] = z[col];
  } else if (col < g.Lc + T) {
    const int t = col - g.Lc;
    const double w = noisew[(size_t)f * T + t];
    const cplx u = z[col];
    beam_ut[((size_t)c * K + i) * T + t] = make_double2(u.x * w, u.y * w);
  }
  if (col == 0) sigma[(size_t)c * K + i] = sig3[(size_t)c * T + i];
}

// Z2[c] = [ beam_svd[c][:nm][:, (p, l >= lmin)] | I_nm ]   (geo2: K rows allocated per chain, ld2 = P * Lc + K)
__global__ void svd_build_pinv_kernel(const cplx* __restrict__ beam_svd, const int* __restrict__ nmodes,
                                      cplx* __restrict__ Z2, const svd_geom* __restrict__ geo2, int K, int P, int L) {
  const int c = blockIdx.z;
  const int i = blockIdx.y;
  if (i >= nmodes[c]) return;
  const svd_geom g = geo2[c];
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= g.ldz) return;
  const int PLc = P * g.Lc;
  cplx v;
  if (col < PLc) {
    const int p = col / g.Lc, l = g.lmin + (col - p * g.Lc);
    v = beam_svd[((size_t)c * K + i) * ((size_t)P * L) + (size_t)p * L + l];
  } else {
    v = make_double2((col - PLc) == i ? 1.0 : 0.0, 0.0);
  }
  Z2[g.zoff + (size_t)i * g.ldz + col] = v;
}

// w[c][i] = 1/s^2 if s > rtol * s_max else 0   (scipy.linalg.pinv: rtol = max(M,N) eps)
__global__ void svd_pinv_weights_kernel(const double* __restrict__ s4, const int* __restrict__ nmodes,
                                        double* __restrict__ w, int K, double rtol) {
  const int c = blockIdx.x;
  const int nm = nmodes[c];
  const double smax = nm > 0 ? s4[(size_t)c * K] : 0.0;  // sorted descending
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    double s = i < nm ? s4[(size_t)c * K + i] : 0.0;
    w[(size_t)c * K + i] = (i < nm && s > rtol * smax && s > 0.0) ? 1.0 / (s * s) : 0.0;
  }
}

// A chain is TALL, and goes through the transposed matrix, when it has at most this share of sky columns per row: P Lc <=
// 95 % of T (m = 320 of configs[2], P Lc = 0.89 T: 2.01 -> 1.64 s per 11 blocks; at P Lc = T even)
constexpr int SVD_TALL_PCT = 95;

// what the caller asked for
struct svd_args {
  int nblk, F, T, P, L;
  const int* lmin_host;
  const cplx* beam; const double* noisew; double polsvcut;
  cplx *beam_svd, *ibeam, *beam_ut; double* sigma; int *nmodes_host, *sweeps_host;
  int nch, PL, K;   // chains (blk * F + f), P * L, min(L, T)
};

// the switches of a call, read per call: the tests flip them
struct svd_routes {
  bool compact, narrow, tall, subspace, debug;
  explicit svd_routes(int P) {
    auto on = [](const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; };
    compact = getenv("DM_SVD_NO_COMPACT") == nullptr;   // the chains work on the columns l >= lmin only
    narrow = on("DM_SVD_NARROW") && P > 1;   // =0: SVD2 / SVD3 on all columns of Z (the passengers of a phase ride through it)
    // =0: all chains as they lie, none through the transposed matrix.  P == 1 reads it once per process: the untransposed
    // SVD3 counts the rounding residues of a rank-deficient block in `nmodes` (the static is set by the first P == 1 call)
    auto once = [&] { static const bool v = on("DM_SVD_TALL"); return v; };
    tall = P == 1 ? once() : on("DM_SVD_TALL");
    subspace = on("DM_SVD_SUBSPACE");        // =0: SVD1 and SVD2 converge as SVDs instead of handing on a subspace
    debug = getenv("DM_DEBUG") != nullptr;   // a line per phase on stderr
  }
};

// the chains of one phase that run on the transposed matrix Yt = (w B)^H (P Lc x T): SVD1 of a polarised telescope, SVD3 of
// an unpolarised one
struct svd_tall {
  std::vector<int> on;        // per chain
  std::vector<size_t> yoff;   // element offset of the chain's Yt
  size_t ytot = 0;
  int n = 0, kc_max = 0;      // chains on this route; their largest P Lc
  cplx* Yt{}; double* sigt{};   // sigt: row norms of Yt' = Sigma U^H, T per chain
  int* d_on{}; size_t* d_yoff{};
};

// what the stages of dm_svd_chain_lmin share
struct svd_ws {
  svd_routes rt;
  std::vector<svd_geom> geo, geo3;    // geo3, Z3: the narrow route's matrix of SVD3, r3 rows x (Lc + T) columns per chain
  svd_geom *d_geo{}, *d_geo3{}; size_t ztot = 0; int ldz_max = 0;
  cplx *Z{}, *Z3{};
  double* sig{};                      // row norms of the phase in flight, T per chain
  std::vector<double> hs;             // ... on the host
  std::vector<int> r1, cut2, alive;   // rows kept by SVD1; rows above SVD2's cut; the reference's `(s1 > 0.0).any()`
  std::vector<int> row0, nrow3;       // the rows SVD3 works on
  svd_tall tall1, tall3;
  std::vector<int> nmodes; int* d_nm{}; int maxnm = 0, sw = 0;
  svd_ws(const svd_routes& r, int nch, int T)
      : rt(r), hs((size_t)nch * T), r1(nch, T), cut2(nch, 0), alive(nch, 1), row0(nch), nrow3(nch), nmodes(nch, 0) {}
};

// rows of U^H (nrows x T, leading dimension ldu) times the noise-weighted slice of the input block of chain c — polarisation
// pp, columns l >= lmin — into `out`
dm_gemm_desc svd_ut_wb(const svd_args& a, const svd_ws& w, int c, int pp, const cplx* u, int ldu, cplx* out, int ldo, int nrows) {
  const svd_geom& g = w.geo[c];
  return dm_gemm_make(u, ldu, 1, false, a.beam + (size_t)c * a.T * a.PL + (size_t)pp * a.L + g.lmin, a.PL, 1, false, out, ldo,
                      nrows, g.Lc, a.T, 1.0, 0.0, a.noisew + (size_t)(c % a.F) * a.T);
}

// ---- stage: geometry.  Chain c = blk * F + f works on the columns l >= lmin[blk] of every polarisation
void svd_geometry(const svd_args& a, svd_ws& w) {
  w.geo.resize(a.nch);
  for (int c = 0; c < a.nch; ++c) {
    const int lm = (a.lmin_host && w.rt.compact) ? a.lmin_host[c / a.F] : 0;
    w.geo[c] = svd_geom{w.ztot, lm, a.L - lm, a.P * (a.L - lm) + a.T};
    w.ztot += (size_t)a.T * w.geo[c].ldz;
    w.ldz_max = std::max(w.ldz_max, w.geo[c].ldz);
  }
}

// ---- stage: Z = [ noisew * beam | I ] of every chain
int svd_build_z(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  w.Z = dm_ws_alloc_t<cplx>(ctx, w.ztot);
  w.sig = dm_ws_alloc_t<double>(ctx, (size_t)a.nch * a.T);
  w.d_geo = dm_ws_upload(ctx, w.geo);
  if (!w.Z || !w.sig || !w.d_geo) return DM_ENOMEM;
  DM_SVD_LAUNCH(ctx, svd_build_z_kernel, dim3((w.ldz_max + 255) / 256, a.T, a.nch), a.beam, a.noisew, w.Z, w.d_geo, a.F, a.T, a.P, a.L);
  return DM_OK;
}

// one Jacobi phase on the chains as they lie: row norms into w.sig and w.hs, sweeps into slot `phase` of the caller's array
int svd_rows_pass(dm_ctx* ctx, const svd_args& a, svd_ws& w, const std::vector<dm_jac_problem>& pr, const dm_jac_rows_opts& o, int phase) {
  DM_TRY(dm_jacobi_rows(ctx, pr, w.sig, a.T, &w.sw, &o));   // (no work, no launch, when every chain is on the transposed route)
  if (a.sweeps_host) a.sweeps_host[phase] = w.sw;
  return dm_download(ctx, w.hs.data(), w.sig, sizeof(double) * w.hs.size());
}

// ---- the transposed route, in three steps: which chains take it (the 95 % rule, none unless `enabled`) and where their Yt lies; ...
void svd_tall_classify(const svd_args& a, const svd_ws& w, svd_tall& t, bool enabled) {
  t.on.assign(a.nch, 0);
  t.yoff.assign(a.nch, 0);
  for (int c = 0; c < a.nch; ++c) {
    const int Kc = a.P * w.geo[c].Lc;
    t.on[c] = (enabled && Kc * 100 <= a.T * SVD_TALL_PCT) ? 1 : 0;
    if (t.on[c]) { t.yoff[c] = t.ytot; t.ytot += (size_t)Kc * a.T; ++t.n; t.kc_max = std::max(t.kc_max, Kc); }
  }
}

// ... Yt out of the input blocks; ...
int svd_tall_build(dm_ctx* ctx, const svd_args& a, const svd_ws& w, svd_tall& t) {
  if (t.n == 0) return DM_OK;
  t.Yt = dm_ws_alloc_t<cplx>(ctx, t.ytot);
  t.sigt = dm_ws_alloc_t<double>(ctx, (size_t)a.nch * a.T);
  t.d_on = dm_ws_upload(ctx, t.on);
  t.d_yoff = dm_ws_upload(ctx, t.yoff);
  if (!t.Yt || !t.sigt || !t.d_on || !t.d_yoff) return DM_ENOMEM;
  DM_TRY(dm_fill_zero(ctx, t.sigt, sizeof(double) * (size_t)a.nch * a.T));
  DM_SVD_LAUNCH(ctx, svd_build_yt_kernel, dim3((t.kc_max + 31) / 32, (a.T + 31) / 32, a.nch), a.beam, a.noisew, t.Yt, w.d_geo, t.d_yoff,
                t.d_on, a.F, a.T, a.P, a.L);
  return DM_OK;
}

// ... its rows orthogonalised over all T columns (Yt' = Sigma U^H), and the first P Lc row norms of each chain merged into w.hs
int svd_tall_pass(dm_ctx* ctx, const svd_args& a, svd_ws& w, const svd_tall& t, const dm_jac_rows_opts& o, int phase) {
  if (t.n == 0) return DM_OK;
  std::vector<dm_jac_problem> pt(a.nch);
  for (int c = 0; c < a.nch; ++c) pt[c] = dm_jac_problem{t.Yt + t.yoff[c], a.T, 0, t.on[c] ? a.P * w.geo[c].Lc : 0, a.T, 0, a.T};
  int swt = 0;
  DM_TRY(dm_jacobi_rows(ctx, pt, t.sigt, a.T, &swt, &o));
  w.sw = std::max(w.sw, swt);
  if (a.sweeps_host) a.sweeps_host[phase] = w.sw;
  std::vector<double> hst((size_t)a.nch * a.T);
  DM_TRY(dm_download(ctx, hst.data(), t.sigt, sizeof(double) * hst.size()));
  for (int c = 0; c < a.nch; ++c)
    for (int i = 0; t.on[c] && i < a.T; ++i) w.hs[(size_t)c * a.T + i] = i < a.P * w.geo[c].Lc ? hst[(size_t)c * a.T + i] : 0.0;
  return DM_OK;
}

// rows of the tall chains after SVD1: [ u_i^H (w B) | u_i^H ], i < r1
int svd_tall_rows(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  const svd_tall& t = w.tall1;
  int maxr1 = 0;
  for (int c = 0; c < a.nch; ++c) if (t.on[c]) maxr1 = std::max(maxr1, w.r1[c]);
  int* d_r1 = dm_ws_upload(ctx, w.r1);
  if (!d_r1) return DM_ENOMEM;
  if (maxr1 == 0) return DM_OK;
  DM_SVD_LAUNCH(ctx, svd_tall_rows_kernel, dim3((a.T + 255) / 256, maxr1, a.nch), t.Yt, t.d_yoff, t.d_on, d_r1, t.sigt, w.Z, w.d_geo, a.T,
                a.P);
  std::vector<dm_gemm_desc> g;
  g.reserve((size_t)t.n * a.P);
  for (int c = 0; c < a.nch; ++c) {
    if (!t.on[c] || w.r1[c] == 0) continue;
    cplx* z = w.Z + w.geo[c].zoff;
    const cplx* u = z + (size_t)a.P * w.geo[c].Lc;
    for (int pp = 0; pp < a.P; ++pp)
      g.push_back(svd_ut_wb(a, w, c, pp, u, w.geo[c].ldz, z + (size_t)pp * w.geo[c].Lc, w.geo[c].ldz, w.r1[c]));
  }
  return dm_gemm_grouped_launch(ctx, g);
}

// ---- stage: SVD1, image with rtol 1e-10 (beamtransfer.py:826, :98); tall chains through the transposed matrix
int svd_phase1(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  svd_tall& t = w.tall1;
  svd_tall_classify(a, w, t, w.rt.tall);
  std::vector<dm_jac_problem> pr(a.nch);
  for (int c = 0; c < a.nch; ++c)
    pr[c] = dm_jac_problem{w.Z + w.geo[c].zoff, w.geo[c].ldz, 0, t.on[c] ? 0 : a.T, w.geo[c].ldz, 0, a.P * w.geo[c].Lc};
  // SVD1 keeps s > 1e-10 s_0 (beamtransfer.py:826): rows two decades further down are left out of the sweeps
  dm_jac_rows_opts o1;
  o1.unconverged = true;
  o1.drop_below = 1e-12;
  // SVD1 hands its IMAGE to SVD2 (the rows above the cut, as a subspace): DM_SVD_SUBSPACE=0 converges it as an SVD
  if (w.rt.subspace) o1.subspace_cut = 1e-10;
  DM_TRY(svd_rows_pass(ctx, a, w, pr, o1, 0));
  // The Gram matrices of the transposed problems have exactly zero rows and columns (sky columns beyond a frequency's band
  // limit) — what exposed the underflow in the Householder scalars of the band chase (DM_REFL_TINY, dm_kernels.h).
  // Both reductions are right now; the one-stage one is as fast at n ~ 450 (2.64 against 2.63 s on 14 blocks at
  // m = 300) and stays the choice of this call.
  dm_jac_rows_opts ot = o1;
  ot.subspace_cut = 0.0;   // the rows of Yt become sigma_i u_i^H only when they are ORTHOGONAL: a converged SVD, not a split
  ot.one_stage_eig = true;
  DM_TRY(svd_tall_build(ctx, a, w, t));
  DM_TRY(svd_tall_pass(ctx, a, w, t, ot, 0));
  for (int c = 0; c < a.nch; ++c) {
    const double* s = &w.hs[(size_t)c * a.T];
    w.r1[c] = (int)std::count_if(s, s + a.T, [s](double x) { return x > s[0] * 1e-10; });
    w.alive[c] = (s[0] > 0.0) ? 1 : 0;   // the reference's guard `(s1 > 0.0).any()` (beamtransfer.py:855-857)
  }
  if (t.n > 0) DM_TRY(svd_tall_rows(ctx, a, w));
  if (w.rt.debug) {
    // decades of the SVD1 spectrum of the first chain, and the rank range over the batch
    const double* s = &w.hs[0];
    int dec[20] = {0};
    for (int i = 0; i < a.T; ++i) {
      const double r = s[i] > 0.0 ? -std::log10(s[i] / s[0]) : 19.0;
      dec[std::min(19, std::max(0, (int)r))]++;
    }
    fprintf(stderr, "[svd_chain] SVD1 sweeps %d, r1 %d..%d, chain 0 per-decade counts:", w.sw,
            *std::min_element(w.r1.begin(), w.r1.end()), *std::max_element(w.r1.begin(), w.r1.end()));
    for (int d = 0; d < 20; ++d) fprintf(stderr, " %d", dec[d]);
    fprintf(stderr, "\n");
  }
  return DM_OK;
}

// ---- stage: SVD2, left null space of the polarised columns, `>=` cut (:844-848, :137)
// (narrow: the phase works on the columns [pol | I] — the view starts behind the total-intensity block, which is
// stale from here on and rebuilt for SVD3 from the identity part)
int svd_phase2(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  std::vector<dm_jac_problem> pr(a.nch);
  for (int c = 0; c < a.nch; ++c) {
    const svd_geom& g = w.geo[c];
    pr[c] = w.rt.narrow ? dm_jac_problem{w.Z + g.zoff + g.Lc, g.ldz, 0, w.r1[c], g.ldz - g.Lc, 0, (a.P - 1) * g.Lc}
                     : dm_jac_problem{w.Z + g.zoff, g.ldz, 0, w.r1[c], g.ldz, g.Lc, a.P * g.Lc};
  }
  dm_jac_rows_opts o2;
  o2.unconverged = true;
  if (w.rt.subspace && a.polsvcut > 0.0 && a.polsvcut <= 1e-3) {   // SVD2 hands its null space (the rows below the cut) to SVD3
    o2.subspace_cut = a.polsvcut;
    o2.subspace_margin = 100.0;
  }
  DM_TRY(svd_rows_pass(ctx, a, w, pr, o2, 1));
  for (int c = 0; c < a.nch; ++c) {
    const double* s = &w.hs[(size_t)c * a.T];
    w.cut2[c] = (int)std::count_if(s, s + w.r1[c], [&](double x) { return x >= s[0] * a.polsvcut; });
  }
  if (w.rt.debug)
    fprintf(stderr, "[svd_chain] SVD2 sweeps %d, cut2 %d..%d\n", w.sw, *std::min_element(w.cut2.begin(), w.cut2.end()),
            *std::max_element(w.cut2.begin(), w.cut2.end()));
  return DM_OK;
}

// Z3 of the narrow route: the identity part out of Z, the total-intensity part U^H diag(noisew) B_T by one product per chain
// out of the input block; `pr` then points at Z3
int svd_build_z3(dm_ctx* ctx, const svd_args& a, svd_ws& w, std::vector<dm_jac_problem>& pr) {
  w.geo3.resize(a.nch);
  size_t z3tot = 0;
  int maxr3 = 0;
  for (int c = 0; c < a.nch; ++c) {
    w.geo3[c] = svd_geom{z3tot, w.geo[c].lmin, w.geo[c].Lc, w.geo[c].Lc + a.T};
    z3tot += (size_t)w.nrow3[c] * w.geo3[c].ldz;
    maxr3 = std::max(maxr3, w.nrow3[c]);
  }
  w.Z3 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(z3tot, 1));
  w.d_geo3 = dm_ws_upload(ctx, w.geo3);
  int* d_r0 = dm_ws_upload(ctx, w.row0);
  int* d_n3 = dm_ws_upload(ctx, w.nrow3);
  if (!w.Z3 || !w.d_geo3 || !d_r0 || !d_n3) return DM_ENOMEM;
  if (maxr3 > 0) {
    DM_SVD_LAUNCH(ctx, svd_build_z3_kernel, dim3((a.T + 255) / 256, maxr3, a.nch), w.Z, w.d_geo, w.d_geo3, d_r0, d_n3, w.Z3, a.T, a.P);
    std::vector<dm_gemm_desc> g;
    g.reserve(a.nch);
    for (int c = 0; c < a.nch; ++c) {
      if (w.nrow3[c] == 0) continue;
      cplx* z3 = w.Z3 + w.geo3[c].zoff;
      g.push_back(svd_ut_wb(a, w, c, 0, z3 + w.geo[c].Lc, w.geo3[c].ldz, z3, w.geo3[c].ldz, w.nrow3[c]));
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
  }
  for (int c = 0; c < a.nch; ++c)
    pr[c] = dm_jac_problem{w.Z3 + w.geo3[c].zoff, w.geo3[c].ldz, 0, w.nrow3[c], w.geo3[c].ldz, 0, w.geo[c].Lc};
  return DM_OK;
}

// ---- stage: SVD3 on the total-intensity columns, rtol 0 (:859-865), then the mode counts
int svd_phase3(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  svd_tall& t = w.tall3;
  std::vector<dm_jac_problem> pr(a.nch);
  for (int c = 0; c < a.nch; ++c) {
    w.row0[c] = w.cut2[c];
    w.nrow3[c] = w.alive[c] ? std::max(0, w.r1[c] - w.cut2[c]) : 0;
    pr[c] = dm_jac_problem{w.Z + w.geo[c].zoff, w.geo[c].ldz, w.row0[c], w.nrow3[c], w.geo[c].ldz, 0, w.geo[c].Lc};
  }
  if (w.rt.narrow) DM_TRY(svd_build_z3(ctx, a, w, pr));
  // Unpolarised telescopes: SVD3 is the whole chain, and a block with Lc <= 0.95 T sky columns goes through the
  // transposed matrix Yt = (w B)^H (Lc x T) — Lc rows to orthogonalise instead of T (configs[1]: T = 92, Lc = 129 - m)
  svd_tall_classify(a, w, t, w.rt.tall && a.P == 1);
  for (int c = 0; c < a.nch; ++c) if (t.on[c]) pr[c].nrows = 0;
  DM_TRY(svd_tall_build(ctx, a, w, t));
  // polarised: certainly not orthogonal yet.  Unpolarised: the measuring pass is kept, it retires the
  // all-zero and trivially orthogonal blocks of the high m (a fifth of config 2) before the eigensolver.
  dm_jac_rows_opts o3;
  o3.unconverged = a.P > 1;
  DM_TRY(svd_rows_pass(ctx, a, w, pr, o3, 2));
  DM_TRY(svd_tall_pass(ctx, a, w, t, o3, 2));
  for (int c = 0; c < a.nch; ++c) {
    const double* s = &w.hs[(size_t)c * a.T];
    const int lim = std::min(t.on[c] ? w.geo[c].Lc : w.nrow3[c], a.K);
    w.nmodes[c] = a.nmodes_host[c] = (int)std::count_if(s, s + lim, [](double x) { return x > 0.0; });  // rtol = 0.0: strictly positive
    w.maxnm = std::max(w.maxnm, w.nmodes[c]);
  }
  if (w.rt.debug)
    fprintf(stderr, "[svd_chain] SVD3 sweeps %d, nmodes %d..%d\n", w.sw, *std::min_element(w.nmodes.begin(), w.nmodes.end()), w.maxnm);
  return DM_OK;
}

// ---- stage: the products beam_svd, beam_ut, sigma (zero past nmodes)
int svd_products(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  const int nch = a.nch, F = a.F, T = a.T, P = a.P, L = a.L, K = a.K, PL = a.PL, maxnm = w.maxnm;
  const svd_tall& t = w.tall3;
  int* d_row0 = dm_ws_upload(ctx, w.row0);
  w.d_nm = dm_ws_upload(ctx, w.nmodes);
  if (!d_row0 || !w.d_nm) return DM_ENOMEM;
  DM_TRY(dm_fill_zero(ctx, a.beam_svd, sizeof(cplx) * (size_t)nch * K * PL));
  DM_TRY(dm_fill_zero(ctx, a.beam_ut, sizeof(cplx) * (size_t)nch * K * T));
  DM_TRY(dm_fill_zero(ctx, a.sigma, sizeof(double) * (size_t)nch * K));
  if (maxnm > 0 && !w.rt.narrow) {
    const int* d_nm_z = w.d_nm;
    if (t.n > 0) {   // the rows of those chains are not in Z
      std::vector<int> nmz(w.nmodes);
      for (int c = 0; c < nch; ++c) if (t.on[c]) nmz[c] = 0;
      d_nm_z = dm_ws_upload(ctx, nmz);
      if (!d_nm_z) return DM_ENOMEM;
    }
    DM_SVD_LAUNCH(ctx, svd_extract_kernel, dim3((w.ldz_max + 255) / 256, maxnm, nch), w.Z, w.d_geo, d_row0, d_nm_z, a.noisew, w.sig,
                  a.beam_svd, a.beam_ut, a.sigma, F, T, P, L, K);
    if (t.n > 0) {
      // u_i^H = Yt'[i] / sigma_i (in place), beam_ut = u_i^H diag(noisew), sigma; beam = u_i^H (w B): one product per chain
      DM_SVD_LAUNCH(ctx, svd_tall3_products_kernel, dim3((T + 255) / 256, maxnm, nch), t.Yt, t.d_yoff, t.d_on, w.d_nm, t.sigt, a.noisew,
                    a.beam_ut, a.sigma, F, T, K);
      std::vector<dm_gemm_desc> g;
      g.reserve(t.n);
      for (int c = 0; c < nch; ++c) {
        if (!t.on[c] || w.nmodes[c] == 0) continue;
        g.push_back(svd_ut_wb(a, w, c, 0, t.Yt + t.yoff[c], T, a.beam_svd + (size_t)c * K * PL + w.geo[c].lmin, PL, w.nmodes[c]));
      }
      DM_TRY(dm_gemm_grouped_launch(ctx, g));
    }
  }
  if (maxnm > 0 && w.rt.narrow) {
    DM_SVD_LAUNCH(ctx, svd_extract3_kernel, dim3((L + T + 255) / 256, maxnm, nch), w.Z3, w.d_geo3, w.d_nm, a.noisew, w.sig, a.beam_svd,
                  a.beam_ut, a.sigma, F, T, P, L, K);
    // the polarised part of `beam = ut3 . bfr` (beamtransfer.py:877): rows of U^H (the identity part of Z3) times the
    // noise-weighted input block, one product per polarisation into the columns l >= lmin of the (zero-filled) output
    std::vector<dm_gemm_desc> g;
    g.reserve((size_t)nch * (P - 1));
    for (int c = 0; c < nch; ++c) {
      const int nm = w.nmodes[c];
      if (nm == 0) continue;
      const cplx* u = w.Z3 + w.geo3[c].zoff + w.geo[c].Lc;
      for (int pp = 1; pp < P; ++pp)
        g.push_back(svd_ut_wb(a, w, c, pp, u, w.geo3[c].ldz, a.beam_svd + (size_t)c * K * PL + (size_t)pp * L + w.geo[c].lmin, PL, nm));
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
  }
  return DM_OK;
}

// ---- stage: pseudo-inverse of `beam` (:887-921)
int svd_pinv(dm_ctx* ctx, const svd_args& a, svd_ws& w) {
  const int nch = a.nch, P = a.P, L = a.L, K = a.K, PL = a.PL, maxnm = w.maxnm;
  DM_TRY(dm_fill_zero(ctx, a.ibeam, sizeof(cplx) * (size_t)nch * PL * K));
  if (maxnm == 0) return DM_OK;
  // [beam | I] per chain: K rows of P * Lc + K columns
  std::vector<svd_geom> geo2(nch);
  size_t z2tot = 0;
  int ld2_max = 0;
  for (int c = 0; c < nch; ++c) {
    geo2[c] = svd_geom{z2tot, w.geo[c].lmin, w.geo[c].Lc, P * w.geo[c].Lc + K};
    z2tot += (size_t)K * geo2[c].ldz;
    ld2_max = std::max(ld2_max, geo2[c].ldz);
  }
  // Z is no longer needed: reuse its storage when it is large enough
  cplx* Z2 = (z2tot <= w.ztot) ? w.Z : dm_ws_alloc_t<cplx>(ctx, z2tot);
  double* s4 = dm_ws_alloc_t<double>(ctx, (size_t)nch * K);
  double* w4 = dm_ws_alloc_t<double>(ctx, (size_t)nch * K);
  svd_geom* d_geo2 = dm_ws_upload(ctx, geo2);
  if (!Z2 || !s4 || !w4 || !d_geo2) return DM_ENOMEM;
  DM_SVD_LAUNCH(ctx, svd_build_pinv_kernel, dim3((ld2_max + 255) / 256, maxnm, nch), a.beam_svd, w.d_nm, Z2, d_geo2, K, P, L);
  std::vector<dm_jac_problem> pr(nch);
  for (int c = 0; c < nch; ++c)
    pr[c] = dm_jac_problem{Z2 + geo2[c].zoff, geo2[c].ldz, 0, w.nmodes[c], P * w.geo[c].Lc + w.nmodes[c], 0, P * w.geo[c].Lc};
  // unpolarised: these are exactly the rows SVD3 left orthogonal over the same columns (the measuring pass
  // sees that and skips everything); polarised: orthogonal over the T columns only
  dm_jac_rows_opts o4;
  o4.unconverged = P > 1;
  DM_TRY(dm_jacobi_rows(ctx, pr, s4, K, &w.sw, &o4));
  if (a.sweeps_host) a.sweeps_host[3] = w.sw;
  // scipy.linalg.pinv: rtol = max(M, N) eps of the matrix it is GIVEN — the padded (nm x P L) beam (beamtransfer.py:891)
  const double rtol = (double)std::max(PL, maxnm) * 2.220446049250313e-16;
  DM_SVD_LAUNCH(ctx, svd_pinv_weights_kernel, dim3(nch), s4, w.d_nm, w4, K, rtol);
  std::vector<dm_gemm_desc> g;
  g.reserve(nch);
  for (int c = 0; c < nch; ++c) {
    const int nm = w.nmodes[c];
    if (nm == 0) continue;
    const int ld2 = geo2[c].ldz, Lc = w.geo[c].Lc;
    const cplx* Y = Z2 + geo2[c].zoff;                   // (nm x P Lc): rows = s_k v_k^H
    const cplx* W = Y + P * Lc;                          // (nm x nm): rows of U_b^H
    // ibeam (PL x nm) = Y^H diag(w) W ; destination is (P, L, K) with K the fastest axis: one product per
    // polarisation, into the rows l >= lmin of the (zero-filled) output
    for (int pp = 0; pp < P; ++pp)
      g.push_back(dm_gemm_make(Y + (size_t)pp * Lc, 1, ld2, true, W, ld2, 1, false,
                               a.ibeam + (size_t)c * PL * K + ((size_t)pp * L + w.geo[c].lmin) * K, K, Lc, nm, nm, 1.0, 0.0,
                               w4 + (size_t)c * K));
  }
  return dm_gemm_grouped_launch(ctx, g);
}

}  // namespace

extern "C" int dm_svd_chain(dm_ctx* ctx, int nblk, int F, int T, int P, int L, const void* beam_m_dev,
                            const double* noisew_dev, double polsvcut, void* beam_svd_dev, void* invbeam_svd_dev,
                            void* beam_ut_dev, double* sigma_dev, int* nmodes_host, int* sweeps_host) {
  return dm_svd_chain_lmin(ctx, nblk, F, T, P, L, nullptr, beam_m_dev, noisew_dev, polsvcut, beam_svd_dev,
                           invbeam_svd_dev, beam_ut_dev, sigma_dev, nmodes_host, sweeps_host);
}

extern "C" int dm_svd_chain_lmin(dm_ctx* ctx, int nblk, int F, int T, int P, int L, const int* lmin_host,
                                 const void* beam_m_dev, const double* noisew_dev, double polsvcut,
                                 void* beam_svd_dev, void* invbeam_svd_dev, void* beam_ut_dev, double* sigma_dev,
                                 int* nmodes_host, int* sweeps_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nblk >= 0 && F > 0 && T > 0 && P > 0 && L > 0 && beam_m_dev && noisew_dev && beam_svd_dev &&
                  beam_ut_dev && sigma_dev && nmodes_host);
  if (sweeps_host) { sweeps_host[0] = sweeps_host[1] = sweeps_host[2] = sweeps_host[3] = 0; }
  if (nblk == 0) return DM_OK;
  if (lmin_host) for (int b = 0; b < nblk; ++b) DM_ARG(ctx, lmin_host[b] >= 0 && lmin_host[b] < L);
  const svd_args a{nblk, F, T, P, L, lmin_host, reinterpret_cast<const cplx*>(beam_m_dev), noisew_dev, polsvcut,
                   reinterpret_cast<cplx*>(beam_svd_dev), reinterpret_cast<cplx*>(invbeam_svd_dev),
                   reinterpret_cast<cplx*>(beam_ut_dev), sigma_dev, nmodes_host, sweeps_host, nblk * F, P * L, std::min(L, T)};
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  svd_ws w(svd_routes(P), a.nch, T);
  svd_geometry(a, w);
  DM_TRY(svd_build_z(ctx, a, w));
  if (P > 1) {
    DM_TRY(svd_phase1(ctx, a, w));
    DM_TRY(svd_phase2(ctx, a, w));
  }
  DM_TRY(svd_phase3(ctx, a, w));
  DM_TRY(svd_products(ctx, a, w));
  if (a.ibeam) DM_TRY(svd_pinv(ctx, a, w));
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}
