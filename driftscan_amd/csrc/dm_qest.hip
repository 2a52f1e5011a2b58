// dm_qest.hip — quadratic estimator of the band powers, q_a = Re y^H C^-1 Q_a C^-1 x, for R data columns per m-block.
//
// Replaces PSEstimation.q_estimator (drift/core/psestimation.py:582-652).  Per block, for X (nmodes x R):
//   x1 = E^H diag(1 / (lam + 1)) X                   one grouped ZGEMM (the weights ride on the contraction index)
//   x2[l, f, :] = B_f[:, 0, l]^H x1[f-range, :]       one grouped ZGEMM per (block, frequency), temperature only
//   q[a, :] = Re sum_{l >= l0} sum_{f, f'} conj(y2[l, f, :]) C_a[f, f', l] x2[l, f', :]     dm_band_qform
// and the noise term sum_i Re(x0_i conj(y0_i)) w_i, w = (crosspower ? 0 : 1) + (zero_mean ? lam : 0).
// The two projections and the band products are dm_band.hip's, shared with dm_psmc_alt.
// Every reduction is a fixed-order sum (no atomics): two calls give bit-identical results.
#include "dm_common.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <vector>

namespace {

struct w_desc { const double* lam; double* w; int n; };

// w[i] = 1 / (lam[i] + 1)
__global__ __launch_bounds__(256) void qest_weights_kernel(const w_desc* __restrict__ ds) {
  const w_desc d = ds[blockIdx.y];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += gridDim.x * 256) d.w[i] = 1.0 / (d.lam[i] + 1.0);
}

// q[b][a][r] = sum_lc part[(a * nlc + lc) * N + b R + r]   (fixed order); zero for blocks without modes
__global__ __launch_bounds__(256) void qest_reduce_kernel(const double* __restrict__ part, double* __restrict__ q,
                                                         const int* __restrict__ active, int N, int R, int nbands,
                                                         int nq, int nlc) {
  const int n = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
  if (n >= N) return;
  const int b = n / R, r = n - b * R;
  double s = 0.0;
  if (active[b])
    for (int c = 0; c < nlc; ++c) s += part[((size_t)a * nlc + c) * N + n];
  q[((size_t)b * nq + a) * R + r] = s;
}

struct noise_desc { const cplx* x; const cplx* y; const double* lam; double* q; int nm; };

// q_noise[r] = sum_i Re(x_i conj(y_i)) w_i / (lam_i + 1)^2, w = c_noise + c_lam lam; one workgroup per (block, column),
// a strided walk and a tree in LDS: fixed order
__global__ __launch_bounds__(256) void qest_noise_kernel(const noise_desc* __restrict__ ds, int R, double c_noise,
                                                        double c_lam) {
  __shared__ double red[256];
  const noise_desc d = ds[blockIdx.y];
  const int r = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < d.nm; i += 256) {
    const cplx xv = d.x[(size_t)i * R + r], yv = d.y[(size_t)i * R + r];
    const double lam = d.lam[i], s0 = 1.0 / (lam + 1.0);
    s += (xv.x * yv.x + xv.y * yv.y) * s0 * s0 * (c_noise + c_lam * lam);
  }
  dm_block_sum256(red, s);
  if (threadIdx.x == 0) d.q[r] = red[0];
}

}  // namespace

extern "C" int dm_qestimate(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev,
                            const int* svnum_host, const int* l0_host, int nbands, const double* cl_bands_dev,
                            const void* evecs_dev, const int64_t* evecs_off_host, const int* nmodes_host,
                            const double* evals_dev, const int64_t* evals_off_host, int R, const void* x_dev,
                            const void* y_dev, const int64_t* x_off_host, int flags, double* q_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nbands > 0 && beam_svd_dev && cl_bands_dev && evecs_dev && evecs_off_host && evals_dev && x_dev &&
                  x_off_host && q_dev);
  dm_band_proj pj;
  DM_TRY(pj.init(ctx, nblk, F, K, P, L, svnum_host, l0_host, nmodes_host, evals_off_host, R));
  if (nblk == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  const bool noise = (flags & DM_QEST_NOISE) != 0, cross = y_dev != nullptr;
  const int nq = nbands + (noise ? 1 : 0);
  const int N = nblk * R, nset = cross ? 2 : 1;
  const std::vector<int>& active = pj.active;
  const cplx* xin = reinterpret_cast<const cplx*>(x_dev);
  const cplx* yin = cross ? reinterpret_cast<const cplx*>(y_dev) : xin;

  const int nlc = (L + DM_BAND_LC - 1) / DM_BAND_LC;
  const size_t x2n = (size_t)nblk * L * F * R;
  cplx* x1 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(pj.tot1, 1));
  cplx* y1 = cross ? dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(pj.tot1, 1)) : x1;
  cplx* x2 = dm_ws_alloc_t<cplx>(ctx, x2n);
  cplx* y2 = cross ? dm_ws_alloc_t<cplx>(ctx, x2n) : x2;
  double* w = dm_ws_alloc_t<double>(ctx, std::max<size_t>(pj.totw, 1));
  double* tab = dm_ws_alloc_t<double>(ctx, (size_t)nbands * L * F * F);
  double* part = dm_ws_alloc_t<double>(ctx, (size_t)nbands * nlc * N);
  int* d_l0 = dm_ws_upload(ctx, pj.l0eff);
  int* d_act = dm_ws_upload(ctx, active);
  if (!x1 || !y1 || !x2 || !y2 || !w || !tab || !part || !d_l0 || !d_act) return DM_ENOMEM;

  dm_band_tables(ctx, cl_bands_dev, tab, nbands, F, L);
  // w = 1 / (lam + 1) for the active blocks
  {
    std::vector<w_desc> wd;
    int maxn = 0;
    for (int b = 0; b < nblk; ++b)
      if (active[b]) {
        wd.push_back(w_desc{evals_dev + evals_off_host[b], w + evals_off_host[b], nmodes_host[b]});
        maxn = std::max(maxn, nmodes_host[b]);
      }
    if (!wd.empty()) {
      w_desc* d_wd = dm_ws_upload(ctx, wd);
      if (!d_wd) return DM_ENOMEM;
      DM_PLAUNCH(ctx, DM_PROF_UTIL, qest_weights_kernel, dim3((maxn + 255) / 256, (unsigned)wd.size()), dim3(256), 0,
                 ctx->stream, d_wd);
    }
  }
  // x1 = E^H diag(w) X, x2 = B^H x1 (and y1, y2), then the band terms
  const cplx* const xs[2] = {xin, yin};
  cplx* const x1s[2] = {x1, y1};
  cplx* const x2s[2] = {x2, y2};
  DM_TRY(pj.to_svd(ctx, reinterpret_cast<const cplx*>(evecs_dev), evecs_off_host, w, x_off_host, nset, xs, x1s));
  DM_TRY(pj.to_sky(ctx, reinterpret_cast<const cplx*>(beam_svd_dev), nset, x1s, x2s));
  dm_band_qform(ctx, x2, y2, tab, d_l0, part, F, L, R, N, nbands);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, qest_reduce_kernel, dim3((N + 255) / 256, nbands), dim3(256), 0, ctx->stream, part, q_dev,
             d_act, N, R, nbands, nq, nlc);
  // the noise term
  if (noise) {
    std::vector<noise_desc> nd;
    for (int b = 0; b < nblk; ++b) {
      double* qb = q_dev + ((size_t)b * nq + nbands) * R;
      if (!active[b]) {
        DM_TRY(dm_fill_zero(ctx, qb, sizeof(double) * R));
        continue;
      }
      nd.push_back(noise_desc{xin + x_off_host[b], yin + x_off_host[b], evals_dev + evals_off_host[b], qb, nmodes_host[b]});
    }
    if (!nd.empty()) {
      noise_desc* d_nd = dm_ws_upload(ctx, nd);
      if (!d_nd) return DM_ENOMEM;
      const double c_noise = (flags & DM_QEST_CROSSPOWER) ? 0.0 : 1.0, c_lam = (flags & DM_QEST_ZERO_MEAN) ? 1.0 : 0.0;
      DM_PLAUNCH(ctx, DM_PROF_UTIL, qest_noise_kernel, dim3((unsigned)R, (unsigned)nd.size()), dim3(256), 0, ctx->stream,
                 d_nd, R, c_noise, c_lam);
    }
  }
  DM_HIP(ctx, hipGetLastError());
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}
