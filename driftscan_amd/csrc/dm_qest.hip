// dm_qest.hip — quadratic estimator of the band powers, q_a = Re y^H C^-1 Q_a C^-1 x, for R data columns per m-block.
//
// Replaces PSEstimation.q_estimator (drift/core/psestimation.py:582-652).  Per block, for X (nmodes x R):
//   x1 = E^H diag(1 / (lam + 1)) X                   one grouped ZGEMM (the weights ride on the contraction index)
//   x2[l, f, :] = B_f[:, 0, l]^H x1[f-range, :]       one grouped ZGEMM per (block, frequency), temperature only
//   q[a, :] = Re sum_{l >= l0} sum_{f, f'} conj(y2[l, f, :]) C_a[f, f', l] x2[l, f', :]     band_qform (below)
// and the noise term sum_i Re(x0_i conj(y0_i)) w_i, w = (crosspower ? 0 : 1) + (zero_mean ? lam : 0).
// Every reduction is a fixed-order sum (no atomics): two calls give bit-identical results.
#include "dm_common.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int QF_LC = 4;          // multipoles per band_qform workgroup: the partial sums over l are per chunk of QF_LC
constexpr int QF_NJ = 4;          // 16-column MFMA sub-tiles per wave
constexpr int QF_COLS = 4 * 16 * QF_NJ;   // real columns (re / im of a complex column) per workgroup: 256
constexpr int QF_TILE = 4096;     // doubles of the staged table tile (32 KB of LDS)

struct w_desc { const double* lam; double* w; int n; };

// w[i] = 1 / (lam[i] + 1)
__global__ __launch_bounds__(256) void qest_weights_kernel(const w_desc* __restrict__ ds) {
  const w_desc d = ds[blockIdx.y];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += gridDim.x * 256) d.w[i] = 1.0 / (d.lam[i] + 1.0);
}

// (nbands, F*F, L) -> (nbands, L, F*F): every (band, l) tile contiguous for band_qform's staging
__global__ __launch_bounds__(256) void qest_table_transpose_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                   int FF, int L) {
  __shared__ double t[32][33];
  const size_t band = blockIdx.z;
  const double* src = in + band * (size_t)FF * L;
  double* dst = out + band * (size_t)FF * L;
  const int l0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int p = p0 + r, l = l0 + tx;
    t[r][tx] = (p < FF && l < L) ? src[(size_t)p * L + l] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int l = l0 + r, p = p0 + tx;
    if (l < L && p < FF) dst[(size_t)l * FF + p] = t[tx][r];
  }
}

// band_qform: part[(a * nlc + lc) * N + n] = Re sum_{l in chunk lc, l >= l0_b} sum_{f,f'} conj(Y[l,f,n]) C_a[l][f][f'] X[l,f',n]
// for the complex columns n = b R + r of the batch (x2 / y2 laid out (nblk, L, F, R) c128).
// The complex columns are 2N real columns; Z = C_a[l] X is an F x F by F x 2N real product on v_mfma_f64_16x16x4_f64:
//   A = rows i0..i0+15 of the staged tile (LDS), B = 16 real columns of X, D = Z[i0 + (lane >> 4) + 4 r][col],
// and each lane folds its D values straight into Y . Z for its column: Z never leaves the registers.  A workgroup owns
// 256 real columns and a chunk of QF_LC multipoles and walks every band; the tile of (a, l) is staged into LDS once per
// workgroup in row chunks of at most QF_TILE doubles.  The sums over the four row groups and over re / im are fixed
// cross-lane additions, the chunks of l are added by qest_reduce_kernel in order.
__global__ __launch_bounds__(256) void band_qform_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                        const double* __restrict__ tab, const int* __restrict__ l0b,
                                                        double* __restrict__ part, int F, int L, int R, int N, int nbands,
                                                        int nlc) {
  __shared__ double tile[QF_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = blockIdx.y;
  const int lbeg = lc * QF_LC, lend = min(L, lbeg + QF_LC);
  const int Fk = (F + 3) & ~3;                                    // contraction length padded to the MFMA's K = 4
  const int FR = max(16, min((F + 15) & ~15, (QF_TILE / Fk) & ~15));  // rows per staged chunk, a multiple of 16
  const int kq = lane >> 4, cj = lane & 15;
  // this lane's real column in each sub-tile: offset of its (b, l = 0, f = 0) element in doubles, and its first l
  size_t base[QF_NJ];
  int lfirst[QF_NJ];
#pragma unroll
  for (int j = 0; j < QF_NJ; ++j) {
    const int c = blockIdx.x * QF_COLS + wave * 16 * QF_NJ + j * 16 + cj;   // real column
    if (c < 2 * N) {
      const int n = c >> 1, b = n / R, r = n - b * R;
      base[j] = (size_t)b * L * F * 2 * R + 2 * (size_t)r + (c & 1);
      lfirst[j] = l0b[b];
    } else {
      base[j] = 0;
      lfirst[j] = L;   // masked
    }
  }
  const size_t fstride = 2 * (size_t)R;   // doubles between (l, f) and (l, f + 1)
  for (int a = 0; a < nbands; ++a) {
    double acc[QF_NJ];
#pragma unroll
    for (int j = 0; j < QF_NJ; ++j) acc[j] = 0.0;
    for (int l = lbeg; l < lend; ++l) {
      const double* T = tab + ((size_t)a * L + l) * F * F;
      for (int r0 = 0; r0 < F; r0 += FR) {
        const int nr = min(FR, F - r0);
        __syncthreads();
        for (int e = threadIdx.x; e < FR * Fk; e += 256) {
          const int i = e / Fk, k = e - i * Fk;
          tile[e] = (i < nr && k < F) ? T[(size_t)(r0 + i) * F + k] : 0.0;
        }
        __syncthreads();
        for (int i0 = 0; i0 < nr; i0 += 16) {
#pragma unroll
          for (int j = 0; j < QF_NJ; ++j) {
            const bool on = l >= lfirst[j];
            const double* xc = X + base[j] + (size_t)l * F * fstride;
            dm_f64x4 z = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < Fk; k0 += 4) {
              const int k = k0 + kq;
              const double av = tile[(i0 + cj) * Fk + k];
              const double bv = (on && k < F) ? xc[(size_t)k * fstride] : 0.0;
              z = dm_mfma(av, bv, z);
            }
            if (on) {
              const double* yc = Y + base[j] + (size_t)l * F * fstride;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int f = r0 + i0 + kq + 4 * q;
                if (f < r0 + nr) acc[j] += yc[(size_t)f * fstride] * z[q];
              }
            }
          }
        }
      }
    }
    // sum over the four row groups (lanes 16 apart), then re + im (neighbouring lanes): fixed order
#pragma unroll
    for (int j = 0; j < QF_NJ; ++j) {
      double v = acc[j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      v += __shfl_xor(v, 1);
      const int c = blockIdx.x * QF_COLS + wave * 16 * QF_NJ + j * 16 + cj;
      if (lane < 16 && (cj & 1) == 0 && c < 2 * N) part[((size_t)a * nlc + lc) * N + (c >> 1)] = v;
    }
  }
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
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) d.q[r] = red[0];
}

}  // namespace

extern "C" int dm_qestimate(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev,
                            const int* svnum_host, const int* l0_host, int nbands, const double* cl_bands_dev,
                            const void* evecs_dev, const int64_t* evecs_off_host, const int* nmodes_host,
                            const double* evals_dev, const int64_t* evals_off_host, int R, const void* x_dev,
                            const void* y_dev, const int64_t* x_off_host, int flags, double* q_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nblk >= 0 && F > 0 && K > 0 && P > 0 && L > 0 && nbands > 0 && R > 0 && beam_svd_dev && svnum_host &&
                  l0_host && cl_bands_dev && evecs_dev && evecs_off_host && nmodes_host && evals_dev && evals_off_host &&
                  x_dev && x_off_host && q_dev);
  DM_ARG(ctx, F <= 256 && (int64_t)nblk * R < (1LL << 29));   // the staged row chunk holds >= 16 rows of <= 256
  if (nblk == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  const bool noise = (flags & DM_QEST_NOISE) != 0, cross = y_dev != nullptr;
  const int nq = nbands + (noise ? 1 : 0);
  const int N = nblk * R, PL = P * L;
  const cplx* evecs = reinterpret_cast<const cplx*>(evecs_dev);
  const cplx* beam = reinterpret_cast<const cplx*>(beam_svd_dev);
  const cplx* xin = reinterpret_cast<const cplx*>(x_dev);
  const cplx* yin = cross ? reinterpret_cast<const cplx*>(y_dev) : xin;

  std::vector<int> ndof(nblk, 0), active(nblk, 0), l0eff(nblk, L);
  std::vector<int64_t> off1(nblk, 0);
  size_t tot1 = 0, totw = 0;
  for (int b = 0; b < nblk; ++b) {
    for (int f = 0; f < F; ++f) ndof[b] += svnum_host[b * F + f];
    DM_ARG(ctx, svnum_host[b * F] >= 0 && ndof[b] >= 0);
    active[b] = nmodes_host[b] > 0 && ndof[b] > 0 && l0_host[b] < L;
    if (active[b]) l0eff[b] = std::max(l0_host[b], 0);
    off1[b] = (int64_t)tot1;
    tot1 += (size_t)ndof[b] * R;
    totw = std::max<size_t>(totw, (size_t)evals_off_host[b] + std::max(nmodes_host[b], 0));
  }
  const int nlc = (L + QF_LC - 1) / QF_LC;
  const size_t x2n = (size_t)nblk * L * F * R;
  cplx* x1 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot1, 1));
  cplx* y1 = cross ? dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot1, 1)) : x1;
  cplx* x2 = dm_ws_alloc_t<cplx>(ctx, x2n);
  cplx* y2 = cross ? dm_ws_alloc_t<cplx>(ctx, x2n) : x2;
  double* w = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totw, 1));
  double* tab = dm_ws_alloc_t<double>(ctx, (size_t)nbands * L * F * F);
  double* part = dm_ws_alloc_t<double>(ctx, (size_t)nbands * nlc * N);
  int* d_l0 = dm_ws_upload(ctx, l0eff);
  int* d_act = dm_ws_upload(ctx, active);
  if (!x1 || !y1 || !x2 || !y2 || !w || !tab || !part || !d_l0 || !d_act) return DM_ENOMEM;

  // the band tables with every (a, l) tile contiguous
  {
    const int FF = F * F;
    DM_PLAUNCH(ctx, DM_PROF_UTIL, qest_table_transpose_kernel, dim3((L + 31) / 32, (FF + 31) / 32, nbands), dim3(256), 0,
               ctx->stream, cl_bands_dev, tab, FF, L);
  }
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
  // x1 = E^H diag(w) X (and y1)
  {
    std::vector<dm_gemm_desc> g;
    for (int b = 0; b < nblk; ++b) {
      if (!active[b]) continue;
      const int n = ndof[b], nm = nmodes_host[b];
      const cplx* Eb = evecs + evecs_off_host[b];
      g.push_back(dm_gemm_make(Eb, 1, n, true, xin + x_off_host[b], R, 1, false, x1 + off1[b], R, n, R, nm, 1.0, 0.0,
                               w + evals_off_host[b]));
      if (cross)
        g.push_back(dm_gemm_make(Eb, 1, n, true, yin + x_off_host[b], R, 1, false, y1 + off1[b], R, n, R, nm, 1.0, 0.0,
                                 w + evals_off_host[b]));
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
  }
  // x2[b][l][f][:] = B_f[:, 0, l]^H x1[f-range] for l >= l0 (and y2); frequencies without modes are zero
  {
    std::vector<dm_gemm_desc> g;
    for (int b = 0; b < nblk; ++b) {
      if (!active[b]) continue;
      const int l0 = l0eff[b];
      bool gaps = false;
      for (int f = 0; f < F; ++f) gaps |= svnum_host[b * F + f] == 0;
      if (gaps) {
        DM_TRY(dm_fill_zero(ctx, x2 + (size_t)b * L * F * R, sizeof(cplx) * (size_t)L * F * R));
        if (cross) DM_TRY(dm_fill_zero(ctx, y2 + (size_t)b * L * F * R, sizeof(cplx) * (size_t)L * F * R));
      }
      int row = 0;
      for (int f = 0; f < F; ++f) {
        const int ns = svnum_host[b * F + f];
        if (ns > 0) {
          const cplx* Bf = beam + (((size_t)b * F + f) * K) * PL + l0;   // pol 0
          const size_t co = (size_t)b * L * F * R + ((size_t)l0 * F + f) * R;
          g.push_back(dm_gemm_make(Bf, 1, PL, true, x1 + off1[b] + (size_t)row * R, R, 1, false, x2 + co, F * R, L - l0,
                                   R, ns));
          if (cross)
            g.push_back(dm_gemm_make(Bf, 1, PL, true, y1 + off1[b] + (size_t)row * R, R, 1, false, y2 + co, F * R,
                                     L - l0, R, ns));
        }
        row += ns;
      }
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
  }
  // the band terms
  DM_PLAUNCH(ctx, DM_PROF_UTIL, band_qform_kernel, dim3((unsigned)((2 * (size_t)N + QF_COLS - 1) / QF_COLS), nlc), dim3(256),
             0, ctx->stream, reinterpret_cast<const double*>(x2), reinterpret_cast<const double*>(y2), tab, d_l0, part, F,
             L, R, N, nbands, nlc);
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
