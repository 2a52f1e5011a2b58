// dm_psmc.hip — the Monte-Carlo Fisher estimators: counter-based sample draws, the moments of the sampled q, and the
// band vectors of the stochastic-trace estimator.
//
// Replaces PSMonteCarlo.gen_sample / _work_fisher_bias_m (drift/core/psmc.py:26-89), CrossPower._work_fisher_bias_m
// (drift/core/crosspower.py:10-45) and PSMonteCarloAlt.gen_vecs / _work_fisher_bias_m (drift/core/psmc.py:111-199).
//
// Draws: Philox4x32-10 keyed by the 64-bit seed, counter (mode i, sample s, m, stream); one block of the generator is
// one complex draw, so a draw is a fixed function of (seed, m, s, i, stream) whatever the split into calls, batches or
// ranks.  Every reduction is a fixed-order sum (no atomics): two calls give bit-identical results.
#include "dm_common.h"
#include "dm_kernels.h"
#include "dm_philox.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int BG_CHUNK = 2048;    // complex elements of (mode, sample) per band_gram partial sum

struct draw_desc { const double* lam; cplx* x; int n; int m; };

// x[i * R + r] = draw(i, s0 + r) * (lam_i + 1)^(power / 2)
//   kind 0: complex standard normal, E|z|^2 = 1 (Box-Muller: |z| = sqrt(-log u1), arg z = 2 pi u2)
//   kind 1: Rademacher +-1 (the top bit of the first word), real
__global__ __launch_bounds__(256) void psmc_draw_kernel(const draw_desc* __restrict__ ds, uint32_t k0, uint32_t k1,
                                                       uint32_t stream, int kind, int power, int s0, int R) {
  const draw_desc d = ds[blockIdx.y];
  const size_t tot = (size_t)d.n * R;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const int i = (int)(e / R), r = (int)(e - (size_t)i * R);
    // the sample number in uint32_t: s0 + r may pass 2^31 (dm_psmc_draw admits s0 + R <= 2^32), which an int sum must not
    uint32_t c[4] = {(uint32_t)i, (uint32_t)s0 + (uint32_t)r, (uint32_t)d.m, stream};
    philox4x32_10(c, k0, k1);
    double sc = 1.0;
    if (power > 0) sc = sqrt(d.lam[i] + 1.0);
    else if (power < 0) sc = 1.0 / sqrt(d.lam[i] + 1.0);
    cplx z;
    if (kind == DM_PSMC_RADEMACHER) {
      z.x = (c[0] >> 31) ? -sc : sc;
      z.y = 0.0;
    } else {
      z = philox_normal(c, sc);
    }
    d.x[e] = z;
  }
}

// mean[b][a] = sum_s q[b][a][s] / ns: one workgroup per (a, b), a strided walk and a tree in LDS
__global__ __launch_bounds__(256) void psmc_mean_kernel(const double* __restrict__ q, double* __restrict__ mean, int nq,
                                                       int ns) {
  __shared__ double red[256];
  const size_t row = (size_t)blockIdx.y * nq + blockIdx.x;
  const double* qa = q + row * ns;
  double s = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256) s += qa[i];
  dm_block_sum256(red, s);
  if (threadIdx.x == 0) mean[row] = red[0] / ns;
}

// cov[b][a][c] = cov[b][c][a] = sum_s (q_a - mean_a)(q_c - mean_c) / (ns - 1) for c <= a: one workgroup per (a nq + c, b)
__global__ __launch_bounds__(256) void psmc_cov_kernel(const double* __restrict__ q, const double* __restrict__ mean,
                                                      double* __restrict__ cov, int nq, int ns) {
  __shared__ double red[256];
  const int a = blockIdx.x / nq, c = blockIdx.x - a * nq, b = blockIdx.y;
  if (c > a) return;
  const double* qa = q + ((size_t)b * nq + a) * ns;
  const double* qc = q + ((size_t)b * nq + c) * ns;
  const double ma = mean[(size_t)b * nq + a], mc = mean[(size_t)b * nq + c];
  double s = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256) s += (qa[i] - ma) * (qc[i] - mc);
  dm_block_sum256(red, s);
  if (threadIdx.x == 0) {
    const double v = red[0] / (ns - 1);
    cov[((size_t)b * nq + a) * nq + c] = v;
    cov[((size_t)b * nq + c) * nq + a] = v;
  }
}

// w[i] = (lam[i] + 1)^-1/2 over the whole eigenvalue array of the batch
__global__ __launch_bounds__(256) void psmc_rsqrt_kernel(const double* __restrict__ lam, double* __restrict__ w, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = 1.0 / sqrt(lam[i] + 1.0);
}

struct gram_desc { const cplx* v; const double* w; int nm; };   // v: band 0 of the block, bands vstride apart

// v[a][i][r] *= w[i] for every band of the block: the C^-1/2 weight of the modes
__global__ __launch_bounds__(256) void psmc_rowscale_kernel(const gram_desc* __restrict__ ds, size_t vstride, int R) {
  const gram_desc d = ds[blockIdx.y];
  cplx* v = const_cast<cplx*>(d.v) + blockIdx.z * vstride;
  const size_t tot = (size_t)d.nm * R;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const double w = d.w[e / R];
    cplx t = v[e];
    t.x *= w;
    t.y *= w;
    v[e] = t;
  }
}

// part[b][a][c][chunk] = sum_{e in chunk} v_a[e] conj(v_c[e]) for c <= a over the (mode, sample) elements e of block b:
// one workgroup per (chunk, a nbands + c, block), a strided walk and a tree in LDS
__global__ __launch_bounds__(256) void band_gram_kernel(const gram_desc* __restrict__ ds, size_t vstride, int R,
                                                       int nbands, int nchunk, double2* __restrict__ part) {
  __shared__ double2 red[256];
  const int a = blockIdx.y / nbands, c = blockIdx.y - a * nbands;
  if (c > a) return;
  const gram_desc d = ds[blockIdx.z];
  const size_t tot = (size_t)d.nm * R;
  const size_t e0 = (size_t)blockIdx.x * BG_CHUNK, e1 = min(tot, e0 + BG_CHUNK);
  const cplx* va = d.v + a * vstride;
  const cplx* vc = d.v + c * vstride;
  double sr = 0.0, si = 0.0;
  for (size_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const cplx x = va[e], y = vc[e];
    sr += x.x * y.x + x.y * y.y;
    si += x.y * y.x - x.x * y.y;
  }
  dm_block_sum256(red, make_double2(sr, si));
  if (threadIdx.x == 0) part[(((size_t)blockIdx.z * nbands + a) * nbands + c) * nchunk + blockIdx.x] = red[0];
}

// F[b][a][c] = sum_chunk part / ns, F[b][c][a] = conj (fixed order); one thread per (a, c, b)
__global__ __launch_bounds__(256) void band_gram_reduce_kernel(const double2* __restrict__ part, cplx* __restrict__ fisher,
                                                              const int* __restrict__ nchunks, int nbands, int nchunk,
                                                              double ns) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= nbands * nbands) return;
  const int a = p / nbands, c = p - a * nbands;
  if (c > a) return;
  const double2* pp = part + (((size_t)b * nbands + a) * nbands + c) * nchunk;
  double sr = 0.0, si = 0.0;
  for (int k = 0; k < nchunks[b]; ++k) {
    sr += pp[k].x;
    si += pp[k].y;
  }
  cplx v;
  v.x = sr / ns;
  v.y = si / ns;
  fisher[((size_t)b * nbands + a) * nbands + c] = v;
  v.y = -v.y;
  if (c != a) fisher[((size_t)b * nbands + c) * nbands + a] = v;
}

}  // namespace

extern "C" int dm_psmc_draw(dm_ctx* ctx, int nblk, const int* m_host, const int* nmodes_host, const double* evals_dev,
                            const int64_t* evals_off_host, uint64_t seed, int stream, int kind, int power, int s0, int R,
                            void* x_dev, const int64_t* x_off_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nblk >= 0 && m_host && nmodes_host && x_dev && x_off_host && R > 0 && s0 >= 0 && stream >= 0);
  DM_ARG(ctx, (kind == DM_PSMC_NORMAL || kind == DM_PSMC_RADEMACHER) && power >= -1 && power <= 1);
  DM_ARG(ctx, power == 0 || (evals_dev && evals_off_host));
  DM_ARG(ctx, (int64_t)s0 + R <= (1LL << 32));
  dm_ws_scope ws_scope__(ctx);
  std::vector<draw_desc> dd;
  size_t maxtot = 0;
  for (int b = 0; b < nblk; ++b) {
    DM_ARG(ctx, nmodes_host[b] >= 0 && m_host[b] >= 0);
    if (nmodes_host[b] == 0) continue;
    dd.push_back(draw_desc{power ? evals_dev + evals_off_host[b] : nullptr, reinterpret_cast<cplx*>(x_dev) + x_off_host[b],
                           nmodes_host[b], m_host[b]});
    maxtot = std::max(maxtot, (size_t)nmodes_host[b] * R);
  }
  if (dd.empty()) return DM_OK;
  draw_desc* d_dd = dm_ws_upload(ctx, dd);
  if (!d_dd) return DM_ENOMEM;
  const unsigned gx = (unsigned)std::min<size_t>((maxtot + 255) / 256, 4096);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, psmc_draw_kernel, dim3(gx, (unsigned)dd.size()), dim3(256), 0, ctx->stream, d_dd,
             (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream, kind, power, s0, R);
  DM_HIP(ctx, hipGetLastError());
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}

extern "C" int dm_psmc_moments(dm_ctx* ctx, int nblk, int nq, int ns, const double* q_dev, double* mean_dev,
                               double* cov_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nblk >= 0 && nq > 0 && ns >= 2 && q_dev && mean_dev && cov_dev && nblk <= 65535);
  if (nblk == 0) return DM_OK;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, psmc_mean_kernel, dim3((unsigned)nq, (unsigned)nblk), dim3(256), 0, ctx->stream, q_dev,
             mean_dev, nq, ns);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, psmc_cov_kernel, dim3((unsigned)(nq * nq), (unsigned)nblk), dim3(256), 0, ctx->stream,
             q_dev, mean_dev, cov_dev, nq, ns);
  DM_HIP(ctx, hipGetLastError());
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}

extern "C" int dm_psmc_alt(dm_ctx* ctx, int nblk, int F, int K, int P, int L, const void* beam_svd_dev,
                           const int* svnum_host, const int* l0_host, int nbands, const double* cl_bands_dev,
                           const void* evecs_dev, const int64_t* evecs_off_host, const int* nmodes_host,
                           const double* evals_dev, const int64_t* evals_off_host, int R, const void* x_dev,
                           const int64_t* x_off_host, int nsamples, void* v_dev, void* fisher_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nbands > 0 && nsamples > 0 && beam_svd_dev && cl_bands_dev && evecs_dev && evecs_off_host && evals_dev &&
                  x_dev && x_off_host && fisher_dev);
  DM_ARG(ctx, nblk <= 65535 && nbands <= 128);
  dm_band_proj pj;
  DM_TRY(pj.init(ctx, nblk, F, K, P, L, svnum_host, l0_host, nmodes_host, evals_off_host, R));
  if (nblk == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);
  const int N = nblk * R, PL = P * L;
  const std::vector<int>& ndof = pj.ndof;
  const std::vector<int>& active = pj.active;
  const std::vector<int>& l0eff = pj.l0eff;
  const std::vector<int64_t>& off1 = pj.off1;
  const size_t tot1 = pj.tot1, totw = pj.totw;
  const cplx* evecs = reinterpret_cast<const cplx*>(evecs_dev);
  const cplx* beam = reinterpret_cast<const cplx*>(beam_svd_dev);
  const cplx* xin = reinterpret_cast<const cplx*>(x_dev);
  cplx* fisher = reinterpret_cast<cplx*>(fisher_dev);

  std::vector<int64_t> offv(nblk, 0);
  size_t totv = 0;
  for (int b = 0; b < nblk; ++b) {
    DM_ARG(ctx, nmodes_host[b] >= 0);
    offv[b] = (int64_t)totv;
    totv += (size_t)nmodes_host[b] * R;
  }
  const size_t x2n = (size_t)nblk * L * F * R;
  cplx* x1 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot1, 1));
  cplx* x2 = dm_ws_alloc_t<cplx>(ctx, x2n);
  cplx* z = dm_ws_alloc_t<cplx>(ctx, x2n * nbands);
  cplx* y1 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot1, 1) * nbands);
  cplx* v = v_dev ? reinterpret_cast<cplx*>(v_dev) : dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totv, 1) * nbands);
  double* w = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totw, 1));
  double* tab = dm_ws_alloc_t<double>(ctx, (size_t)nbands * L * F * F);
  int* d_l0 = dm_ws_upload(ctx, l0eff);
  if (!x1 || !x2 || !z || !y1 || !v || !w || !tab || !d_l0) return DM_ENOMEM;
  if (v_dev && totv > 0) DM_TRY(dm_fill_zero(ctx, v, sizeof(cplx) * totv * nbands));   // (nbands, T): nothing where T = 0

  dm_band_tables(ctx, cl_bands_dev, tab, nbands, F, L);
  // x1 = E^H X (the draws carry their C^-1/2 weight already), x2 = B^H x1, Z_a = C_a x2 for every band
  DM_TRY(pj.to_svd(ctx, evecs, evecs_off_host, nullptr, x_off_host, 1, &xin, &x1));
  DM_TRY(pj.to_sky(ctx, beam, 1, &x1, &x2));
  dm_band_apply(ctx, x2, tab, d_l0, z, F, L, R, N, nbands);
  // y1_a[f-range] = B_f[:, 0, l >= l0] Z_a[l >= l0][f], then v_a = E y1_a
  {
    std::vector<dm_gemm_desc> g;
    for (int b = 0; b < nblk; ++b) {
      if (!active[b]) continue;
      const int l0 = l0eff[b];
      for (int a = 0; a < nbands; ++a) {
        const cplx* za = z + ((size_t)b * nbands + a) * L * F * R;
        int row = 0;
        for (int f = 0; f < F; ++f) {
          const int ns = svnum_host[b * F + f];
          if (ns > 0) {
            const cplx* Bf = beam + (((size_t)b * F + f) * K) * PL + l0;
            g.push_back(dm_gemm_make(Bf, PL, 1, false, za + ((size_t)l0 * F + f) * R, F * R, 1, false,
                                     y1 + a * tot1 + off1[b] + (size_t)row * R, R, ns, R, L - l0));
          }
          row += ns;
        }
      }
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
    g.clear();
    for (int b = 0; b < nblk; ++b) {
      if (!active[b]) continue;
      const int n = ndof[b], nm = nmodes_host[b];
      for (int a = 0; a < nbands; ++a)
        g.push_back(dm_gemm_make(evecs + evecs_off_host[b], n, 1, false, y1 + a * tot1 + off1[b], R, 1, false,
                                 v + a * totv + offv[b], R, nm, R, n));
    }
    DM_TRY(dm_gemm_grouped_launch(ctx, g));
  }
  // the weights (lam + 1)^-1/2, applied to the rows of every v_a, then the Gram matrices
  std::vector<gram_desc> gd;
  std::vector<int> nch(nblk, 0);
  int nchunk = 1;
  size_t maxnm = 1;
  for (int b = 0; b < nblk; ++b) {
    gd.push_back(gram_desc{v + offv[b], w + evals_off_host[b], active[b] ? nmodes_host[b] : 0});
    nch[b] = (int)(((size_t)gd.back().nm * R + BG_CHUNK - 1) / BG_CHUNK);
    nchunk = std::max(nchunk, nch[b]);
    maxnm = std::max(maxnm, (size_t)gd.back().nm);
  }
  DM_ARG(ctx, nchunk <= (1 << 30));
  gram_desc* d_gd = dm_ws_upload(ctx, gd);
  int* d_nch = dm_ws_upload(ctx, nch);
  double2* part = dm_ws_alloc_t<double2>(ctx, (size_t)nblk * nbands * nbands * nchunk);
  if (!d_gd || !d_nch || !part) return DM_ENOMEM;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, psmc_rsqrt_kernel, dim3((unsigned)((totw + 255) / 256)), dim3(256), 0, ctx->stream,
             evals_dev, w, totw);
  {
    const unsigned gx = (unsigned)std::min<size_t>((maxnm * R + 255) / 256, 4096);
    DM_PLAUNCH(ctx, DM_PROF_UTIL, psmc_rowscale_kernel, dim3(gx, (unsigned)nblk, (unsigned)nbands), dim3(256), 0,
               ctx->stream, d_gd, totv, R);
  }
  DM_PLAUNCH(ctx, DM_PROF_UTIL, band_gram_kernel, dim3((unsigned)nchunk, (unsigned)(nbands * nbands), (unsigned)nblk),
             dim3(256), 0, ctx->stream, d_gd, totv, R, nbands, nchunk, part);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, band_gram_reduce_kernel, dim3((unsigned)((nbands * nbands + 255) / 256), (unsigned)nblk),
             dim3(256), 0, ctx->stream, part, fisher, d_nch, nbands, nchunk, (double)nsamples);
  DM_HIP(ctx, hipGetLastError());
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}
