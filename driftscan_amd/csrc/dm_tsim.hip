// dm_tsim.hip — receiver noise of simulated timestreams, drawn in the time domain:
// out[r, i, p, t] = sigma[i, p] z with z the unit complex normal of (pair p, global frequency, time sample t,
// realisation first + r); and the per-feed gain errors of section 4.15: their Fourier coefficients (ts_gain_coeff), the
// gains from the two series (ts_gain_compose) and the stacked baseline gains applied to the sky part (ts_gain_apply).
//
// Draws: Philox4x32-10 keyed by the 64-bit seed, counter (p, fglobal[i], t, ((first + r) << 8) | STREAM_TS_NOISE); one
// block of the generator is one complex draw (dm_philox.h), so a draw is a fixed function of those five numbers whatever
// frequencies, realisation range or chunking a call asks for.  The low byte of word 3 keeps the noise apart from the
// Monte-Carlo streams (0, 1, 2) and the sky streams (16, 17), whose word 3 is the bare stream number.
#include "dm_common.h"
#include "dm_philox.h"
#include "dm_gain_table.h"
#include "../../include/driftmi.h"

#include <vector>

namespace {

constexpr uint32_t STREAM_TS_NOISE = 24;
constexpr uint32_t STREAM_TS_GAIN_AMP = 25, STREAM_TS_GAIN_PHASE = 26;

// One draw per lane over the flat (r, i, p, t) index: consecutive lanes are consecutive t (and run on into the next row),
// so a wave stores 1 KB contiguous, one 16-byte store per lane.  The flat index is 64-bit (nreal nf npairs ntime passes
// 2^31); its split is one 64-bit division per workgroup and 32-bit divisions per lane (rows < 2^31, ntime <= 2^30).
__global__ __launch_bounds__(256) void ts_noise_kernel(const double* __restrict__ sigma, const int* __restrict__ fglobal,
                                                       cplx* __restrict__ out, unsigned long long total, uint32_t ntime,
                                                       uint32_t npairs, uint32_t ncell, uint32_t first, uint32_t k0,
                                                       uint32_t k1) {
  const unsigned long long base = (unsigned long long)blockIdx.x * 256u;
  const unsigned long long idx = base + threadIdx.x;
  if (idx >= total) return;
  const unsigned long long row0 = base / ntime;                  // uniform in the workgroup
  const uint32_t tt = (uint32_t)(base - row0 * ntime) + threadIdx.x;
  const uint32_t q = tt / ntime;
  const uint32_t t = tt - q * ntime;
  const uint32_t row = (uint32_t)row0 + q;                       // (r, i, p) flat
  const uint32_t r = row / ncell, cell = row - r * ncell;        // cell = i npairs + p
  const uint32_t i = cell / npairs, p = cell - i * npairs;
  uint32_t c[4] = {p, (uint32_t)fglobal[i], t, ((first + r) << 8) | STREAM_TS_NOISE};
  philox4x32_10(c, k0, k1);
  dm_stg(out, (size_t)idx, philox_normal(c, dm_ldg(sigma, cell)));
}

// Coefficients sigma c_k (A_k - i B_k) = sigma c_k sqrt(2) conj(z) of one gain component, one draw per lane over the flat
// (r, i, feed, k) index, split as in ts_noise_kernel.  Counter (feed, fglobal[i] or 0xFFFFFFFF, k, ((first + r) << 8) | stream).
__global__ __launch_bounds__(256) void ts_gain_coeff_kernel(const double* __restrict__ ck, const int* __restrict__ fglobal,
                                                            cplx* __restrict__ out, unsigned long long total, uint32_t nk,
                                                            uint32_t nfeed, uint32_t ncell, double sigma, uint32_t first,
                                                            uint32_t stream, uint32_t k0, uint32_t k1) {
  const unsigned long long base = (unsigned long long)blockIdx.x * 256u;
  const unsigned long long idx = base + threadIdx.x;
  if (idx >= total) return;
  const unsigned long long row0 = base / nk;                     // uniform in the workgroup
  const uint32_t kk = (uint32_t)(base - row0 * nk) + threadIdx.x;
  const uint32_t q = kk / nk;
  const uint32_t k = kk - q * nk;
  const uint32_t row = (uint32_t)row0 + q;                       // (r, i, feed) flat
  const uint32_t r = row / ncell, cell = row - r * ncell;        // cell = i nfeed + feed
  const uint32_t i = cell / nfeed, a = cell - i * nfeed;
  uint32_t c[4] = {a, fglobal ? (uint32_t)fglobal[i] : 0xFFFFFFFFu, k, ((first + r) << 8) | stream};
  philox4x32_10(c, k0, k1);
  const cplx z = philox_normal(c, sigma * dm_ldg(ck, k) * 1.4142135623730951);
  dm_stg(out, (size_t)idx, make_double2(z.x, -z.y));
}

// g = (1 + Re xa) exp(i Re xp), one element per lane (the series come out of the ZGEMM as complex numbers).
__global__ __launch_bounds__(256) void ts_gain_compose_kernel(const cplx* __restrict__ xa, const cplx* __restrict__ xp,
                                                              cplx* __restrict__ g, unsigned long long total) {
  const unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (idx >= total) return;
  const double amp = 1.0 + dm_ldg(xa, (size_t)idx).x;
  double sn, cs;
  sincos(dm_ldg(xp, (size_t)idx).x, &sn, &cs);
  dm_stg(g, (size_t)idx, make_double2(amp * cs, amp * sn));
}

// out[r, f, c, t] (+)= G sky[r, f, c, t],  G = (1 / n_c) sum_{(i, j) in c} g_i conj(g_j)  at (r, f, t).
// One workgroup per (r, f, tile of TT time samples): g[., tile] of all feeds is staged in LDS as [feed][TT] (16 samples
// are one 256-byte row, one slot of every bank: the ds_read_b128 lane groups then never collide, whatever the feeds).  A
// wave takes the classes wave, wave + 4, ...; its 64 lanes are W = 64 / TT member slots x TT samples: slot s sums the
// members s, s + W, ... of the class in that order, and the slots are added by an xor butterfly (s ^ 1, s ^ 2, ...).  So
// the order of the sum is a function of (n_c, W) and W of nfeed alone — never of the batch or of the other classes.
// Per member and wave: one 8-byte table load per slot, two 16-byte LDS reads and four FMAs per lane.  The LDS reads are the
// floor (the fp64 FMAs need half their cycles); measured, the kernel runs at 5.5 times that floor with its waves waiting
// on the chain table -> LDS address -> g most of the time.
template <int TT>
__global__ __launch_bounds__(256) void ts_gain_apply_kernel(const cplx* __restrict__ g, const cplx* __restrict__ sky,
                                                            cplx* __restrict__ out, const int* __restrict__ class_off,
                                                            const int2* __restrict__ members, uint32_t nfeed,
                                                            uint32_t npairs, uint32_t ntime, uint32_t ntiles, uint32_t nf,
                                                            uint32_t g_each, unsigned long long rstride, int accumulate) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT]
  constexpr uint32_t S = 256 / TT, W = 64 / TT;
  const uint32_t rf = blockIdx.x / ntiles, ti = blockIdx.x - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  const size_t grow = (size_t)((g_each ? r : 0u) * nf + f) * nfeed;
  for (uint32_t a = threadIdx.x / TT; a < nfeed; a += S)
    gtile[a * TT + tt] = live ? dm_ldg(g, (grow + a) * ntime + t) : make_double2(0.0, 0.0);
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  for (uint32_t c = wave; c < npairs; c += 4) {
    const int m0 = class_off[c], m1 = class_off[c + 1];
    double ax = 0.0, ay = 0.0;
#pragma unroll 4
    for (int k = m0 + (int)s; k < m1; k += (int)W) {
      const int2 m = members[k];
      const cplx gi = gtile[(uint32_t)m.x * TT + tt], gj = gtile[(uint32_t)m.y * TT + tt];
      ax = fma(gi.x, gj.x, ax);
      ax = fma(gi.y, gj.y, ax);
      ay = fma(gi.y, gj.x, ay);
      ay = fma(-gi.x, gj.y, ay);
    }
#pragma unroll
    for (int o = TT; o < 64; o <<= 1) {
      ax += __shfl_xor(ax, o, 64);
      ay += __shfl_xor(ay, o, 64);
    }
    if (s == 0 && live) {
      const double n = (double)(m1 - m0);
      const size_t e = (size_t)r * rstride + ((size_t)f * npairs + c) * ntime + t;
      cplx v = cmul(make_double2(ax / n, ay / n), dm_ldg(sky, e));
      if (accumulate) v = cadd(dm_ldg(out, e), v);
      dm_stg(out, e, v);
    }
  }
}

template <int TT>
int ts_gain_apply_launch(dm_ctx* ctx, unsigned nblocks, size_t lds, const cplx* g, const cplx* sky, cplx* out,
                         const int* class_off, const int2* members, uint32_t nfeed, uint32_t npairs, uint32_t ntime,
                         uint32_t ntiles, uint32_t nf, uint32_t g_each, unsigned long long rstride, int accumulate) {
  if (lds > (size_t)DM_GAIN_LDS_SHARED)
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&ts_gain_apply_kernel<TT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  DM_PLAUNCH(ctx, DM_PROF_UTIL, ts_gain_apply_kernel<TT>, dim3(nblocks), dim3(256), lds, ctx->stream, g, sky, out, class_off,
             members, nfeed, npairs, ntime, ntiles, nf, g_each, rstride, accumulate);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

int ts_realisations_fit(dm_ctx* ctx, const char* who, int first, int nreal) {
  if ((int64_t)first + nreal > (1LL << 24)) {
    ctx->err = std::string(who) + ": realisation " + std::to_string((int64_t)first + nreal - 1) +
               " does not fit the 24 bits of the counter word it shares with the stream number";
    return DM_EARG;
  }
  return DM_OK;
}

}  // namespace

extern "C" int dm_ts_noise(dm_ctx* ctx, int nreal, int nf, int npairs, int ntime, const double* sigma_dev,
                           const int* fglobal_host, uint64_t seed, int first, void* out_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nreal >= 0 && nf >= 0 && npairs >= 0 && ntime >= 0 && first >= 0);
  DM_TRY(ts_realisations_fit(ctx, "dm_ts_noise", first, nreal));
  DM_ARG(ctx, ntime <= (1 << 30) && (int64_t)nreal * nf * npairs < (1LL << 31));
  const unsigned long long total = (unsigned long long)nreal * nf * npairs * (unsigned long long)ntime;
  if (total == 0) return DM_OK;
  DM_ARG(ctx, sigma_dev != nullptr && fglobal_host != nullptr && out_dev != nullptr);
  for (int i = 0; i < nf; ++i) DM_ARG(ctx, fglobal_host[i] >= 0);
  const unsigned long long nblocks = (total + 255) / 256;
  DM_ARG(ctx, nblocks < (1ULL << 31));
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  const int* fg = dm_ws_upload(ctx, std::vector<int>(fglobal_host, fglobal_host + nf));
  if (!fg) return DM_ENOMEM;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, ts_noise_kernel, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, sigma_dev, fg,
             static_cast<cplx*>(out_dev), total, (uint32_t)ntime, (uint32_t)npairs, (uint32_t)(nf * npairs),
             (uint32_t)first, (uint32_t)seed, (uint32_t)(seed >> 32));
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

extern "C" int dm_ts_gain_coeff(dm_ctx* ctx, int nreal, int nf, int nfeed, int nk, const int* fglobal_host, int broadband,
                                const double* ck_host, double sigma, uint64_t seed, int first, int stream, void* out_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nreal >= 0 && nf >= 0 && nfeed >= 0 && nk >= 0 && first >= 0);
  DM_ARG(ctx, stream == (int)STREAM_TS_GAIN_AMP || stream == (int)STREAM_TS_GAIN_PHASE);
  DM_TRY(ts_realisations_fit(ctx, "dm_ts_gain_coeff", first, nreal));
  DM_ARG(ctx, nk <= (1 << 30) && (int64_t)nreal * nf * nfeed < (1LL << 31));
  const unsigned long long total = (unsigned long long)nreal * nf * nfeed * (unsigned long long)nk;
  if (total == 0) return DM_OK;
  DM_ARG(ctx, ck_host != nullptr && out_dev != nullptr && (broadband || fglobal_host != nullptr));
  if (!broadband)
    for (int i = 0; i < nf; ++i) DM_ARG(ctx, fglobal_host[i] >= 0);
  const unsigned long long nblocks = (total + 255) / 256;
  DM_ARG(ctx, nblocks < (1ULL << 31));
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  const int* fg = nullptr;
  if (!broadband) {
    fg = dm_ws_upload(ctx, std::vector<int>(fglobal_host, fglobal_host + nf));
    if (!fg) return DM_ENOMEM;
  }
  const double* ck = dm_ws_upload(ctx, std::vector<double>(ck_host, ck_host + nk));
  if (!ck) return DM_ENOMEM;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, ts_gain_coeff_kernel, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, ck, fg,
             static_cast<cplx*>(out_dev), total, (uint32_t)nk, (uint32_t)nfeed, (uint32_t)(nf * nfeed), sigma,
             (uint32_t)first, (uint32_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32));
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

extern "C" int dm_ts_gain_compose(dm_ctx* ctx, int64_t n, const void* xamp_dev, const void* xphase_dev, void* g_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 0);
  if (n == 0) return DM_OK;
  DM_ARG(ctx, xamp_dev != nullptr && xphase_dev != nullptr && g_dev != nullptr);
  const unsigned long long nblocks = ((unsigned long long)n + 255) / 256;
  DM_ARG(ctx, nblocks < (1ULL << 31));
  DM_HIP(ctx, hipSetDevice(ctx->device));
  DM_PLAUNCH(ctx, DM_PROF_UTIL, ts_gain_compose_kernel, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream,
             static_cast<const cplx*>(xamp_dev), static_cast<const cplx*>(xphase_dev), static_cast<cplx*>(g_dev),
             (unsigned long long)n);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

extern "C" int dm_ts_gain_tile(int nfeed) { return dm_gain_tile(nfeed); }

extern "C" int dm_ts_gain_apply(dm_ctx* ctx, int nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                                const int* class_off_host, const int* members_host, const void* g_dev, const void* sky_dev,
                                void* out_dev, int64_t rstride, int accumulate) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nreal >= 0 && nf >= 0 && nfeed >= 0 && npairs >= 0 && ntime >= 0);
  DM_ARG(ctx, g_nreal == 1 || g_nreal == nreal);
  if (rstride == 0) rstride = (int64_t)nf * npairs * ntime;
  DM_ARG(ctx, rstride >= (int64_t)nf * npairs * ntime);
  const std::string bad = dm_gain_table_check(nfeed, npairs, class_off_host, members_host);
  if (!bad.empty()) {
    ctx->err = "dm_ts_gain_apply: " + bad;
    return DM_EARG;
  }
  if (nreal == 0 || nf == 0 || npairs == 0 || ntime == 0) return DM_OK;
  DM_ARG(ctx, g_dev != nullptr && sky_dev != nullptr && out_dev != nullptr);
  const int tile = dm_gain_tile(nfeed);
  const int64_t ntiles = ((int64_t)ntime + tile - 1) / tile;
  DM_ARG(ctx, (int64_t)nreal * nf * ntiles < (1LL << 31) && (int64_t)nreal * nf * npairs < (1LL << 31));
  const unsigned nblocks = (unsigned)((int64_t)nreal * nf * ntiles);
  const size_t lds = (size_t)nfeed * tile * sizeof(cplx);
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  const int* off = dm_ws_upload(ctx, std::vector<int>(class_off_host, class_off_host + npairs + 1));
  const int* mem = dm_ws_upload(ctx, std::vector<int>(members_host, members_host + 2 * (size_t)class_off_host[npairs]));
  if (!off || !mem) return DM_ENOMEM;
  const cplx* g = static_cast<const cplx*>(g_dev);
  const cplx* sky = static_cast<const cplx*>(sky_dev);
  cplx* out = static_cast<cplx*>(out_dev);
  const int2* mem2 = reinterpret_cast<const int2*>(mem);
  const uint32_t g_each = g_nreal == nreal ? 1u : 0u;
#define DM_GAIN_CASE(TT)                                                                                              \
  case TT:                                                                                                            \
    return ts_gain_apply_launch<TT>(ctx, nblocks, lds, g, sky, out, off, mem2, (uint32_t)nfeed, (uint32_t)npairs,     \
                                    (uint32_t)ntime, (uint32_t)ntiles, (uint32_t)nf, g_each,        \
                                    (unsigned long long)rstride, accumulate)
  switch (tile) {
    DM_GAIN_CASE(16);
    DM_GAIN_CASE(8);
    DM_GAIN_CASE(4);
    DM_GAIN_CASE(2);
    DM_GAIN_CASE(1);
  }
#undef DM_GAIN_CASE
  return DM_EARG;
}
