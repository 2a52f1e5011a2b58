// dm_tsim.hip — receiver noise of simulated timestreams, drawn in the time domain:
// out[r, i, p, t] = sigma[i, p] z with z the unit complex normal of (pair p, global frequency, time sample t,
// realisation first + r).
//
// Draws: Philox4x32-10 keyed by the 64-bit seed, counter (p, fglobal[i], t, ((first + r) << 8) | STREAM_TS_NOISE); one
// block of the generator is one complex draw (dm_philox.h), so a draw is a fixed function of those five numbers whatever
// frequencies, realisation range or chunking a call asks for.  The low byte of word 3 keeps the noise apart from the
// Monte-Carlo streams (0, 1, 2) and the sky streams (16, 17), whose word 3 is the bare stream number.
#include "dm_common.h"
#include "dm_philox.h"
#include "../../include/driftmi.h"

#include <vector>

namespace {

constexpr uint32_t STREAM_TS_NOISE = 24;

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

}  // namespace

extern "C" int dm_ts_noise(dm_ctx* ctx, int nreal, int nf, int npairs, int ntime, const double* sigma_dev,
                           const int* fglobal_host, uint64_t seed, int first, void* out_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nreal >= 0 && nf >= 0 && npairs >= 0 && ntime >= 0 && first >= 0);
  if ((int64_t)first + nreal > (1LL << 24)) {
    ctx->err = "dm_ts_noise: realisation " + std::to_string((int64_t)first + nreal - 1) +
               " does not fit the 24 bits of the counter word it shares with the stream number";
    return DM_EARG;
  }
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
