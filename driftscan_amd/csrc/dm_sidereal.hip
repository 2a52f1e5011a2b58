// dm_sidereal.hip — sidereal stacking: dm_sidereal_regrid resamples one day of every row from
// its own cadence phi_j = phi0 + j dphi onto the sidereal grid phi_k = 2 pi k / ntime with a Lanczos kernel stretched
// to the coarser spacing, honours the day's flags, and writes or adds to the accumulators of the stack.
//
// The tap geometry of a day (first tap, tap count and coefficients of every k) is made on the host in long double
// (dm_sidereal_table.h) and uploaded once per call, so the kernel is a banded gather with a per-row validity rule.  A
// workgroup of 4 waves takes one (frequency, tile of rt <= 16 rows, tile of nk <= 64 grid samples of one turn): the
// input samples jlo .. jlo + njs - 1 that the tile's taps touch are staged in LDS once — a wave stages the rows wave,
// wave + 4, ..., its lanes one contiguous run of a row, 16 bytes of x (and 8 of w) per lane — and every element of x
// and w comes from HBM once per call, up to the halo of 2 a s samples between neighbouring tiles.  A flagged sample is
// staged as x = 0 with the mark 1 / w = -1, so that its value, NaN included, reaches nothing.  Then lane = grid sample,
// a thread holds up to 4 rows (wave, wave + 4, ...) and walks the taps of its k once: the coefficient comes from the
// transposed table coef[t][k] (consecutive lanes, consecutive addresses) and is applied to all its rows.  The sums of
// a sample run over t = 0, 1, ... in that order whatever the row, the batch or the row tile, so a row has the same bits
// alone and in any batch; the tap sum of x is compensated (sid_dot2).  Outputs are stored 16 (sum) and 8 (wsum, sq)
// bytes per lane, k contiguous across the lanes.
#include "dm_common.h"
#include "dm_sidereal_table.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <vector>

// No implicit contraction anywhere in this file: where the compiler fuses a multiply and an add may differ between the
// copies it makes of a loop body (full and partial row sets, unrolled and remainder taps), and the bits of a sample must
// not depend on which copy ran.  The fused operations that are wanted are written as __builtin_fma.
#pragma clang fp contract(off)

namespace {

constexpr int SID_WAVES = 4, SID_RPT = DM_SIDEREAL_ROWS / SID_WAVES;

// s + e += c x with the rounding errors of the product and of the sum kept in e (Ogita, Rump and Oishi's Dot2): the tap
// sum of x comes out as if in twice the precision, so that |xh|^2 of sq holds to a few ulps even where the taps cancel.
__device__ __forceinline__ void sid_dot2(double& s, double& e, double c, double x) {
  const double p = c * x;
  const double pe = __builtin_fma(c, x, -p);
  const double t = s + p;
  const double z = t - s;
  const double se = (s - (t - z)) + (p - z);
  s = t;
  e += se + pe;
}

template <bool HAS_W>
__global__ __launch_bounds__(SID_WAVES * 64) void sidereal_regrid_kernel(
    const cplx* __restrict__ x, const double* __restrict__ w, cplx* __restrict__ sum, double* __restrict__ wsum,
    double* __restrict__ sq, int* __restrict__ hits, const int4* __restrict__ tiles, const int4* __restrict__ taps,
    const double2* __restrict__ all, const double* __restrict__ coef, uint32_t nrow, uint32_t nt_in, uint32_t ntime,
    uint32_t ntiles, uint32_t nrtiles, uint32_t rt, uint32_t pitch, double min_share, int accumulate) {
  extern __shared__ cplx sid_lds[];
  cplx* xs = sid_lds;                                                     // [rt][pitch]
  double* wis = reinterpret_cast<double*>(sid_lds + (size_t)rt * pitch);  // [rt][pitch], HAS_W only: 1 / w, -1 flagged
  const uint32_t ti = blockIdx.x % ntiles, cell = blockIdx.x / ntiles;
  const uint32_t ri = cell % nrtiles, f = cell / nrtiles;
  const int4 tile = tiles[ti];                                            // k0, nk, jlo, njs
  const uint32_t row0 = ri * rt;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t rl = wave; rl < rt && row0 + rl < nrow; rl += SID_WAVES) {
    const size_t base = ((size_t)f * nrow + row0 + rl) * nt_in + (uint32_t)tile.z;
    for (uint32_t i = lane; i < (uint32_t)tile.w; i += 64u) {
      cplx v = dm_ldg(x, base + i);
      if constexpr (HAS_W) {
        const double wv = dm_ldg(w, base + i);
        const bool ok = wv > 0.0;
        if (!ok) v = make_double2(0.0, 0.0);
        wis[rl * pitch + i] = ok ? 1.0 / wv : -1.0;
      }
      xs[rl * pitch + i] = v;
    }
  }
  __syncthreads();
  if (lane >= (uint32_t)tile.y) return;
  const uint32_t k = (uint32_t)tile.x + lane;
  const int4 tp = taps[k];                                                // first, span, ntaps
  const double2 al = all[k];                                              // A_all, S_all
  // the taps inside the day; those outside exist and are flagged
  const int t0 = tp.x < 0 ? -tp.x : 0;
  const int t1 = tp.x + tp.y > (int)nt_in ? (int)nt_in - tp.x : tp.y;
  double sx[SID_RPT], sy[SID_RPT], ex[SID_RPT], ey[SID_RPT], sv[SID_RPT], sa[SID_RPT], ss[SID_RPT];
  int nu[SID_RPT], tl[SID_RPT];
  uint32_t rbase[SID_RPT];
  bool live[SID_RPT];
#pragma unroll
  for (int r = 0; r < SID_RPT; ++r) {
    const uint32_t rl = wave + SID_WAVES * r;
    live[r] = rl < rt && row0 + rl < nrow;
    rbase[r] = (live[r] ? rl : wave) * pitch;   // wave < rt always holds for a live wave; a dead row reads row `wave`
    sx[r] = sy[r] = ex[r] = ey[r] = sv[r] = sa[r] = ss[r] = 0.0;
    nu[r] = tl[r] = 0;
  }
  if (!live[0]) return;
  int nr = 0;                                 // rows of this wave: wave, wave + 4, ... below rt and nrow
#pragma unroll
  for (int r = 0; r < SID_RPT; ++r) nr += live[r] ? 1 : 0;
  nr = __builtin_amdgcn_readfirstlane(nr);
  const int off = tp.x - tile.z;
  // one tap of all the thread's rows; a coefficient that is exactly 0 is not a tap
  auto tap = [&](double c, int t) {
    if (c == 0.0) return;
    const double ac = fabs(c), cc = c * c;
#pragma unroll
    for (int r = 0; r < SID_RPT; ++r) {
      if (r >= nr) break;                     // the same for the whole wave
      const uint32_t e = rbase[r] + (uint32_t)(off + t);
      const cplx v = xs[e];
      if constexpr (HAS_W) {
        const double wi = wis[e];
        if (wi >= 0.0) {
          sid_dot2(sx[r], ex[r], c, v.x);
          sid_dot2(sy[r], ey[r], c, v.y);
          sv[r] = __builtin_fma(cc, wi, sv[r]);
          sa[r] += ac;
          ss[r] += c;
          nu[r] += 1;
          tl[r] = t;
        }
      } else {
        sid_dot2(sx[r], ex[r], c, v.x);
        sid_dot2(sy[r], ey[r], c, v.y);
        sv[r] += cc;
        sa[r] += ac;
        ss[r] += c;
        nu[r] += 1;
      }
    }
  };
  // the coefficients of four taps are loaded before the first of them is used: their latency is paid once per four
  const double* cp = coef + (size_t)(t0 > 0 ? t0 : 0) * ntime + k;
  int t = t0;
  for (; t + 4 <= t1; t += 4) {
    double c4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) c4[u] = cp[(size_t)u * ntime];
    cp += 4 * (size_t)ntime;
#pragma unroll
    for (int u = 0; u < 4; ++u) tap(c4[u], t + u);
  }
  for (; t < t1; ++t) {
    const double c = *cp;
    cp += ntime;
    tap(c, t);
  }
#pragma unroll
  for (int r = 0; r < SID_RPT; ++r) {
    if (!live[r]) continue;
    // A >= min_share A_all holds for min_share = 1 exactly when no tap is missing: decided by the count, not by rounding
    const bool share = nu[r] == tp.z || (min_share < 1.0 && sa[r] >= min_share * al.x);
    const bool valid = nu[r] > 0 && share && ss[r] >= 0.5 * al.y && ss[r] > 0.0;
    const size_t e = ((size_t)f * nrow + row0 + wave + SID_WAVES * r) * ntime + k;
    if (valid) {
      const double hx = (sx[r] + ex[r]) / ss[r], hy = (sy[r] + ey[r]) / ss[r];
      double W = (ss[r] * ss[r]) / sv[r];
      if constexpr (HAS_W)   // one tap: W = S^2 / (c^2 / w) is w itself, bit for bit
        if (nu[r] == 1) W = dm_ldg(w, ((size_t)f * nrow + row0 + wave + SID_WAVES * r) * nt_in + (uint32_t)(tp.x + tl[r]));
      double ox = W * hx, oy = W * hy, ow = W, oq = W * (hx * hx + hy * hy);
      int oh = 1;
      if (accumulate) {
        const cplx p = dm_ldg(sum, e);
        ox += p.x;
        oy += p.y;
        ow += dm_ldg(wsum, e);
        if (sq) oq += dm_ldg(sq, e);
        if (hits) oh += hits[e];
      }
      dm_stg(sum, e, make_double2(ox, oy));
      dm_stg(wsum, e, ow);
      if (sq) dm_stg(sq, e, oq);
      if (hits) hits[e] = oh;
    } else if (!accumulate) {
      dm_stg(sum, e, make_double2(0.0, 0.0));
      dm_stg(wsum, e, 0.0);
      if (sq) dm_stg(sq, e, 0.0);
      if (hits) hits[e] = 0;
    }
  }
}

int sid_refuse(dm_ctx* ctx, const std::string& what) {
  ctx->err = "dm_sidereal_regrid: " + what;
  return DM_EARG;
}

}  // namespace

extern "C" int dm_sidereal_max_taps(void) { return DM_SIDEREAL_MAX_TAPS; }

extern "C" int dm_sidereal_regrid(dm_ctx* ctx, int nf, int nrow, int nt_in, int ntime, int a, double phi0, double dphi,
                                  double min_share, const void* x_dev, const double* w_dev, void* sum_dev,
                                  double* wsum_dev, double* sq_dev, int* hits_dev, int accumulate) {
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt_in < 0) return sid_refuse(ctx, "negative size");
  const std::string bad = dm_sidereal_check(nt_in, ntime, a, phi0, dphi, min_share);
  if (!bad.empty()) return sid_refuse(ctx, bad);
  const uint64_t nin = (uint64_t)nf * nrow * nt_in, nout = (uint64_t)nf * nrow * ntime;
  if (nout == 0) return DM_OK;
  if (!sum_dev || !wsum_dev || (nin > 0 && !x_dev)) return sid_refuse(ctx, "null x, sum or wsum with work to do");
  {
    const uint64_t ip[2] = {(uint64_t)x_dev, (uint64_t)w_dev}, ib[2] = {16 * nin, w_dev ? 8 * nin : 0};
    const uint64_t op[4] = {(uint64_t)sum_dev, (uint64_t)wsum_dev, (uint64_t)sq_dev, (uint64_t)hits_dev};
    const uint64_t ob[4] = {16 * nout, 8 * nout, sq_dev ? 8 * nout : 0, hits_dev ? 4 * nout : 0};
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 2; ++i)
        if (dm_spans_overlap(ip[i], ib[i], 0, op[o], ob[o], 0, 1))
          return sid_refuse(ctx, "an output shares an element with x or w");
      for (int p = 0; p < o; ++p)
        if (dm_spans_overlap(op[p], ob[p], 0, op[o], ob[o], 0, 1))
          return sid_refuse(ctx, "two outputs share an element");
    }
  }
  DM_HIP(ctx, hipSetDevice(ctx->device));
  if (nin == 0) {   // no day: nothing is valid
    if (!accumulate) {
      DM_HIP(ctx, hipMemsetAsync(sum_dev, 0, 16 * nout, ctx->stream));
      DM_HIP(ctx, hipMemsetAsync(wsum_dev, 0, 8 * nout, ctx->stream));
      if (sq_dev) DM_HIP(ctx, hipMemsetAsync(sq_dev, 0, 8 * nout, ctx->stream));
      if (hits_dev) DM_HIP(ctx, hipMemsetAsync(hits_dev, 0, 4 * nout, ctx->stream));
    }
    return DM_OK;
  }
  dm_sidereal_geom g;
  dm_sidereal_geometry(nt_in, ntime, a, phi0, dphi, &g);
  const bool has_w = w_dev != nullptr;
  const size_t esz = has_w ? 24 : 16;
  const uint32_t pitch = (uint32_t)g.span_max;
  uint32_t rt = (uint32_t)(DM_SIDEREAL_LDS / (esz * pitch));
  if (rt > DM_SIDEREAL_ROWS) rt = DM_SIDEREAL_ROWS;
  if (rt > (uint32_t)nrow) rt = (uint32_t)nrow;
  if (rt < 1) return sid_refuse(ctx, "a tile of one row does not fit in LDS");   // not reached: SPAN x 24 <= LDS
  const uint64_t ntiles = g.tiles.size() / 4, nrtiles = ((uint64_t)nrow + rt - 1) / rt;
  if (ntiles * nrtiles * (uint64_t)nf >= (1ull << 31)) return sid_refuse(ctx, "too many workgroups for one launch");
  dm_ws_scope ws(ctx);
  std::vector<int> tp(4 * (size_t)ntime, 0);
  std::vector<double> al(2 * (size_t)ntime);
  for (int k = 0; k < ntime; ++k) {
    tp[4 * (size_t)k] = g.first[k];
    tp[4 * (size_t)k + 1] = g.span[k];
    tp[4 * (size_t)k + 2] = g.ntaps[k];
    al[2 * (size_t)k] = g.a_all[k];
    al[2 * (size_t)k + 1] = g.s_all[k];
  }
  const int4* tiles = reinterpret_cast<const int4*>(dm_ws_upload(ctx, g.tiles));
  const int4* taps = reinterpret_cast<const int4*>(dm_ws_upload(ctx, tp));
  const double2* all = reinterpret_cast<const double2*>(dm_ws_upload(ctx, al));
  const double* coef = dm_ws_upload(ctx, g.coef);
  if (!tiles || !taps || !all || !coef) return DM_ENOMEM;
  const size_t lds = (size_t)rt * pitch * esz;
  const unsigned nblocks = (unsigned)(ntiles * nrtiles * (uint64_t)nf);
  const cplx* x = static_cast<const cplx*>(x_dev);
  cplx* sum = static_cast<cplx*>(sum_dev);
  if (has_w)
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (sidereal_regrid_kernel<true>), dim3(nblocks), dim3(SID_WAVES * 64), lds, ctx->stream, x,
               w_dev, sum, wsum_dev, sq_dev, hits_dev, tiles, taps, all, coef, (uint32_t)nrow, (uint32_t)nt_in,
               (uint32_t)ntime, (uint32_t)ntiles, (uint32_t)nrtiles, rt, pitch, min_share, accumulate);
  else
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (sidereal_regrid_kernel<false>), dim3(nblocks), dim3(SID_WAVES * 64), lds, ctx->stream, x,
               w_dev, sum, wsum_dev, sq_dev, hits_dev, tiles, taps, all, coef, (uint32_t)nrow, (uint32_t)nt_in,
               (uint32_t)ntime, (uint32_t)ntiles, (uint32_t)nrtiles, rt, pitch, min_share, accumulate);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}
