// dm_stack.hip — unstacked (per-feed-pair) visibilities: dm_vis_stack, the weighted and
// optionally calibrated mean of the redundant feed pairs of every unique baseline, and dm_vis_expand, its counterpart
// that spreads a stacked sky over the feed pairs with the per-feed gains on it.
//
// Rows: member m of the class table (class_off, members) is the feed pair (i, j) = members[m] of class c(m); the
// members of a class are consecutive rows, so a class is a segment of the row axis and the stack a segment reduction.
// Both kernels share one layout: a workgroup takes one (realisation, frequency, tile of TT time samples, chunk of
// classes); with gains, g[., tile] of all feeds is staged in LDS as [feed][TT] exactly as ts_gain_apply_kernel does
// (dm_tsim.hip).  A workgroup has NW = 8 waves with gains and 4 without (stack_waves, expand_waves); a wave takes the
// classes wave, wave + NW, ... of the chunk; its 64 lanes are W = 64 / TT member slots x TT samples: slot s takes the
// members s, s + W, ... of the class in that order, each lane one 16-byte load (or store) per member, TT consecutive
// lanes one contiguous run of TT x 16 bytes of a row.  TT = dm_gain_tile(nfeed) with gains, 16 without; the chunks
// never cut a class.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_sum.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <vector>

namespace {

// Waves per workgroup: stack_waves (dm_stack_sum.h), 8 with gains and 4 without.  The expansion takes 8 only on the tiles
// of 8 samples and fewer, where the LDS tile is what limits the workgroups of a CU: on the 16-sample tile it measured
// slower with 8 (2.28 ms against 1.92 ms at 128 feeds).
constexpr int expand_waves(bool has_g, int tt) { return has_g && tt <= 8 ? 8 : 4; }

// N = sum w conj(g_i) g_j V, D = sum w |g_i|^2 |g_j|^2 over the members of a class; out = N / D, wout = D / n_c, both 0
// where D == 0; the sums are stack_class_sums of dm_stack_sum.h, which dm_redcal.hip shares.  Slot s adds its members in
// the table's order and the slots are added by an xor butterfly (s ^ 1, s ^ 2, ...), so the order of both sums is a function of (n_c, W) and W of nfeed alone — never of the batch, the chunk, the
// realisation or the other classes.  HAS_G false: no LDS and no table load (conj(g_i) g_j = 1); HAS_W false: no weight
// load.  mfac (one f64 per member: the product of its two feed weights) is optional at run time.  Every element of vis
// (and of w) is loaded once.
template <int TT, bool HAS_G, bool HAS_W>
__global__ __launch_bounds__(stack_waves(HAS_G) * 64) void vis_stack_kernel(const cplx* __restrict__ vis,
                                                                            const double* __restrict__ w,
                                                        const cplx* __restrict__ g, const double* __restrict__ mfac,
                                                        cplx* __restrict__ out, double* __restrict__ wout,
                                                        const int* __restrict__ class_off, const int2* __restrict__ members,
                                                        const int* __restrict__ chunk_off, uint32_t nfeed, uint32_t npairs,
                                                        uint32_t nmem, uint32_t ntime, uint32_t ntiles, uint32_t nchunks,
                                                        uint32_t nf, uint32_t g_each, uint32_t w_each,
                                                        unsigned long long vstride, unsigned long long ostride) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT], HAS_G only
  constexpr int NW = stack_waves(HAS_G);
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const uint32_t rf = cell / ntiles, ti = cell - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  if constexpr (HAS_G)
    stack_stage_gains<TT, NW>(gtile, g, (size_t)((g_each ? r : 0u) * nf + f) * nfeed, nfeed, ntime, tt, t, live);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  const size_t vrow = (size_t)r * vstride + (size_t)f * nmem * ntime + t;
  const size_t wrow = ((size_t)(w_each ? r : 0u) * nf + f) * nmem * ntime + t;
  const int c1 = chunk_off[chunk + 1];
  for (int c = chunk_off[chunk] + (int)wave; c < c1; c += NW) {
    const int m0 = class_off[c], m1 = class_off[c + 1];
    double nx, ny, d;
    stack_class_sums<TT, HAS_G, HAS_W>(vis, w, mfac, members, gtile, vrow, wrow, ntime, m0, m1, s, tt, live, nx, ny, d);
    if (s == 0 && live) {
      const size_t e = (size_t)r * ostride + ((size_t)f * npairs + (uint32_t)c) * ntime + t;
      const bool some = d > 0.0;
      dm_stg(out, e, some ? make_double2(nx / d, ny / d) : make_double2(0.0, 0.0));
      dm_stg(wout, e, some ? d / (double)(m1 - m0) : 0.0);
    }
  }
}

// out[r, f, m, t] (+)= g_i conj(g_j) sky[r, f, c(m), t]: the layout of vis_stack_kernel with the roles of load and store
// exchanged — a lane loads the sky of its sample once per class and stores one element per member of its slot.  HAS_G
// false: the class row is copied to every member, no LDS and no table load.
template <int TT, bool HAS_G>
__global__ __launch_bounds__(expand_waves(HAS_G, TT) * 64) void vis_expand_kernel(const cplx* __restrict__ sky,
                                                                                  const cplx* __restrict__ g,
                                                         cplx* __restrict__ out, const int* __restrict__ class_off,
                                                         const int2* __restrict__ members, const int* __restrict__ chunk_off,
                                                         uint32_t nfeed, uint32_t npairs, uint32_t nmem, uint32_t ntime,
                                                         uint32_t ntiles, uint32_t nchunks, uint32_t nf, uint32_t g_each,
                                                         unsigned long long sstride, unsigned long long ostride,
                                                         int accumulate) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT], HAS_G only
  constexpr uint32_t W = 64 / TT;
  constexpr int NW = expand_waves(HAS_G, TT);
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const uint32_t rf = cell / ntiles, ti = cell - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  if constexpr (HAS_G)
    stack_stage_gains<TT, NW>(gtile, g, (size_t)((g_each ? r : 0u) * nf + f) * nfeed, nfeed, ntime, tt, t, live);
  if (!live) return;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  const size_t srow = (size_t)r * sstride + (size_t)f * npairs * ntime + t;
  const size_t orow = (size_t)r * ostride + (size_t)f * nmem * ntime + t;
  const int c1 = chunk_off[chunk + 1];
  for (int c = chunk_off[chunk] + (int)wave; c < c1; c += NW) {
    const int m0 = class_off[c], m1 = class_off[c + 1];
    const cplx sv = dm_ldg(sky, srow + (size_t)c * ntime);
#pragma unroll 4
    for (int k = m0 + (int)s; k < m1; k += (int)W) {
      cplx v = sv;
      if constexpr (HAS_G) {
        const int2 m = members[k];
        const cplx gi = gtile[(uint32_t)m.x * TT + tt], gj = gtile[(uint32_t)m.y * TT + tt];
        v = cmul(cmulc(gi, gj), sv);
      }
      const size_t e = orow + (size_t)k * ntime;
      if (accumulate) v = cadd(dm_ldg(out, e), v);
      dm_stg(out, e, v);
    }
  }
}

// What the two entry points share: the checked table and its split on the device, and the grid.
struct stack_plan {
  const int* off = nullptr;
  const int2* mem = nullptr;
  const int* chunk = nullptr;
  int tile = 0;
  uint32_t ntiles = 0, nchunks = 0, nmem = 0;
  unsigned nblocks = 0;
  size_t lds = 0;
};

int stack_plan_make(dm_ctx* ctx, const char* who, int nreal, int nf, int nfeed, int npairs, int ntime,
                    const int* class_off_host, const int* members_host, bool has_g, stack_plan* p) {
  p->tile = dm_stack_tile(nfeed, has_g);
  const int64_t ntiles = ((int64_t)ntime + p->tile - 1) / p->tile;
  const int64_t cells = (int64_t)nreal * nf * ntiles;
  const std::vector<int> chunk = dm_stack_chunks(npairs, class_off_host, cells);
  const int64_t nchunks = (int64_t)chunk.size() - 1;
  if (cells * nchunks >= (1LL << 31) || (int64_t)nreal * nf >= (1LL << 31)) {
    ctx->err = std::string(who) + ": too many workgroups for one launch";
    return DM_EARG;
  }
  p->ntiles = (uint32_t)ntiles;
  p->nchunks = (uint32_t)nchunks;
  p->nmem = (uint32_t)class_off_host[npairs];
  p->nblocks = (unsigned)(cells * nchunks);
  p->lds = has_g ? (size_t)nfeed * p->tile * sizeof(cplx) : 0;
  p->off = dm_ws_upload(ctx, std::vector<int>(class_off_host, class_off_host + npairs + 1));
  p->mem = reinterpret_cast<const int2*>(
      dm_ws_upload(ctx, std::vector<int>(members_host, members_host + 2 * (size_t)class_off_host[npairs])));
  p->chunk = dm_ws_upload(ctx, chunk);
  return p->off && p->mem && p->chunk ? DM_OK : DM_ENOMEM;
}

template <int TT, bool HAS_G, bool HAS_W>
int vis_stack_launch(dm_ctx* ctx, const stack_plan& p, const cplx* vis, const double* w, const cplx* g, const double* mfac,
                     cplx* out, double* wout, uint32_t nfeed, uint32_t npairs, uint32_t ntime, uint32_t nf, uint32_t g_each,
                     uint32_t w_each, unsigned long long vstride, unsigned long long ostride) {
  DM_TRY(dm_lds_attr(ctx, &vis_stack_kernel<TT, HAS_G, HAS_W>, p.lds));
  constexpr unsigned threads = stack_waves(HAS_G) * 64;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, (vis_stack_kernel<TT, HAS_G, HAS_W>), dim3(p.nblocks), dim3(threads), p.lds, ctx->stream, vis, w,
             g, mfac, out, wout, p.off, p.mem, p.chunk, nfeed, npairs, p.nmem, ntime, p.ntiles, p.nchunks, nf, g_each,
             w_each, vstride, ostride);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

template <int TT, bool HAS_G>
int vis_expand_launch(dm_ctx* ctx, const stack_plan& p, const cplx* sky, const cplx* g, cplx* out, uint32_t nfeed,
                      uint32_t npairs, uint32_t ntime, uint32_t nf, uint32_t g_each, unsigned long long sstride,
                      unsigned long long ostride, int accumulate) {
  DM_TRY(dm_lds_attr(ctx, &vis_expand_kernel<TT, HAS_G>, p.lds));
  constexpr unsigned threads = expand_waves(HAS_G, TT) * 64;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, (vis_expand_kernel<TT, HAS_G>), dim3(p.nblocks), dim3(threads), p.lds, ctx->stream, sky, g, out,
             p.off, p.mem, p.chunk, nfeed, npairs, p.nmem, ntime, p.ntiles, p.nchunks, nf, g_each, sstride, ostride,
             accumulate);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // namespace

extern "C" int dm_vis_stack(dm_ctx* ctx, int nreal, int w_nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                            const int* class_off_host, const int* members_host, const void* vis_dev, const double* w_dev,
                            const void* g_dev, const double* feed_weight_host, void* out_dev, double* wout_dev,
                            int64_t vis_rstride, int64_t out_rstride) {
  if (!ctx) return DM_EARG;
  const char* who = "dm_vis_stack";
  const bool has_g = g_dev != nullptr, has_w = w_dev != nullptr;
  const std::string bad = dm_pair_args_check(nreal, nf, nfeed, npairs, ntime, std::min(vis_rstride, out_rstride), nullptr,
                                             nullptr, class_off_host, members_host, has_g, feed_weight_host);
  if (!bad.empty()) return dm_refuse(ctx, who, bad);
  DM_ARG(ctx, !has_w || w_nreal == 1 || w_nreal == nreal);
  DM_ARG(ctx, !has_g || g_nreal == 1 || g_nreal == nreal);
  const int64_t nmem = npairs > 0 ? class_off_host[npairs] : 0;
  if (vis_rstride == 0) vis_rstride = (int64_t)nf * nmem * ntime;
  if (out_rstride == 0) out_rstride = (int64_t)nf * npairs * ntime;
  DM_ARG(ctx, vis_rstride >= (int64_t)nf * nmem * ntime && out_rstride >= (int64_t)nf * npairs * ntime);
  if (nreal == 0 || nf == 0 || npairs == 0 || ntime == 0) return DM_OK;
  if (!vis_dev || !out_dev || !wout_dev) return dm_refuse(ctx, who, "null pointer with work to do");
  const uint64_t vrow = (uint64_t)nf * nmem * ntime, orow = (uint64_t)nf * npairs * ntime;
  if (dm_spans_overlap((uint64_t)vis_dev, 16 * vrow, 16 * (uint64_t)vis_rstride, (uint64_t)out_dev, 16 * orow,
                       16 * (uint64_t)out_rstride, nreal) ||
      dm_spans_overlap((uint64_t)vis_dev, 16 * vrow, 16 * (uint64_t)vis_rstride, (uint64_t)wout_dev, 8 * orow,
                       8 * (uint64_t)out_rstride, nreal))
    return dm_refuse(ctx, who, "out or wout shares an element with vis");
  if (dm_spans_overlap((uint64_t)out_dev, 16 * orow, 16 * (uint64_t)out_rstride, (uint64_t)wout_dev, 8 * orow,
                       8 * (uint64_t)out_rstride, nreal))
    return dm_refuse(ctx, who, "out shares an element with wout");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  stack_plan p;
  DM_TRY(stack_plan_make(ctx, who, nreal, nf, nfeed, npairs, ntime, class_off_host, members_host, has_g, &p));
  const double* mfac = nullptr;
  if (feed_weight_host) {
    std::vector<double> fac((size_t)nmem);
    for (int64_t k = 0; k < nmem; ++k) fac[k] = feed_weight_host[members_host[2 * k]] * feed_weight_host[members_host[2 * k + 1]];
    mfac = dm_ws_upload(ctx, fac);
    if (!mfac) return DM_ENOMEM;
  }
  const cplx* vis = static_cast<const cplx*>(vis_dev);
  const cplx* g = static_cast<const cplx*>(g_dev);
  cplx* out = static_cast<cplx*>(out_dev);
  const uint32_t g_each = has_g && g_nreal == nreal ? 1u : 0u, w_each = has_w && w_nreal == nreal ? 1u : 0u;
#define DM_STACK_ARGS                                                                                                  \
  ctx, p, vis, w_dev, g, mfac, out, wout_dev, (uint32_t)nfeed, (uint32_t)npairs, (uint32_t)ntime, (uint32_t)nf, g_each, \
      w_each, (unsigned long long)vis_rstride, (unsigned long long)out_rstride
  if (!has_g)
    return has_w ? vis_stack_launch<DM_STACK_TILE_PLAIN, false, true>(DM_STACK_ARGS)
                 : vis_stack_launch<DM_STACK_TILE_PLAIN, false, false>(DM_STACK_ARGS);
#define DM_STACK_CASE(TT)                                                                  \
  case TT:                                                                                 \
    return has_w ? vis_stack_launch<TT, true, true>(DM_STACK_ARGS) : vis_stack_launch<TT, true, false>(DM_STACK_ARGS)
  switch (p.tile) {
    DM_STACK_CASE(16);
    DM_STACK_CASE(8);
    DM_STACK_CASE(4);
    DM_STACK_CASE(2);
    DM_STACK_CASE(1);
  }
#undef DM_STACK_CASE
#undef DM_STACK_ARGS
  return DM_EARG;
}

extern "C" int dm_vis_expand(dm_ctx* ctx, int nreal, int g_nreal, int nf, int nfeed, int npairs, int ntime,
                             const int* class_off_host, const int* members_host, const void* g_dev, const void* sky_dev,
                             void* out_dev, int64_t sky_rstride, int64_t out_rstride, int accumulate) {
  if (!ctx) return DM_EARG;
  const char* who = "dm_vis_expand";
  const bool has_g = g_dev != nullptr;
  const std::string bad = dm_pair_args_check(nreal, nf, nfeed, npairs, ntime, std::min(sky_rstride, out_rstride), nullptr,
                                             nullptr, class_off_host, members_host, has_g, nullptr);
  if (!bad.empty()) return dm_refuse(ctx, who, bad);
  DM_ARG(ctx, !has_g || g_nreal == 1 || g_nreal == nreal);
  const int64_t nmem = npairs > 0 ? class_off_host[npairs] : 0;
  if (sky_rstride == 0) sky_rstride = (int64_t)nf * npairs * ntime;
  if (out_rstride == 0) out_rstride = (int64_t)nf * nmem * ntime;
  DM_ARG(ctx, sky_rstride >= (int64_t)nf * npairs * ntime && out_rstride >= (int64_t)nf * nmem * ntime);
  if (nreal == 0 || nf == 0 || npairs == 0 || ntime == 0) return DM_OK;
  if (!sky_dev || !out_dev) return dm_refuse(ctx, who, "null pointer with work to do");
  if (dm_spans_overlap((uint64_t)sky_dev, 16 * (uint64_t)nf * npairs * ntime, 16 * (uint64_t)sky_rstride, (uint64_t)out_dev,
                       16 * (uint64_t)nf * nmem * ntime, 16 * (uint64_t)out_rstride, nreal))
    return dm_refuse(ctx, who, "out shares an element with sky");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  stack_plan p;
  DM_TRY(stack_plan_make(ctx, who, nreal, nf, nfeed, npairs, ntime, class_off_host, members_host, has_g, &p));
  const cplx* sky = static_cast<const cplx*>(sky_dev);
  const cplx* g = static_cast<const cplx*>(g_dev);
  cplx* out = static_cast<cplx*>(out_dev);
  const uint32_t g_each = has_g && g_nreal == nreal ? 1u : 0u;
#define DM_EXPAND_ARGS                                                                                       \
  ctx, p, sky, g, out, (uint32_t)nfeed, (uint32_t)npairs, (uint32_t)ntime, (uint32_t)nf, g_each,             \
      (unsigned long long)sky_rstride, (unsigned long long)out_rstride, accumulate
  if (!has_g) return vis_expand_launch<DM_STACK_TILE_PLAIN, false>(DM_EXPAND_ARGS);
#define DM_EXPAND_CASE(TT) \
  case TT:                 \
    return vis_expand_launch<TT, true>(DM_EXPAND_ARGS)
  switch (p.tile) {
    DM_EXPAND_CASE(16);
    DM_EXPAND_CASE(8);
    DM_EXPAND_CASE(4);
    DM_EXPAND_CASE(2);
    DM_EXPAND_CASE(1);
  }
#undef DM_EXPAND_CASE
#undef DM_EXPAND_ARGS
  return DM_EARG;
}
