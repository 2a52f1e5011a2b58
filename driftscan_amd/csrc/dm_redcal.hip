// dm_redcal.hip — redundant-baseline calibration: dm_redcal_solve finds the per-feed gains g and
// the class visibilities y that minimise chi^2 = sum_m omega_m |V_m - g_i conj(g_j) y_c|^2, every (realisation,
// frequency, time sample) a problem of its own, by a damped alternating fixed point.
//
// An iteration is two kernels, launched back to back on the context's stream:
//   redcal_y_kernel   the stack of section 4.17 with the current gains (stack_class_sums of dm_stack_sum.h: the arithmetic
//                     and the summation order of vis_stack_kernel<TT, true, HAS_W>), and the book-keeping of the samples;
//   redcal_g_kernel   feed-major over the incidence table of dm_redcal_table.h: a workgroup takes one (realisation,
//                     frequency, tile of TT samples, chunk of feeds), stages g[., tile] of ALL feeds in LDS as [feed][TT],
//                     a wave takes the feeds wave, wave + 8, ... of the chunk, its lanes are W = 64 / TT slots x TT samples,
//                     slot s takes the incidences s, s + W, ... of the feed and the slots are joined by the xor butterfly.
//                     The new gains go to the other of two buffers: other workgroups still read the old ones.
// The state of a sample (0 iterating, 1 converged and owed its last y, 2 done, 3 out of iterations) is read at the start
// of an iteration from the words the previous one left and written to a second set of words, so no workgroup ever reads
// what another writes in the same launch; the step of a sample is the maximum over its feeds, joined across waves and
// workgroups by an integer atomicMax on the bit pattern of a non-negative double, which is the same in any order.  There
// is no floating-point atomic, and every sum lives inside one wave in an order that (d_a, nfeed) or (n_c, nfeed) fix.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_sum.h"
#include "dm_redcal_table.h"
#include "../../include/driftmi.h"

#include <vector>

namespace {

constexpr int RC_NW = stack_waves(true);   // 8 waves per workgroup: the reason measured in section 4.17

// The state of a sample entering iteration `iter`, from its state and its step after iteration iter - 1.  `last`: the
// pass behind the last iteration, which only closes the books.
__device__ __forceinline__ int redcal_state(int in, double step, double tol, int iter, int last) {
  if (iter == 1) return 0;
  if (in == 0) return step < tol ? 1 : (last ? 3 : 0);
  return in == 1 ? 2 : in;
}

// g[e] = g0[e], or 1 without g0.
__global__ __launch_bounds__(256) void redcal_init_kernel(const cplx* __restrict__ g0, cplx* __restrict__ g,
                                                          unsigned long long n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) dm_stg(g, e, g0 ? dm_ldg(g0, e) : make_double2(1.0, 0.0));
}

// y_c = sum omega conj(g_i) g_j V / sum omega |g_i|^2 |g_j|^2 of the samples that still iterate (state 0) or are owed the
// y of their final gains (state 1); 0 where the denominator is 0.  The workgroup of chunk 0 keeps the books of its tile.
template <int TT, bool HAS_W>
__global__ __launch_bounds__(RC_NW * 64) void redcal_y_kernel(
    const cplx* __restrict__ vis, const double* __restrict__ w, const cplx* __restrict__ g, const double* __restrict__ yfac,
    cplx* __restrict__ y, const int* __restrict__ class_off, const int2* __restrict__ members,
    const int* __restrict__ chunk_off, const int* st_in, int* st_out, const unsigned long long* sb_in,
    unsigned long long* sb_out, int* __restrict__ iters, double* __restrict__ step, int* pending, uint32_t nfeed,
    uint32_t npairs, uint32_t nmem, uint32_t ntime, uint32_t ntiles, uint32_t nchunks, uint32_t nf, uint32_t w_each,
    unsigned long long vstride, double tol, int iter, int last) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT]
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const uint32_t rf = cell / ntiles, ti = cell - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  const size_t smp = (size_t)rf * ntime + t;
  int in = 0, now = 2;
  double stp = 0.0;
  if (live) {
    if (iter > 1) {
      in = st_in[smp];
      stp = __longlong_as_double((long long)sb_in[smp]);
    }
    now = redcal_state(in, stp, tol, iter, last);
    if (chunk == 0 && threadIdx.x < TT) {
      st_out[smp] = now;
      sb_out[smp] = 0ull;
      if (in == 0 && now != 0) {
        iters[smp] = iter - 1;
        dm_stg(step, smp, stp);
      }
      if (pending && now < 2) atomicAdd(pending, 1);
    }
  }
  const bool act = now < 2;
  if (!__syncthreads_or(act)) return;
  stack_stage_gains<TT, RC_NW>(gtile, g, (size_t)rf * nfeed, nfeed, ntime, tt, t, live);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  const size_t vrow = (size_t)r * vstride + (size_t)f * nmem * ntime + t;
  const size_t wrow = ((size_t)(w_each ? r : 0u) * nf + f) * nmem * ntime + t;
  const int c1 = chunk_off[chunk + 1];
  for (int c = chunk_off[chunk] + (int)wave; c < c1; c += RC_NW) {
    const int m0 = class_off[c], m1 = class_off[c + 1];
    double nx, ny, d;
    stack_class_sums<TT, true, HAS_W>(vis, w, yfac, members, gtile, vrow, wrow, ntime, m0, m1, s, tt, act, nx, ny, d);
    if (s == 0 && act)
      dm_stg(y, ((size_t)rf * npairs + (uint32_t)c) * ntime + t,
             d > 0.0 ? make_double2(nx / d, ny / d) : make_double2(0.0, 0.0));
  }
}

// g_a <- (1 - delta) g_a + delta [sum omega V conj(z) + sum omega conj(V) conj(z')] / [sum omega |z|^2 + sum omega |z'|^2]
// over the incidences of feed a (z = conj(g_j) y_c where a is the first feed of the member, z' = conj(g_i y_c) where it
// is the second), g_a kept where the denominator is 0; the step |delta g_a| / |g_a| of the sample goes into sb by
// atomicMax.  Samples of state 1 only have their gains copied to the other buffer; states 2 and 3 are not touched.
template <int TT, bool HAS_W>
__global__ __launch_bounds__(RC_NW * 64) void redcal_g_kernel(
    const cplx* __restrict__ vis, const double* __restrict__ w, const cplx* __restrict__ g, cplx* __restrict__ gnew,
    const double* __restrict__ gfac, const cplx* __restrict__ y, const int* __restrict__ inc_off,
    const int4* __restrict__ inc, const int* __restrict__ chunk_off, const int* __restrict__ st, unsigned long long* sb,
    uint32_t nfeed, uint32_t npairs, uint32_t nmem, uint32_t ntime, uint32_t ntiles, uint32_t nchunks, uint32_t nf,
    uint32_t w_each, unsigned long long vstride, double damping) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT]
  constexpr uint32_t W = 64 / TT;
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const uint32_t rf = cell / ntiles, ti = cell - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  const size_t smp = (size_t)rf * ntime + t;
  const int now = live ? st[smp] : 2;
  if (!__syncthreads_or(now < 2)) return;
  stack_stage_gains<TT, RC_NW>(gtile, g, (size_t)rf * nfeed, nfeed, ntime, tt, t, live);
  const bool act = now == 0;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  const size_t vrow = (size_t)r * vstride + (size_t)f * nmem * ntime + t;
  const size_t wrow = ((size_t)(w_each ? r : 0u) * nf + f) * nmem * ntime + t;
  const size_t yrow = (size_t)rf * npairs * ntime + t;
  const double keep = 1.0 - damping;
  double smax = 0.0;
  const int a1 = chunk_off[chunk + 1];
  for (int a = chunk_off[chunk] + (int)wave; a < a1; a += RC_NW) {
    const int k0 = inc_off[a], k1 = inc_off[a + 1];
    double nx = 0.0, ny = 0.0, d = 0.0;
    if (act) {
#pragma unroll 2
      for (int k = k0 + (int)s; k < k1; k += (int)W) {
        const int4 e = inc[k];                                   // member row, partner, class, side
        cplx v = dm_ldg(vis, vrow + (size_t)e.x * ntime);
        double we = dm_ldg(gfac, (size_t)e.x);
        if constexpr (HAS_W) we *= dm_ldg(w, wrow + (size_t)e.x * ntime);
        cplx yc = dm_ldg(y, yrow + (size_t)e.z * ntime);
        const cplx gp = gtile[(uint32_t)e.y * TT + tt];
        if (e.w) v.y = -v.y;                                     // side 1: conj(V) g_i y_c
        else yc.y = -yc.y;                                       // side 0: V g_j conj(y_c)
        const cplx p = cmul(cmul(gp, yc), v);
        nx = fma(we, p.x, nx);
        ny = fma(we, p.y, ny);
        d = fma(we, cabs2(gp) * cabs2(yc), d);
      }
    }
#pragma unroll
    for (int o = TT; o < 64; o <<= 1) {
      nx += __shfl_xor(nx, o, 64);
      ny += __shfl_xor(ny, o, 64);
      d += __shfl_xor(d, o, 64);
    }
    if (s == 0 && now < 2) {
      const cplx ga = gtile[(uint32_t)a * TT + tt];
      cplx gn = ga;
      if (act && d > 0.0) {
        gn.x = keep * ga.x + damping * (nx / d);
        gn.y = keep * ga.y + damping * (ny / d);
        const double dx = gn.x - ga.x, dy = gn.y - ga.y;
        const double q = dx == 0.0 && dy == 0.0 ? 0.0 : sqrt((dx * dx + dy * dy) / cabs2(ga));
        if (q > smax || q != q) smax = q;                        // (a NaN stays: the sample is then never called converged)
      }
      dm_stg(gnew, ((size_t)rf * nfeed + (uint32_t)a) * ntime + t, gn);
    }
  }
  if (s == 0 && act) atomicMax(&sb[smp], (unsigned long long)__double_as_longlong(smax) & 0x7fffffffffffffffull);
}

// chi2 = sum_m omega_m |V_m - g_i conj(g_j) y_c|^2 at the returned g and y: one workgroup per (realisation, frequency,
// tile); wave v takes the classes v, v + 8, ..., slots and butterfly as above, and the eight waves' sums are added in
// their order through LDS: the order is a function of the table and nfeed alone.
template <int TT, bool HAS_W>
__global__ __launch_bounds__(RC_NW * 64) void redcal_chi2_kernel(
    const cplx* __restrict__ vis, const double* __restrict__ w, const cplx* __restrict__ g, const double* __restrict__ gfac,
    const cplx* __restrict__ y, const int* __restrict__ class_off, const int2* __restrict__ members,
    double* __restrict__ chi2, uint32_t nfeed, uint32_t npairs, uint32_t nmem, uint32_t ntime, uint32_t ntiles, uint32_t nf,
    uint32_t w_each, unsigned long long vstride) {
  extern __shared__ cplx gtile[];                                // [nfeed][TT], then RC_NW x TT doubles
  constexpr uint32_t W = 64 / TT;
  double* red = reinterpret_cast<double*>(gtile + (size_t)nfeed * TT);
  const uint32_t rf = blockIdx.x / ntiles, ti = blockIdx.x - rf * ntiles;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const uint32_t tt = threadIdx.x % TT, t = ti * TT + tt;
  const bool live = t < ntime;
  stack_stage_gains<TT, RC_NW>(gtile, g, (size_t)rf * nfeed, nfeed, ntime, tt, t, live);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t s = (threadIdx.x & 63u) / TT;
  const size_t vrow = (size_t)r * vstride + (size_t)f * nmem * ntime + t;
  const size_t wrow = ((size_t)(w_each ? r : 0u) * nf + f) * nmem * ntime + t;
  const size_t yrow = (size_t)rf * npairs * ntime + t;
  double acc = 0.0;
  if (live)
    for (int c = (int)wave; c < (int)npairs; c += RC_NW) {
      const int m0 = class_off[c], m1 = class_off[c + 1];
      const cplx yc = dm_ldg(y, yrow + (size_t)c * ntime);
      for (int k = m0 + (int)s; k < m1; k += (int)W) {
        const cplx v = dm_ldg(vis, vrow + (size_t)k * ntime);
        double we = dm_ldg(gfac, (size_t)k);
        if constexpr (HAS_W) we *= dm_ldg(w, wrow + (size_t)k * ntime);
        const int2 m = members[k];
        const cplx gi = gtile[(uint32_t)m.x * TT + tt], gj = gtile[(uint32_t)m.y * TT + tt];
        const cplx e = csub(v, cmul(cmulc(gi, gj), yc));
        acc = fma(we, cabs2(e), acc);
      }
    }
#pragma unroll
  for (int o = TT; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (s == 0) red[wave * TT + tt] = acc;
  __syncthreads();
  if (threadIdx.x < TT && live) {
    double sum = red[tt];
#pragma unroll
    for (int v = 1; v < RC_NW; ++v) sum += red[v * TT + tt];
    dm_stg(chi2, (size_t)rf * ntime + t, sum);
  }
}

constexpr const char* RC_WHO = "dm_redcal_solve";

struct redcal_args {
  const cplx *vis, *g0;
  const double* w;
  cplx *g, *y;
  int* iters;
  double *step, *chi2;
  const int* class_off_host;
  const int* members_host;
  const dm_redcal_table* table;
  int nreal, nf, nfeed, npairs, ntime, maxiter;
  uint32_t w_each;
  unsigned long long vstride;
  double damping, tol;
};

template <int TT, bool HAS_W>
int redcal_run(dm_ctx* ctx, const redcal_args& a) {
  const dm_redcal_table& tb = *a.table;
  const uint32_t nfeed = (uint32_t)a.nfeed, npairs = (uint32_t)a.npairs, ntime = (uint32_t)a.ntime, nf = (uint32_t)a.nf;
  const uint32_t nmem = npairs ? (uint32_t)a.class_off_host[npairs] : 0u;
  const int64_t ntiles = ((int64_t)ntime + TT - 1) / TT;
  const int64_t cells = (int64_t)a.nreal * nf * ntiles;
  const std::vector<int> ychunk = dm_stack_chunks(a.npairs, a.class_off_host, cells);
  const std::vector<int> gchunk = dm_redcal_chunks(a.nfeed, tb.inc_off.data(), cells);
  const int64_t nyc = (int64_t)ychunk.size() - 1, ngc = (int64_t)gchunk.size() - 1;
  if (cells * nyc >= (1LL << 31) || cells * ngc >= (1LL << 31) || (int64_t)a.nreal * nf >= (1LL << 31))
    return dm_refuse(ctx, RC_WHO, "too many workgroups for one launch");
  const size_t nsamp = (size_t)a.nreal * nf * ntime, ng = nsamp * nfeed;
  const size_t lds = (size_t)nfeed * TT * sizeof(cplx), lds_chi = lds + (size_t)RC_NW * TT * sizeof(double);
  if (lds_chi > (size_t)DM_GAIN_LDS_BYTES) return dm_refuse(ctx, RC_WHO, "the g tile and the chi^2 sums do not fit in LDS");
  // tables
  const int* off = dm_ws_upload(ctx, std::vector<int>(a.class_off_host, a.class_off_host + npairs + 1));
  const int2* mem = reinterpret_cast<const int2*>(
      dm_ws_upload(ctx, std::vector<int>(a.members_host, a.members_host + 2 * (size_t)nmem)));
  const int* ych = dm_ws_upload(ctx, ychunk);
  const int* gch = dm_ws_upload(ctx, gchunk);
  const double* yfac = dm_ws_upload(ctx, tb.yfac);
  const double* gfac = dm_ws_upload(ctx, tb.gfac);
  const int* inc_off = dm_ws_upload(ctx, tb.inc_off);
  const int4* inc = reinterpret_cast<const int4*>(dm_ws_upload(ctx, tb.inc));
  // the second gain buffer, two sets of state and step words, the counters of the host's checks
  cplx* gws = dm_ws_alloc_t<cplx>(ctx, ng ? ng : 1);
  const int nslots = dm_poll_slots(a.maxiter);
  const size_t words = 2 * nsamp * sizeof(unsigned long long) + 2 * nsamp * sizeof(int) + (size_t)nslots * sizeof(int);
  char* state = reinterpret_cast<char*>(dm_ws_alloc(ctx, words));
  if (!off || !mem || !ych || !gch || !yfac || !gfac || !inc_off || !inc || !gws || !state) return DM_ENOMEM;
  unsigned long long* sb[2] = {reinterpret_cast<unsigned long long*>(state),
                               reinterpret_cast<unsigned long long*>(state) + nsamp};
  int* st[2] = {reinterpret_cast<int*>(sb[1] + nsamp), reinterpret_cast<int*>(sb[1] + nsamp) + nsamp};
  int* pending = st[1] + nsamp;
  DM_HIP(ctx, hipMemsetAsync(state, 0, words, ctx->stream));
  // iteration k reads G[(k - 1) & 1] and writes G[k & 1]: the buffer that iteration maxiter writes is the caller's
  cplx* G[2];
  G[a.maxiter & 1] = a.g;
  G[(a.maxiter & 1) ^ 1] = gws;
  DM_TRY(dm_lds_attr(ctx, &redcal_y_kernel<TT, HAS_W>, lds));
  DM_TRY(dm_lds_attr(ctx, &redcal_g_kernel<TT, HAS_W>, lds));
  DM_TRY(dm_lds_attr(ctx, &redcal_chi2_kernel<TT, HAS_W>, lds_chi));
  if (ng) {
    DM_PLAUNCH(ctx, DM_PROF_UTIL, redcal_init_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, a.g0,
               G[0], (unsigned long long)ng);
    DM_HIP(ctx, hipGetLastError());
  }
  const dim3 ygrid((unsigned)(cells * nyc)), ggrid((unsigned)(cells * ngc)), block(RC_NW * 64);
  auto y_pass = [&](int k, int last, int* count) -> int {
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (redcal_y_kernel<TT, HAS_W>), ygrid, block, lds, ctx->stream, a.vis, a.w,
               (const cplx*)G[(k - 1) & 1], yfac, a.y, off, mem, ych, (const int*)st[(k - 1) & 1], st[k & 1],
               (const unsigned long long*)sb[(k - 1) & 1], sb[k & 1], a.iters, a.step, count, nfeed, npairs, nmem, ntime,
               (uint32_t)ntiles, (uint32_t)nyc, nf, a.w_each, a.vstride, a.tol, k, last);
    DM_HIP(ctx, hipGetLastError());
    return DM_OK;
  };
  const dm_poll_result run = dm_poll_iterate(ctx, a.maxiter, pending, [&](int k, int* count) -> int {
    DM_TRY(y_pass(k, 0, count));
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (redcal_g_kernel<TT, HAS_W>), ggrid, block, lds, ctx->stream, a.vis, a.w,
               (const cplx*)G[(k - 1) & 1], G[k & 1], gfac, (const cplx*)a.y, inc_off, inc, gch, (const int*)st[k & 1],
               sb[k & 1], nfeed, npairs, nmem, ntime, (uint32_t)ntiles, (uint32_t)ngc, nf, a.w_each, a.vstride, a.damping);
    DM_HIP(ctx, hipGetLastError());
    return DM_OK;
  });
  DM_TRY(run.rc);
  // every sample was done (state 2) when the host stopped early; otherwise close the books of the last iteration
  if (!run.all_done) DM_TRY(y_pass(a.maxiter + 1, 1, nullptr));
  DM_PLAUNCH(ctx, DM_PROF_UTIL, (redcal_chi2_kernel<TT, HAS_W>), dim3((unsigned)cells), block, lds_chi, ctx->stream, a.vis,
             a.w, (const cplx*)a.g, gfac, (const cplx*)a.y, off, mem, a.chi2, nfeed, npairs, nmem, ntime, (uint32_t)ntiles, nf,
             a.w_each, a.vstride);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // namespace

extern "C" int dm_redcal_solve(dm_ctx* ctx, int nreal, int w_nreal, int nf, int nfeed, int npairs, int ntime,
                               const int* class_off_host, const int* members_host, const void* vis_dev, const double* w_dev,
                               const double* feed_weight_host, const void* g0_dev, double damping, double tol, int maxiter,
                               void* g_dev, void* y_dev, int* iters_dev, double* step_dev, double* chi2_dev,
                               int64_t vis_rstride) {
  if (!ctx) return DM_EARG;
  const bool has_w = w_dev != nullptr;
  const std::string bad = dm_pair_args_check(nreal, nf, nfeed, npairs, ntime, vis_rstride, has_w ? &w_nreal : nullptr, nullptr,
                                             class_off_host, members_host, true, feed_weight_host);
  if (!bad.empty()) return dm_refuse(ctx, RC_WHO, bad);
  const std::string worse = dm_redcal_args_check(damping, tol, maxiter);
  if (!worse.empty()) return dm_refuse(ctx, RC_WHO, worse);
  const int64_t nmem = npairs > 0 ? class_off_host[npairs] : 0;
  const uint64_t vrow = (uint64_t)nf * nmem * ntime;
  if (vis_rstride == 0) vis_rstride = (int64_t)vrow;
  if ((uint64_t)vis_rstride < vrow) return dm_refuse(ctx, RC_WHO, "vis_rstride is shorter than a realisation");
  if (nreal == 0 || nf == 0 || ntime == 0) return DM_OK;
  const uint64_t nsamp = (uint64_t)nreal * nf * ntime;
  if ((nmem > 0 && !vis_dev) || (nfeed > 0 && !g_dev) || (npairs > 0 && !y_dev) || !iters_dev || !step_dev || !chi2_dev)
    return dm_refuse(ctx, RC_WHO, "null pointer with work to do");
  // outputs against the inputs and against each other, on whole spans
  const dm_span in[3] = {{vis_dev, 16 * ((uint64_t)(nreal - 1) * vis_rstride + vrow), "vis"},
                      {w_dev, 8 * (uint64_t)(has_w ? w_nreal : 0) * vrow, "w"},
                      {g0_dev, g0_dev ? 16 * nsamp * nfeed : 0, "g0"}};
  const dm_span out[5] = {{g_dev, 16 * nsamp * nfeed, "g"}, {y_dev, 16 * nsamp * npairs, "y"}, {iters_dev, 4 * nsamp, "iters"},
                       {step_dev, 8 * nsamp, "step"}, {chi2_dev, 8 * nsamp, "chi2"}};
  const std::string shared = dm_spans_shared(in, 3, out, 5);
  if (!shared.empty()) return dm_refuse(ctx, RC_WHO, shared);
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  const dm_redcal_table table = dm_redcal_build(nfeed, npairs, class_off_host, members_host, feed_weight_host);
  redcal_args a;
  a.vis = static_cast<const cplx*>(vis_dev), a.g0 = static_cast<const cplx*>(g0_dev), a.w = w_dev;
  a.g = static_cast<cplx*>(g_dev), a.y = static_cast<cplx*>(y_dev);
  a.iters = iters_dev, a.step = step_dev, a.chi2 = chi2_dev;
  a.class_off_host = class_off_host, a.members_host = members_host, a.table = &table;
  a.nreal = nreal, a.nf = nf, a.nfeed = nfeed, a.npairs = npairs, a.ntime = ntime, a.maxiter = maxiter;
  a.w_each = has_w && w_nreal == nreal && nreal > 1 ? 1u : 0u;
  a.vstride = (unsigned long long)vis_rstride;
  a.damping = damping, a.tol = tol;
#define DM_REDCAL_CASE(TT) \
  case TT:                 \
    return has_w ? redcal_run<TT, true>(ctx, a) : redcal_run<TT, false>(ctx, a)
  switch (dm_gain_tile(nfeed)) {
    DM_REDCAL_CASE(16);
    DM_REDCAL_CASE(8);
    DM_REDCAL_CASE(4);
    DM_REDCAL_CASE(2);
    DM_REDCAL_CASE(1);
  }
#undef DM_REDCAL_CASE
  return DM_EARG;
}
