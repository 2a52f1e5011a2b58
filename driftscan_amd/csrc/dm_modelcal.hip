// dm_modelcal.hip — sky-model gain calibration: dm_modelcal_solve finds the per-feed gains g that
// minimise chi^2 = sum_{t in q} sum_m omega_m(t) |V_m(t) - g_i conj(g_j) M_c(t)|^2 against a given stacked model M, every
// (realisation, frequency, solution interval q of L samples) a problem of its own, by the damped StEFCal fixed point.
//
// An iteration is ONE kernel on the context's stream:
//   modelcal_g_kernel   feed-major over the incidence table of dm_redcal_table.h built without the "fewer than two" rule:
//                       a workgroup takes one (realisation, frequency, interval, chunk of feeds), stages the gains of ALL
//                       feeds of that interval in LDS (16 nfeed bytes: one gain per feed), a wave takes the feeds wave,
//                       wave + 8, ... of the chunk, and its 64 lanes run over the flattened (incidence, sample of the
//                       interval) index with the sample fastest, so that vis, w and the model are read in runs of
//                       contiguous samples; the lanes are joined by the xor butterfly.  The new gains go to the other of
//                       two buffers [interval][feed]: other workgroups still read the old ones.
//   modelcal_close_kernel  the books of the last iteration, gweight (the denominator of every feed at the returned g, by the
//                       same walk) and g in the caller's layout per chunk of feeds, and chi^2 in the workgroup of chunk 0.
// The state of an interval (0 iterating, 1 converged and owed the copy of its gains to the other buffer, 2 done or not
// asked for, 3 out of iterations) is read from the words the previous launch left and written to a second set; the step
// of an interval is the maximum over its feeds, joined across waves and workgroups by an integer atomicMax on the bit
// pattern of a non-negative double.  Iteration k reads the step words k - 1, joins into the words k and clears the words
// k + 1 (mod 3), so no launch reads or clears what it joins into.  There is no floating-point atomic, and every sum lives
// inside one wave in an order that (d_a, length of the interval) fix.
//
// The design is for intervals of 16 samples and more (a transit lasts many samples).  Shorter ones are correct but slow:
// at L = 1 neighbouring lanes read vis, w and the model ntime elements apart, one 16-byte element per 128-byte line.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_modelcal_table.h"
#include "../../include/driftmi.h"

#include <vector>

namespace {

constexpr int MC_NW = 8;       // waves per workgroup, as the gain step of section 4.18

// The state of an interval entering iteration `iter`, from its state and its step after iteration iter - 1.  Before the
// first iteration the words hold 0 (to solve) or 2 (not asked for).  `last`: the closing pass.
__device__ __forceinline__ int modelcal_state(int in, double step, double tol, int iter, int last) {
  if (iter == 1 || in != 0) return in == 1 ? 2 : in;
  return step < tol ? 1 : (last ? 3 : 0);
}

// Both gain buffers [cell][feed] from g0 (nreal, nf, nfeed, nint), or ones; the first state words from `active`.
__global__ __launch_bounds__(256) void modelcal_init_kernel(const cplx* __restrict__ g0, const int* __restrict__ active,
                                                            cplx* __restrict__ ga, cplx* __restrict__ gb,
                                                            int* __restrict__ st, unsigned long long ng,
                                                            unsigned long long ncells, uint32_t nfeed, uint32_t nint,
                                                            uint32_t nf) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < ng) {
    const size_t cell = e / nfeed, a = e - cell * nfeed;
    const size_t rf = cell / nint, q = cell - rf * nint;
    const cplx v = g0 ? dm_ldg(g0, (rf * nfeed + a) * nint + q) : make_double2(1.0, 0.0);
    dm_stg(ga, e, v);
    dm_stg(gb, e, v);
  }
  if (e < ncells) {
    const size_t rf = e / nint, q = e - rf * nint;
    st[e] = active && active[(rf % nf) * nint + q] == 0 ? 2 : 0;
  }
}

struct mc_rows {
  size_t vrow, wrow, mrow;   // element offsets of sample 0 of the interval in member row 0 / class row 0
  uint32_t ntime, lq;        // the length of a row, the samples of this interval
  uint32_t k0, s0, dq, dr;   // this lane's first (incidence, sample) and its advance by 64 elements
};

// The sums of feed a over its incidences [k0, k1) and the samples of the interval, every lane holding the wave's total:
// d = sum omega |z|^2 and, with NUM, n = sum omega V conj(z) (side 0: z = conj(g_j) M) + sum omega conj(V) conj(z')
// (side 1: z' = conj(g_i M)).
template <bool HAS_W, bool NUM>
__device__ __forceinline__ void modelcal_feed_sums(const cplx* __restrict__ vis, const double* __restrict__ w,
                                                   const cplx* __restrict__ model, const double* __restrict__ fac,
                                                   const int4* __restrict__ inc, const cplx* gl, const mc_rows& rw, int k0,
                                                   int k1, double& nx, double& ny, double& d) {
  nx = 0.0, ny = 0.0, d = 0.0;
  int k = k0 + (int)rw.k0;
  uint32_t s = rw.s0;
  while (k < k1) {
    const int4 e = inc[k];                                       // member row, partner, class, side
    const size_t at = (size_t)e.x * rw.ntime + s;
    double we = dm_ldg(fac, (size_t)e.x);
    if constexpr (HAS_W) we *= dm_ldg(w, rw.wrow + at);
    cplx mc = dm_ldg(model, rw.mrow + (size_t)e.z * rw.ntime + s);
    const cplx gp = gl[e.y];
    if constexpr (NUM) {
      cplx v = dm_ldg(vis, rw.vrow + at);
      if (e.w) v.y = -v.y;                                       // side 1: conj(V) g_i M
      else mc.y = -mc.y;                                         // side 0: V g_j conj(M)
      const cplx p = cmul(cmul(gp, mc), v);
      nx = fma(we, p.x, nx);
      ny = fma(we, p.y, ny);
    }
    d = fma(we, cabs2(gp) * cabs2(mc), d);
    s += rw.dr, k += (int)rw.dq;
    if (s >= rw.lq) s -= rw.lq, ++k;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    if constexpr (NUM) {
      nx += __shfl_xor(nx, o, 64);
      ny += __shfl_xor(ny, o, 64);
    }
    d += __shfl_xor(d, o, 64);
  }
}

__device__ __forceinline__ mc_rows modelcal_rows(uint32_t r, uint32_t f, uint32_t q, uint32_t nf, uint32_t nmem,
                                                 uint32_t npairs, uint32_t ntime, uint32_t L, uint32_t w_each,
                                                 uint32_t m_each, unsigned long long vstride) {
  mc_rows rw;
  const size_t t0 = (size_t)q * L;
  rw.ntime = ntime;
  rw.lq = ntime - (uint32_t)t0 < L ? ntime - (uint32_t)t0 : L;
  rw.vrow = (size_t)r * vstride + (size_t)f * nmem * ntime + t0;
  rw.wrow = ((size_t)(w_each ? r : 0u) * nf + f) * nmem * ntime + t0;
  rw.mrow = ((size_t)(m_each ? r : 0u) * nf + f) * npairs * ntime + t0;
  const uint32_t lane = threadIdx.x & 63u;
  rw.k0 = lane / rw.lq, rw.s0 = lane - rw.k0 * rw.lq;
  rw.dq = 64u / rw.lq, rw.dr = 64u - rw.dq * rw.lq;
  return rw;
}

// g_a <- (1 - delta) g_a + delta n / d over the incidences of feed a and the samples of the interval, g_a kept where
// d == 0; the step |delta g_a| / |g_a| of the interval goes into sb_out by atomicMax.  The workgroup of chunk 0 keeps the
// books.  An interval of state 1 only has its gains copied to the other buffer; states 2 and 3 cost the read of one word.
template <bool HAS_W>
__global__ __launch_bounds__(MC_NW * 64) void modelcal_g_kernel(
    const cplx* __restrict__ vis, const double* __restrict__ w, const cplx* __restrict__ model, const cplx* __restrict__ g,
    cplx* __restrict__ gnew, const double* __restrict__ fac, const int* __restrict__ inc_off, const int4* __restrict__ inc,
    const int* __restrict__ chunk_off, const int* st_in, int* st_out, const unsigned long long* sb_in,
    unsigned long long* sb_out, unsigned long long* sb_next, int* __restrict__ iters, double* __restrict__ step, int* pending,
    uint32_t nfeed, uint32_t npairs, uint32_t nmem, uint32_t ntime, uint32_t nint, uint32_t L, uint32_t nchunks, uint32_t nf,
    uint32_t w_each, uint32_t m_each, unsigned long long vstride, double damping, double tol, int iter) {
  extern __shared__ cplx gl[];                                   // [nfeed]
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const int in = st_in[cell];
  const double stp = in == 0 && iter > 1 ? __longlong_as_double((long long)sb_in[cell]) : 0.0;
  const int now = modelcal_state(in, stp, tol, iter, 0);
  if (chunk == 0 && threadIdx.x == 0) {
    st_out[cell] = now;
    sb_next[cell] = 0ull;
    if (in == 0 && now != 0) {
      iters[cell] = iter - 1;
      dm_stg(step, (size_t)cell, stp);
    }
    if (pending && now < 2) atomicAdd(pending, 1);
  }
  if (now >= 2) return;
  const cplx* gsrc = g + (size_t)cell * nfeed;
  for (uint32_t a = threadIdx.x; a < nfeed; a += MC_NW * 64) gl[a] = dm_ldg(gsrc, (size_t)a);
  __syncthreads();
  const bool act = now == 0;
  const uint32_t rf = cell / nint, q = cell - rf * nint;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const mc_rows rw = modelcal_rows(r, f, q, nf, nmem, npairs, ntime, L, w_each, m_each, vstride);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool lane0 = (threadIdx.x & 63u) == 0;
  const double keep = 1.0 - damping;
  double smax = 0.0;
  const int a1 = chunk_off[chunk + 1];
  for (int a = chunk_off[chunk] + (int)wave; a < a1; a += MC_NW) {
    const cplx ga = gl[a];
    cplx gn = ga;
    if (act) {
      double nx, ny, d;
      modelcal_feed_sums<HAS_W, true>(vis, w, model, fac, inc, gl, rw, inc_off[a], inc_off[a + 1], nx, ny, d);
      if (d > 0.0) {
        gn.x = keep * ga.x + damping * (nx / d);
        gn.y = keep * ga.y + damping * (ny / d);
        const double dx = gn.x - ga.x, dy = gn.y - ga.y;
        const double s = dx == 0.0 && dy == 0.0 ? 0.0 : sqrt((dx * dx + dy * dy) / cabs2(ga));
        if (s > smax || s != s) smax = s;                        // (a NaN stays: the interval is then never called converged)
      }
    }
    if (lane0) dm_stg(gnew, (size_t)cell * nfeed + (uint32_t)a, gn);
  }
  if (lane0 && act) atomicMax(&sb_out[cell], (unsigned long long)__double_as_longlong(smax) & 0x7fffffffffffffffull);
}

// After the last iteration `iter - 1`: the books of the intervals that still iterated, g in the caller's layout and
// gweight for the feeds of the chunk, and in the workgroup of chunk 0 chi^2 = sum omega |V - g_i conj(g_j) M|^2: wave v
// takes the members [nmem v / 8, nmem (v + 1) / 8) with the walk of the gain step, and the eight waves' sums are added
// in their order through LDS.  An interval that was not asked for gets iters, step, chi2 and gweight 0.
template <bool HAS_W>
__global__ __launch_bounds__(MC_NW * 64) void modelcal_close_kernel(
    const cplx* __restrict__ vis, const double* __restrict__ w, const cplx* __restrict__ model, const cplx* __restrict__ g,
    const double* __restrict__ fac, const int* __restrict__ inc_off, const int4* __restrict__ inc,
    const int* __restrict__ chunk_off, const int4* __restrict__ members, const int* __restrict__ st_in,
    const unsigned long long* __restrict__ sb_in, const int* __restrict__ active, cplx* __restrict__ g_out,
    int* __restrict__ iters, double* __restrict__ step, double* __restrict__ chi2, double* __restrict__ gweight,
    uint32_t nfeed, uint32_t npairs, uint32_t nmem, uint32_t ntime, uint32_t nint, uint32_t L, uint32_t nchunks, uint32_t nf,
    uint32_t w_each, uint32_t m_each, unsigned long long vstride, int iter) {
  extern __shared__ cplx gl[];                                   // [nfeed], then MC_NW doubles
  double* red = reinterpret_cast<double*>(gl + nfeed);
  const uint32_t cell = blockIdx.x / nchunks, chunk = blockIdx.x - cell * nchunks;
  const uint32_t rf = cell / nint, q = cell - rf * nint;
  const uint32_t r = rf / nf, f = rf - r * nf;
  const bool idle = active && active[(size_t)f * nint + q] == 0;
  if (chunk == 0 && threadIdx.x == 0) {
    if (idle) {
      iters[cell] = 0;
      dm_stg(step, (size_t)cell, 0.0);
    } else if (st_in[cell] == 0) {                               // iterated to the end: converged by its last step or not
      iters[cell] = iter - 1;
      dm_stg(step, (size_t)cell, __longlong_as_double((long long)sb_in[cell]));
    }
  }
  const cplx* gsrc = g + (size_t)cell * nfeed;
  for (uint32_t a = threadIdx.x; a < nfeed; a += MC_NW * 64) gl[a] = dm_ldg(gsrc, (size_t)a);
  __syncthreads();
  const mc_rows rw = modelcal_rows(r, f, q, nf, nmem, npairs, ntime, L, w_each, m_each, vstride);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool lane0 = (threadIdx.x & 63u) == 0;
  const int a1 = chunk_off[chunk + 1];
  for (int a = chunk_off[chunk] + (int)wave; a < a1; a += MC_NW) {
    double nx = 0.0, ny = 0.0, d = 0.0;
    if (!idle) modelcal_feed_sums<HAS_W, false>(vis, w, model, fac, inc, gl, rw, inc_off[a], inc_off[a + 1], nx, ny, d);
    if (lane0) {
      const size_t at = ((size_t)rf * nfeed + (uint32_t)a) * nint + q;
      dm_stg(g_out, at, gl[a]);
      dm_stg(gweight, at, d);
    }
  }
  if (chunk != 0) return;
  double acc = 0.0;
  if (!idle) {
    const int m1 = (int)((unsigned long long)nmem * (wave + 1) / MC_NW);
    int k = (int)((unsigned long long)nmem * wave / MC_NW) + (int)rw.k0;
    uint32_t s = rw.s0;
    while (k < m1) {
      const size_t at = (size_t)k * ntime + s;
      double we = dm_ldg(fac, (size_t)k);
      if constexpr (HAS_W) we *= dm_ldg(w, rw.wrow + at);
      const int4 m = members[k];                                 // i, j, class
      const cplx mc = dm_ldg(model, rw.mrow + (size_t)m.z * ntime + s);
      const cplx e = csub(dm_ldg(vis, rw.vrow + at), cmul(cmulc(gl[m.x], gl[m.y]), mc));
      acc = fma(we, cabs2(e), acc);
      s += rw.dr, k += (int)rw.dq;
      if (s >= rw.lq) s -= rw.lq, ++k;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (lane0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = red[0];
#pragma unroll
    for (int v = 1; v < MC_NW; ++v) sum += red[v];
    dm_stg(chi2, (size_t)cell, sum);
  }
}

constexpr const char* MC_WHO = "dm_modelcal_solve";

struct modelcal_args {
  const cplx *vis, *model, *g0;
  const double* w;
  const int* active;
  cplx* g;
  int* iters;
  double *step, *chi2, *gweight;
  const int* class_off_host;
  const int* members_host;
  const dm_redcal_table* table;
  int nreal, nf, nfeed, npairs, ntime, interval, maxiter;
  uint32_t w_each, m_each;
  unsigned long long vstride;
  double damping, tol;
};

template <bool HAS_W>
int modelcal_run(dm_ctx* ctx, const modelcal_args& a) {
  const dm_redcal_table& tb = *a.table;
  const uint32_t nfeed = (uint32_t)a.nfeed, npairs = (uint32_t)a.npairs, ntime = (uint32_t)a.ntime, nf = (uint32_t)a.nf;
  const uint32_t nmem = npairs ? (uint32_t)a.class_off_host[npairs] : 0u;
  const int64_t nint = dm_modelcal_nint(a.ntime, a.interval);
  const int64_t cells = (int64_t)a.nreal * nf * nint;
  const std::vector<int> gchunk = dm_redcal_chunks(a.nfeed, tb.inc_off.data(), cells);
  const int64_t ngc = (int64_t)gchunk.size() - 1;
  if (cells * ngc >= (1LL << 31)) return dm_refuse(ctx, MC_WHO, "too many workgroups for one launch");
  const size_t ncells = (size_t)cells, ng = ncells * nfeed;
  const size_t lds = (size_t)nfeed * sizeof(cplx), lds_close = lds + (size_t)MC_NW * sizeof(double);
  // tables: the factors and incidences without the "fewer than two" rule, the members with their class
  const int* gch = dm_ws_upload(ctx, gchunk);
  const double* fac = dm_ws_upload(ctx, tb.gfac);
  const int* inc_off = dm_ws_upload(ctx, tb.inc_off);
  const int4* inc = reinterpret_cast<const int4*>(dm_ws_upload(ctx, tb.inc));
  std::vector<int> mrow(4 * (size_t)nmem, 0);
  for (uint32_t c = 0; c < npairs; ++c)
    for (int k = a.class_off_host[c]; k < a.class_off_host[c + 1]; ++k)
      mrow[4 * (size_t)k] = a.members_host[2 * (size_t)k], mrow[4 * (size_t)k + 1] = a.members_host[2 * (size_t)k + 1],
                       mrow[4 * (size_t)k + 2] = (int)c;
  const int4* mem = reinterpret_cast<const int4*>(dm_ws_upload(ctx, mrow));
  // two gain buffers [cell][feed], three sets of step words, two of state words, the counters of the host's checks
  cplx* gws = dm_ws_alloc_t<cplx>(ctx, 2 * ng + 1);
  const int nslots = dm_poll_slots(a.maxiter);
  const size_t words = 3 * ncells * sizeof(unsigned long long) + 2 * ncells * sizeof(int) + (size_t)nslots * sizeof(int);
  char* state = reinterpret_cast<char*>(dm_ws_alloc(ctx, words));
  if (!gch || !fac || !inc_off || !inc || !mem || !gws || !state) return DM_ENOMEM;
  cplx* G[2] = {gws, gws + ng};
  unsigned long long* sb[3];
  for (int b = 0; b < 3; ++b) sb[b] = reinterpret_cast<unsigned long long*>(state) + (size_t)b * ncells;
  int* st[2] = {reinterpret_cast<int*>(sb[2] + ncells), reinterpret_cast<int*>(sb[2] + ncells) + ncells};
  int* pending = st[1] + ncells;
  DM_HIP(ctx, hipMemsetAsync(state, 0, words, ctx->stream));
  const size_t ninit = ng > ncells ? ng : ncells;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, modelcal_init_kernel, dim3((unsigned)((ninit + 255) / 256)), dim3(256), 0, ctx->stream, a.g0,
             a.active, G[0], G[1], st[0], (unsigned long long)ng, (unsigned long long)ncells, nfeed, (uint32_t)nint, nf);
  DM_HIP(ctx, hipGetLastError());
  const dim3 grid((unsigned)(cells * ngc)), block(MC_NW * 64);
  // iteration k reads G, st and sb of k - 1, writes G and st of k, joins the steps into sb of k and clears sb of k + 1
  const dm_poll_result run = dm_poll_iterate(ctx, a.maxiter, pending, [&](int k, int* count) -> int {
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (modelcal_g_kernel<HAS_W>), grid, block, lds, ctx->stream, a.vis, a.w, a.model,
               (const cplx*)G[(k - 1) & 1], G[k & 1], fac, inc_off, inc, gch, (const int*)st[(k - 1) & 1], st[k & 1],
               (const unsigned long long*)sb[(k - 1) % 3], sb[k % 3], sb[(k + 1) % 3], a.iters, a.step, count, nfeed, npairs,
               nmem, ntime, (uint32_t)nint, (uint32_t)a.interval, (uint32_t)ngc, nf, a.w_each, a.m_each, a.vstride,
               a.damping, a.tol, k);
    DM_HIP(ctx, hipGetLastError());
    return DM_OK;
  });
  DM_TRY(run.rc);
  const int k_last = run.k_last;
  // both gain buffers hold the gains of every finished interval; the one iteration k_last wrote also holds the rest
  DM_PLAUNCH(ctx, DM_PROF_UTIL, (modelcal_close_kernel<HAS_W>), grid, block, lds_close, ctx->stream, a.vis, a.w, a.model,
             (const cplx*)G[k_last & 1], fac, inc_off, inc, gch, mem, (const int*)st[k_last & 1],
             (const unsigned long long*)sb[k_last % 3], a.active, a.g, a.iters, a.step, a.chi2, a.gweight, nfeed, npairs, nmem,
             ntime, (uint32_t)nint, (uint32_t)a.interval, (uint32_t)ngc, nf, a.w_each, a.m_each, a.vstride, k_last + 1);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // namespace

extern "C" int dm_modelcal_solve(dm_ctx* ctx, int nreal, int w_nreal, int m_nreal, int nf, int nfeed, int npairs, int ntime,
                                 int interval, const int* class_off_host, const int* members_host, const void* vis_dev,
                                 const void* model_dev, const double* w_dev, const double* feed_weight_host,
                                 const void* g0_dev, const int* active_dev, double damping, double tol, int maxiter,
                                 void* g_dev, int* iters_dev, double* step_dev, double* chi2_dev, double* gweight_dev,
                                 int64_t vis_rstride) {
  if (!ctx) return DM_EARG;
  const bool has_w = w_dev != nullptr;
  const std::string bad = dm_pair_args_check(nreal, nf, nfeed, npairs, ntime, vis_rstride, has_w ? &w_nreal : nullptr, &m_nreal,
                                             class_off_host, members_host, true, feed_weight_host);
  if (!bad.empty()) return dm_refuse(ctx, MC_WHO, bad);
  const std::string worse = dm_modelcal_args_check(nfeed, interval, damping, tol, maxiter);
  if (!worse.empty()) return dm_refuse(ctx, MC_WHO, worse);
  const int64_t nmem = npairs > 0 ? class_off_host[npairs] : 0;
  const uint64_t vrow = (uint64_t)nf * nmem * ntime;
  if (vis_rstride == 0) vis_rstride = (int64_t)vrow;
  if ((uint64_t)vis_rstride < vrow) return dm_refuse(ctx, MC_WHO, "vis_rstride is shorter than a realisation");
  if (nreal == 0 || nf == 0 || ntime == 0) return DM_OK;
  const uint64_t nint = (uint64_t)dm_modelcal_nint(ntime, interval);
  if (nint * (uint64_t)nreal * nf >= (1ull << 31)) return dm_refuse(ctx, MC_WHO, "too many intervals for one call");
  const uint64_t ncell = (uint64_t)nreal * nf * nint;
  if ((nmem > 0 && (!vis_dev || !model_dev)) || (nfeed > 0 && (!g_dev || !gweight_dev)) || !iters_dev || !step_dev ||
      !chi2_dev)
    return dm_refuse(ctx, MC_WHO, "null pointer with work to do");
  // outputs against the inputs and against each other, on whole spans
  const dm_span in[5] = {{vis_dev, 16 * ((uint64_t)(nreal - 1) * vis_rstride + vrow), "vis"},
                      {model_dev, 16 * (uint64_t)m_nreal * nf * npairs * ntime, "model"},
                      {w_dev, 8 * (uint64_t)(has_w ? w_nreal : 0) * vrow, "w"},
                      {g0_dev, g0_dev ? 16 * ncell * nfeed : 0, "g0"},
                      {active_dev, active_dev ? 4 * (uint64_t)nf * nint : 0, "active"}};
  const dm_span out[5] = {{g_dev, 16 * ncell * nfeed, "g"}, {iters_dev, 4 * ncell, "iters"}, {step_dev, 8 * ncell, "step"},
                       {chi2_dev, 8 * ncell, "chi2"}, {gweight_dev, 8 * ncell * nfeed, "gweight"}};
  const std::string shared = dm_spans_shared(in, 5, out, 5);
  if (!shared.empty()) return dm_refuse(ctx, MC_WHO, shared);
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  const dm_redcal_table table = dm_redcal_build(nfeed, npairs, class_off_host, members_host, feed_weight_host, 1);
  modelcal_args a;
  a.vis = static_cast<const cplx*>(vis_dev), a.model = static_cast<const cplx*>(model_dev);
  a.g0 = static_cast<const cplx*>(g0_dev), a.w = w_dev, a.active = active_dev;
  a.g = static_cast<cplx*>(g_dev), a.iters = iters_dev, a.step = step_dev, a.chi2 = chi2_dev, a.gweight = gweight_dev;
  a.class_off_host = class_off_host, a.members_host = members_host, a.table = &table;
  a.nreal = nreal, a.nf = nf, a.nfeed = nfeed, a.npairs = npairs, a.ntime = ntime, a.interval = interval, a.maxiter = maxiter;
  a.w_each = has_w && w_nreal == nreal && nreal > 1 ? 1u : 0u;
  a.m_each = m_nreal == nreal && nreal > 1 ? 1u : 0u;
  a.vstride = (unsigned long long)vis_rstride;
  a.damping = damping, a.tol = tol;
  return has_w ? modelcal_run<true>(ctx, a) : modelcal_run<false>(ctx, a);
}
