// dm_toeplitz.hip — batched Hermitian positive-definite Toeplitz systems by the normalised Levinson recursion (DESIGN.md
// section 4.16): the weighted least-squares m-modes of flagged timestreams are one such system of order 2 mmax + 1 per
// (frequency, baseline).  A system is given by its first column (n values, not n^2) and solved in 2 n^2 complex
// multiply-adds per right-hand side; the whole recursion of one system lives in the LDS of one CU.
#include "dm_common.h"
#include "dm_toeplitz_args.h"
#include "../../include/driftmi.h"

namespace {

__device__ __forceinline__ cplx cfma(cplx a, cplx b, cplx acc) {   // acc + a b
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
  return acc;
}
__device__ __forceinline__ cplx cfmac(cplx a, cplx b, cplx acc) {  // acc + a conj(b)
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(a.y, b.y, acc.x);
  acc.y = fma(a.y, b.x, acc.y);
  acc.y = fma(-a.x, b.y, acc.y);
  return acc;
}

// Sum over the 64 lanes, the same bits in every lane: lane ^ 1 and lane ^ 2 as DPP quad permutations, then the mirrors of
// a half row and of a row (once the quads, then the half rows hold one value each, these pair every lane with the other
// quad, the other half row: every lane adds the same two numbers), then lane ^ 16 and lane ^ 32 through the LDS crossbar.
__device__ __forceinline__ double tz_wave_sum(double v) {
  v += dm_dpp_f64<0xB1>(v);    // quad_perm:[1,0,3,2]
  v += dm_dpp_f64<0x4E>(v);    // quad_perm:[2,3,0,1]
  v += dm_dpp_f64<0x141>(v);   // row_half_mirror
  v += dm_dpp_f64<0x140>(v);   // row_mirror
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// One system per workgroup of NT threads (64: one wave, no workgroup barrier is left in the code — the compiler drops
// it for a workgroup of one wave; 256: four waves).  One wave per system gives the higher throughput up to n of about
// 768 (more systems per CU, no barriers) and the longer time for a batch that does not fill the device from n of about
// 384 on; the switch is at 384 (measured).
// LDS, all dynamic and 16-byte aligned: r[n] | f[n] | x_0[n] .. x_{nrhs-1}[n] | red[NT / 64 + 1][1 + nrhs].  f and the
// x_j are the vectors 0 and 1 + j of `vec`; x_j holds b'_j from element k on until step k has used it.
//
// Step k: (A) every vector's dot product sum_{i<k} r[k-i] vec_v[i]: a thread adds its elements i = tid, tid + NT, ..
// in that order (four vectors at a time share the read of r), a wave adds its lanes by tz_wave_sum, lane 0 writes
// the wave's partial to red[wave][v]; b'_k of every right-hand side goes to the last row of red.  Barrier.  (B) every
// thread adds the partials wave 0, 1, .. and so holds the same gamma, beta and coefficients; the thread of i updates
// the elements i and k - i of f and of every x_j in place.  Barrier.  The order of every sum is a function of (n, k)
// alone, so a system has the same bits alone, in any batch and at any position.
//
// DIAG (dm_toeplitz_solve_diag): after the last step f solves T' f = beta e_0, so f / (beta c_0) is the first column of
// the inverse and the Gohberg-Semencul formula gives its diagonal as one prefix sum, d_i = (sum_{j<=i} g_j) / (beta c_0)
// with g_j = |f_j|^2 - |f_{n-j}|^2 and f_n := 0.  |f_i|^2 goes into the space of r (dead by then); the thread of
// tid owns the elements tid C .. tid C + C - 1, C = ceil(n / NT): it adds its g in index order, the wave scans the
// threads' sums (tz_wave_scan), every thread adds the totals of the waves before its own in wave order and then walks
// its elements again.  The order is a function of n alone.  A failed system gets zeros.  nrhs = 0 is allowed here.
__device__ __forceinline__ double tz_wave_scan(double v, uint32_t lane) {   // inclusive, over the lanes 0 .. lane
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

template <int NT, bool DIAG>
__global__ __launch_bounds__(NT) void toeplitz_levinson_kernel(const cplx* __restrict__ col, cplx* __restrict__ b,
                                                               int* __restrict__ info, uint32_t n, uint32_t nrhs,
                                                               double* __restrict__ diag) {
  extern __shared__ __attribute__((aligned(16))) cplx tz_lds[];
  constexpr uint32_t NW = NT / 64;
  const uint32_t nvec = 1 + nrhs;
  cplx* const r = tz_lds;
  cplx* const vec = tz_lds + n;
  cplx* const red = tz_lds + (size_t)(2 + nrhs) * n;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t sys = blockIdx.x;                                  // 64-bit element offsets: batch n nrhs passes 2^31
  const cplx* const c = col + sys * n;
  cplx* const bs = b + sys * nrhs * n;
  const uint32_t nb = nrhs * n;                                   // < 2^14: the vectors fit in LDS
  const cplx zero = make_double2(0.0, 0.0);

  const double c0 = dm_ldg(c, 0).x;
  int fail = (c0 > 0.0 && isfinite(c0)) ? 0 : (int)n;             // n: no step has that number (they are 1 .. n - 1)
  if (!fail) {
    for (uint32_t i = tid; i < n; i += NT) {
      const cplx ci = dm_ldg(c, i);
      r[i] = i == 0 ? make_double2(1.0, 0.0) : make_double2(ci.x / c0, ci.y / c0);
      vec[i] = i == 0 ? make_double2(1.0, 0.0) : zero;
    }
    for (uint32_t e = tid; e < nb; e += NT) {
      const cplx v = dm_ldg(bs, e);
      vec[n + e] = make_double2(v.x / c0, v.y / c0);
    }
    __syncthreads();
    double beta = 1.0;
    for (uint32_t k = 1; k < n; ++k) {
      // (A) the dot products with r reversed
      for (uint32_t v0 = 0; v0 < nvec; v0 += 4) {
        cplx acc[4] = {zero, zero, zero, zero};
        for (uint32_t i = tid; i < k; i += NT) {
          const cplx rk = r[k - i];
#pragma unroll
          for (uint32_t g = 0; g < 4; ++g)
            if (v0 + g < nvec) acc[g] = cfma(rk, vec[(size_t)(v0 + g) * n + i], acc[g]);
        }
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) {
          acc[g].x = tz_wave_sum(acc[g].x);
          acc[g].y = tz_wave_sum(acc[g].y);
        }
        if (lane == 0) {
#pragma unroll
          for (uint32_t g = 0; g < 4; ++g)
            if (v0 + g < nvec) red[wave * nvec + v0 + g] = acc[g];
        }
      }
      for (uint32_t v = 1 + tid; v < nvec; v += NT) red[NW * nvec + v] = vec[(size_t)v * n + k];
      __syncthreads();
      // (B) the reflection coefficient and the in-place updates
      cplx ef = red[0];
#pragma unroll
      for (uint32_t w = 1; w < NW; ++w) ef = cadd(ef, red[w * nvec]);
      const cplx gamma = make_double2(-ef.x / beta, -ef.y / beta);
      beta *= 1.0 - cabs2(gamma);
      if (!(beta > 0.0) || !isfinite(beta)) {                     // the same value in every thread: all leave together
        fail = (int)k;
        break;
      }
      cplx* const f = vec;
      for (uint32_t i = tid; 2 * i <= k; i += NT) {
        const uint32_t j = k - i;
        const cplx fi = f[i], fj = i == 0 ? zero : f[j];          // f_k := 0 before the step
        f[i] = cfmac(gamma, fj, fi);
        if (j != i) f[j] = cfmac(gamma, fi, fj);
      }
      for (uint32_t v = 1; v < nvec; ++v) {
        cplx ex = red[v];
#pragma unroll
        for (uint32_t w = 1; w < NW; ++w) ex = cadd(ex, red[w * nvec + v]);
        const cplx bk = red[NW * nvec + v];
        const cplx coef = make_double2((bk.x - ex.x) / beta, (bk.y - ex.y) / beta);
        cplx* const x = vec + (size_t)v * n;
        for (uint32_t i = tid; 2 * i <= k; i += NT) {
          const uint32_t j = k - i;
          const cplx fi = f[i], fj = f[j];                        // this thread's own writes of the loop above
          const cplx xi = x[i], xj = i == 0 ? zero : x[j];        // x_k := 0 (the element held b'_k until now)
          x[i] = cfmac(coef, fj, xi);
          if (j != i) x[j] = cfmac(coef, fi, xj);
        }
      }
      __syncthreads();
    }
    if constexpr (DIAG) {
      if (!fail) {                                                // the same value in every thread
        double* const p = reinterpret_cast<double*>(r);           // |f_i|^2, i < n: r is dead
        double* const tot = reinterpret_cast<double*>(red);       // the waves' totals: red is dead too
        double* const ds = diag + sys * n;
        for (uint32_t i = tid; i < n; i += NT) p[i] = cabs2(vec[i]);
        __syncthreads();
        const uint32_t per = (n + NT - 1) / NT;
        const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
        double own = 0.0;
        for (uint32_t i = lo; i < hi; ++i) own += p[i] - (i == 0 ? 0.0 : p[n - i]);
        const double incl = tz_wave_scan(own, lane);
        const double before = __shfl_up(incl, 1, 64);
        if (NW > 1) {
          if (lane == 63) tot[wave] = incl;
          __syncthreads();
        }
        double run = 0.0;
        for (uint32_t w = 0; w < wave; ++w) run += tot[w];
        if (lane > 0) run += before;
        const double scale = beta * c0;
        for (uint32_t i = lo; i < hi; ++i) {
          run += p[i] - (i == 0 ? 0.0 : p[n - i]);
          dm_stg(ds, i, run / scale);
        }
      }
    }
  }
  if constexpr (DIAG) {
    if (fail)
      for (uint32_t i = tid; i < n; i += NT) dm_stg(diag + sys * n, i, 0.0);
  }
  if (fail) {
    for (uint32_t e = tid; e < nb; e += NT) dm_stg(bs, e, zero);
  } else {
    for (uint32_t e = tid; e < nb; e += NT) dm_stg(bs, e, vec[n + e]);
  }
  if (tid == 0) info[sys] = fail;
}

template <int NT, bool DIAG>
int toeplitz_launch(dm_ctx* ctx, int n, int nrhs, int batch, const cplx* col, cplx* b, int* info, double* diag) {
  const size_t lds = (size_t)dm_toeplitz_lds(n, nrhs);
  if (lds > (size_t)DM_TOEPLITZ_LDS_PLAIN)
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&toeplitz_levinson_kernel<NT, DIAG>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  DM_PLAUNCH(ctx, DM_PROF_UTIL, (toeplitz_levinson_kernel<NT, DIAG>), dim3((unsigned)batch), dim3(NT), lds, ctx->stream,
             col, b, info, (uint32_t)n, (uint32_t)nrhs, diag);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // namespace

extern "C" int dm_toeplitz_max_rhs(int n) { return dm_toeplitz_max_rhs_of(n); }

extern "C" int dm_toeplitz_solve(dm_ctx* ctx, int n, int nrhs, int batch, const void* col_dev, void* b_dev,
                                 int* info_dev) {
  if (!ctx) return DM_EARG;
  const std::string bad = dm_toeplitz_check(n, nrhs, batch, col_dev, b_dev, info_dev);
  if (!bad.empty()) {
    ctx->err = "dm_toeplitz_solve: " + bad;
    return DM_EARG;
  }
  if (batch == 0) return DM_OK;
  DM_HIP(ctx, hipSetDevice(ctx->device));
  const cplx* col = static_cast<const cplx*>(col_dev);
  cplx* b = static_cast<cplx*>(b_dev);
  if (n <= DM_TOEPLITZ_WAVE_N) return toeplitz_launch<64, false>(ctx, n, nrhs, batch, col, b, info_dev, nullptr);
  return toeplitz_launch<256, false>(ctx, n, nrhs, batch, col, b, info_dev, nullptr);
}

extern "C" int dm_toeplitz_solve_diag(dm_ctx* ctx, int n, int nrhs, int batch, const void* col_dev, void* b_dev,
                                      double* diag_dev, int* info_dev) {
  if (!ctx) return DM_EARG;
  const std::string bad = dm_toeplitz_check_diag(n, nrhs, batch, col_dev, b_dev, diag_dev, info_dev);
  if (!bad.empty()) {
    ctx->err = "dm_toeplitz_solve_diag: " + bad;
    return DM_EARG;
  }
  if (batch == 0) return DM_OK;
  DM_HIP(ctx, hipSetDevice(ctx->device));
  const cplx* col = static_cast<const cplx*>(col_dev);
  cplx* b = nrhs > 0 ? static_cast<cplx*>(b_dev) : nullptr;     // without right-hand sides b is never touched
  if (n <= DM_TOEPLITZ_WAVE_N) return toeplitz_launch<64, true>(ctx, n, nrhs, batch, col, b, info_dev, diag_dev);
  return toeplitz_launch<256, true>(ctx, n, nrhs, batch, col, b, info_dev, diag_dev);
}
