// dm_stack_sum.h — the device code that dm_stack.hip and dm_redcal.hip (section 4.18) share:
// the gains of a time tile staged in LDS and the weighted, calibrated sums of one class.  One text, so the y step of the
// redundant-calibration solver has the arithmetic and the summation order of vis_stack_kernel by construction.
#pragma once

#include "dm_common.h"

#if defined(__HIPCC__)

// Waves per workgroup of the kernels that stage gains: 8, so that the two workgroups whose 64 KiB tiles fit in a CU's LDS
// keep four waves on every SIMD (with 4 the stack ran at 1.4 waves per SIMD at 512 feeds, waiting 83 % of their cycles:
// DESIGN.md section 4.17); 4 without gains.
constexpr int stack_waves(bool has_g) { return has_g ? 8 : 4; }

// The gains of one time tile into LDS: [feed][TT], zeros past ntime.
template <int TT, int NW>
__device__ __forceinline__ void stack_stage_gains(cplx* gtile, const cplx* __restrict__ g, size_t grow, uint32_t nfeed,
                                                  uint32_t ntime, uint32_t tt, uint32_t t, bool live) {
  constexpr uint32_t S = NW * 64 / TT;
  for (uint32_t a = threadIdx.x / TT; a < nfeed; a += S)
    gtile[a * TT + tt] = live ? dm_ldg(g, (grow + a) * ntime + t) : make_double2(0.0, 0.0);
  __syncthreads();
}

// N = sum w conj(g_i) g_j V and D = sum w |g_i|^2 |g_j|^2 over the members [m0, m1) of a class, for the sample of this
// lane: slot s adds its members s, s + W, ... in the table's order and the slots are added by an xor butterfly (s ^ 1,
// s ^ 2, ...), so the order of both sums is a function of (n_c, W) alone.  On return every slot holds the sums.  HAS_G
// false: no LDS and no table load (conj(g_i) g_j = 1); HAS_W false: no weight load; mfac (one f64 per member) is
// optional at run time.  A lane that is not `live` adds nothing and still takes part in the butterfly.
template <int TT, bool HAS_G, bool HAS_W>
__device__ __forceinline__ void stack_class_sums(const cplx* __restrict__ vis, const double* __restrict__ w,
                                                 const double* __restrict__ mfac, const int2* __restrict__ members,
                                                 const cplx* gtile, size_t vrow, size_t wrow, uint32_t ntime, int m0, int m1,
                                                 uint32_t s, uint32_t tt, bool live, double& nx, double& ny, double& d) {
  constexpr uint32_t W = 64 / TT;
  nx = 0.0, ny = 0.0, d = 0.0;
  if (live) {
#pragma unroll 4
    for (int k = m0 + (int)s; k < m1; k += (int)W) {
      const cplx v = dm_ldg(vis, vrow + (size_t)k * ntime);
      double we = 1.0;
      if constexpr (HAS_W) we = dm_ldg(w, wrow + (size_t)k * ntime);
      if (mfac) we *= dm_ldg(mfac, (size_t)k);
      if constexpr (HAS_G) {
        const int2 m = members[k];
        const cplx gi = gtile[(uint32_t)m.x * TT + tt], gj = gtile[(uint32_t)m.y * TT + tt];
        const cplx p = cmul(cmulc(gj, gi), v);                 // conj(g_i) g_j V
        nx = fma(we, p.x, nx);
        ny = fma(we, p.y, ny);
        d = fma(we, cabs2(gi) * cabs2(gj), d);
      } else {
        nx = fma(we, v.x, nx);
        ny = fma(we, v.y, ny);
        d += we;
      }
    }
  }
#pragma unroll
  for (int o = TT; o < 64; o <<= 1) {
    nx += __shfl_xor(nx, o, 64);
    ny += __shfl_xor(ny, o, 64);
    d += __shfl_xor(d, o, 64);
  }
}

#endif  // __HIPCC__
