// dm_philox.h — the counter-based sample stream shared by the Monte-Carlo estimators (dm_psmc.hip) and the sky draws
// (dm_skysim.hip): Philox4x32-10, the 53-bit uniforms and the Box-Muller map.  Both files compile this text, so a
// (key, counter) gives the same bits in either.
#pragma once

#include "dm_common.h"

#if defined(__HIPCC__)

// ---- Philox4x32-10 (Salmon et al., SC'11) ----------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
  }
}

// 53-bit uniform in (0, 1] from two words: ((a >> 5) 2^26 + (b >> 6) + 1) 2^-53, exact in double
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  const uint64_t k = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
  return (double)(k + 1) * 0x1p-53;
}

// complex standard normal, E|z|^2 = 1, times sc, from one generated block: |z| = sqrt(-log u1), arg z = 2 pi u2
__device__ __forceinline__ cplx philox_normal(const uint32_t c[4], double sc) {
  const double u1 = u53(c[0], c[1]), u2 = u53(c[2], c[3]);
  const double rad = sqrt(-log(u1)) * sc;
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  cplx z;
  z.x = rad * cs;
  z.y = rad * sn;
  return z;
}

#endif  // __HIPCC__
