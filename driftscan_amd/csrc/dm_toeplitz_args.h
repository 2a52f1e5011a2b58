// dm_toeplitz_args.h — host-side sizing and argument checks of dm_toeplitz_solve[_diag].  Plain C++
// with no HIP in it, so a stand-alone program can compile and call it (scratch/toeplitz_args_check.cpp does, under the
// address and undefined-behaviour sanitizers); dm_toeplitz.hip includes the same text.
#pragma once

#include <cstdint>
#include <string>

constexpr int64_t DM_TOEPLITZ_LDS_BYTES = 160 * 1024;   // LDS of one CU on gfx950: the most one workgroup can hold
constexpr int64_t DM_TOEPLITZ_LDS_PLAIN = 64 * 1024;    // above this the launch raises the kernel's dynamic LDS limit
#ifndef DM_TOEPLITZ_WAVE_MAX
#define DM_TOEPLITZ_WAVE_MAX 384                        // measured, DESIGN.md section 4.16 (a build may move it to measure)
#endif
constexpr int DM_TOEPLITZ_WAVE_N = DM_TOEPLITZ_WAVE_MAX;  // n up to this: one wave per system, beyond: 256 threads
constexpr int DM_TOEPLITZ_RED_ROWS = 5;                 // reduction rows: one per wave of the largest workgroup + b'_k

// LDS of one workgroup: r, f and the nrhs solution vectors (n complex128 each), then the reduction scratch of
// DM_TOEPLITZ_RED_ROWS rows of 1 + nrhs complex128 (the partial dot products of every wave and the element b'_k).
inline int64_t dm_toeplitz_lds(int64_t n, int64_t nrhs) {
  return (2 + nrhs) * n * 16 + DM_TOEPLITZ_RED_ROWS * (1 + nrhs) * 16;
}

// Largest nrhs whose LDS need fits one CU, 0 if not even one right-hand side does (n > 3410).
inline int dm_toeplitz_max_rhs_of(int64_t n) {
  if (n < 1) return 0;
  const int64_t per_rhs = 16 * n + 16 * DM_TOEPLITZ_RED_ROWS;
  const int64_t fixed = 32 * n + 16 * DM_TOEPLITZ_RED_ROWS;
  if (fixed + per_rhs > DM_TOEPLITZ_LDS_BYTES) return 0;
  const int64_t r = (DM_TOEPLITZ_LDS_BYTES - fixed) / per_rhs;
  return (int)(r > 65535 ? 65535 : r);
}

// Empty when a call may be launched (or is the batch = 0 no-op), else what is wrong with it.
inline std::string dm_toeplitz_check(int n, int nrhs, int batch, const void* col, const void* b, const void* info) {
  if (n < 1) return "n = " + std::to_string(n) + " < 1";
  if (nrhs < 1) return "nrhs = " + std::to_string(nrhs) + " < 1";
  const int most = dm_toeplitz_max_rhs_of(n);
  if (nrhs > most)
    return "nrhs = " + std::to_string(nrhs) + " right-hand sides of order " + std::to_string(n) + " need " +
           std::to_string(dm_toeplitz_lds(n, nrhs)) + " bytes of LDS, a CU has " + std::to_string(DM_TOEPLITZ_LDS_BYTES) +
           " (dm_toeplitz_max_rhs: " + std::to_string(most) + ")";
  if (batch < 0) return "batch = " + std::to_string(batch) + " < 0";
  if (batch > 0 && (!col || !b || !info)) return "null pointer with batch > 0";
  return "";
}

// The same for dm_toeplitz_solve_diag: nrhs = 0 is allowed (the diagonal alone: b is then not looked at, null or not)
// and `diag` must be there.  Order n without right-hand sides needs the LDS of r, f and the reduction rows.
inline std::string dm_toeplitz_check_diag(int n, int nrhs, int batch, const void* col, const void* b, const void* diag,
                                          const void* info) {
  if (n < 1) return "n = " + std::to_string(n) + " < 1";
  if (nrhs < 0) return "nrhs = " + std::to_string(nrhs) + " < 0";
  if (nrhs > 0) {
    const std::string bad = dm_toeplitz_check(n, nrhs, batch, col, b, info);
    if (!bad.empty()) return bad;
  } else if (dm_toeplitz_lds(n, 0) > DM_TOEPLITZ_LDS_BYTES) {
    return "order " + std::to_string(n) + " needs " + std::to_string(dm_toeplitz_lds(n, 0)) + " bytes of LDS, a CU has " +
           std::to_string(DM_TOEPLITZ_LDS_BYTES);
  }
  if (batch < 0) return "batch = " + std::to_string(batch) + " < 0";
  if (batch > 0 && (!col || !diag || !info)) return "null pointer with batch > 0";
  return "";
}
