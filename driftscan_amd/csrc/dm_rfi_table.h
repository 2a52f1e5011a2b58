// dm_rfi_table.h — the argument check and the two tables of dm_rfi_flag, plain C++ so that
// they can be compiled and checked without a device.  Both tables depend on the parameters alone, never on the data: they
// are made once per call in long double and rounded to double once, and they are part of the method.
//
//   g_d = exp(-d^2 / (2 sigma_k^2)), d = 0 .. H, H = ceil(3 sigma_k): the background kernel
//   t[it][M] = alpha + chi_M s_it beta, chi_M = chi1 rho^(-log2 M), s_it = base^(niter - 1 - it): the threshold of the
//   window length M in iteration it, in units of the median amplitude; alpha = sqrt(pi / (4 ln 2)) and
//   beta = sqrt((1 - pi / 4) / ln 2) are the mean and the standard deviation of a Rayleigh amplitude in those units.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#define DM_RFI_MAX_SEGMENT 2048   // samples of one segment: 27 bytes of LDS per sample, 55 KB at the most
#define DM_RFI_MAX_H 32           // half width of the background kernel
#define DM_RFI_MAX_WINDOWS 7      // 1, 2, 4, ..., 64
#define DM_RFI_MAX_WINDOW 64
#define DM_RFI_MAX_ITER 8
#define DM_RFI_SQRT_LN2 0.83255461115769775635   // sigma = median / sqrt(ln 2) for a Rayleigh amplitude

// What the kernel is handed by value: both tables and the window lengths.
struct dm_rfi_tables {
  double g[DM_RFI_MAX_H + 1];                            // g[d], d = 0 .. H
  double t[DM_RFI_MAX_ITER][DM_RFI_MAX_WINDOWS];         // t[it][i] of window[i]
  int window[DM_RFI_MAX_WINDOWS];
  int nwin, H, niter, min_good;
};

inline long double dm_rfi_pi() { return 3.14159265358979323846264338327950288L; }
inline long double dm_rfi_ln2() { return 0.693147180559945309417232121458176568L; }

// Empty string: fine.  Everything dm_rfi_flag refuses about the parameters.
inline std::string dm_rfi_check(int nt, int segment, double kernel_sigma, int nwin, const int* windows, double chi1,
                                double rho, int niter, double base, int min_good, double row_share) {
  if (nt < 0) return "negative size";
  if (segment < 1 || segment > DM_RFI_MAX_SEGMENT)
    return "segment outside 1.." + std::to_string(DM_RFI_MAX_SEGMENT);
  if (!std::isfinite(kernel_sigma) || !(kernel_sigma > 0.0)) return "kernel_sigma not finite or <= 0";
  if (ceill(3.0L * (long double)kernel_sigma) > (long double)DM_RFI_MAX_H)
    return "H = ceil(3 kernel_sigma) > " + std::to_string(DM_RFI_MAX_H);
  if (nwin < 1 || nwin > DM_RFI_MAX_WINDOWS || !windows) return "windows: 1.." + std::to_string(DM_RFI_MAX_WINDOWS) + " lengths expected";
  for (int i = 0; i < nwin; ++i) {
    const int M = windows[i];
    if (M < 1 || M > DM_RFI_MAX_WINDOW || (M & (M - 1)) != 0 || (i > 0 && M <= windows[i - 1]))
      return "windows are not ascending powers of two <= " + std::to_string(DM_RFI_MAX_WINDOW);
  }
  if (!std::isfinite(chi1) || !(chi1 > 0.0)) return "chi1 not finite or <= 0";
  if (!std::isfinite(rho) || !(rho >= 1.0)) return "rho not finite or < 1";
  if (niter < 1 || niter > DM_RFI_MAX_ITER) return "niter outside 1.." + std::to_string(DM_RFI_MAX_ITER);
  if (!std::isfinite(base) || !(base >= 1.0)) return "base not finite or < 1";
  if (min_good < 1) return "min_good < 1";
  if (!(row_share > 0.0 && row_share <= 1.0)) return "row_share outside (0, 1]";
  return std::string();
}

inline int dm_rfi_halfwidth(double kernel_sigma) { return (int)ceill(3.0L * (long double)kernel_sigma); }

inline void dm_rfi_make_tables(double kernel_sigma, int nwin, const int* windows, double chi1, double rho, int niter,
                               double base, int min_good, dm_rfi_tables* tb) {
  const long double s = (long double)kernel_sigma, ln2 = dm_rfi_ln2(), pi = dm_rfi_pi();
  const long double alpha = sqrtl(pi / (4.0L * ln2)), beta = sqrtl((1.0L - pi / 4.0L) / ln2);
  tb->H = dm_rfi_halfwidth(kernel_sigma);
  tb->nwin = nwin;
  tb->niter = niter;
  tb->min_good = min_good;
  for (int d = 0; d <= DM_RFI_MAX_H; ++d)
    tb->g[d] = d <= tb->H ? (double)expl(-((long double)d * d) / (2.0L * s * s)) : 0.0;
  for (int i = 0; i < DM_RFI_MAX_WINDOWS; ++i) tb->window[i] = i < nwin ? windows[i] : 0;
  for (int it = 0; it < DM_RFI_MAX_ITER; ++it)
    for (int i = 0; i < DM_RFI_MAX_WINDOWS; ++i) {
      tb->t[it][i] = 0.0;
      if (it >= niter || i >= nwin) continue;
      int lg = 0;
      while ((1 << lg) < windows[i]) ++lg;
      const long double chi = (long double)chi1 * powl((long double)rho, -(long double)lg);
      const long double sit = powl((long double)base, (long double)(niter - 1 - it));
      tb->t[it][i] = (double)(alpha + chi * sit * beta);
    }
}
