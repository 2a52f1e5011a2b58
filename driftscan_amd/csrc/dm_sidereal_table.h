// dm_sidereal_table.h — the tap geometry of dm_sidereal_regrid, plain C++ so that it can be
// compiled and checked without a device.  The geometry of a day depends on (nt_in, ntime, a, phi0, dphi) alone, never on
// the row or the frequency: it is computed once per call in long double and rounded to double.
//
// For grid sample k (phi_k = 2 pi k / ntime): s = max(1, (2 pi / ntime) / dphi), u = (phi_k + 2 pi n - phi0) / dphi in
// [0, 2 pi / dphi), taps j in [ceil(u - a s), floor(u + a s)] with c_j = L_a((u - j) / s), L_a(t) = sinc(t) sinc(t / a)
// inside |t| < a.  A j whose c_j is exactly 0 is not a tap.  Positions are known to DM_SIDEREAL_SNAP of a sample (what
// `sidereal_stack` asks of a day's phi): a u that close to an integer is that integer, a cadence ratio that close to 1
// is 1, so that on-grid data at equal cadence has exactly one tap of coefficient 1 however 2 pi / ntime was rounded.
// sin(pi t) is taken of t - round(t), which makes the zeros of sinc exact.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#define DM_SIDEREAL_MAX_TAPS 1024   // 2 a s + 1 at the most: s up to 170 with a = 3, up to 63 with a = 8
#define DM_SIDEREAL_SPAN 1344       // input samples of one row that a tile stages (32 KB of LDS with weights)
#define DM_SIDEREAL_KT 64           // grid samples of a tile: one per lane of a wave
#define DM_SIDEREAL_ROWS 16         // rows of a tile at the most: 4 waves x 4 rows per thread
#define DM_SIDEREAL_LDS (32 * 1024)
#define DM_SIDEREAL_SNAP 1e-9L

struct dm_sidereal_geom {
  int ntaps_max = 0;                 // T: the widest tap span of a sample, zero coefficients inside it included
  std::vector<int> first;            // [ntime] j of the first tap (may be negative)
  std::vector<int> span;             // [ntime] last tap - first tap + 1 (0: none)
  std::vector<int> ntaps;            // [ntime] taps, i.e. coefficients that are not exactly 0
  std::vector<double> coef;          // [T][ntime]: coef[t * ntime + k] = c_{first[k] + t}, 0 beyond span[k]
  std::vector<double> a_all, s_all;  // [ntime] sum |c_j| and sum c_j over all taps
  std::vector<int> tiles;            // [ntiles][4]: k0, nk, jlo, njs (the staged input samples jlo .. jlo + njs - 1)
  int span_max = 0;                  // the largest njs
};

inline long double dm_sidereal_pi() { return 3.14159265358979323846264338327950288L; }

inline long double dm_sidereal_sinc(long double t) {
  if (t == 0.0L) return 1.0L;
  const long double r = roundl(t), pi = dm_sidereal_pi();
  const long double sn = sinl(pi * (t - r));
  return (fmodl(fabsl(r), 2.0L) == 1.0L ? -sn : sn) / (pi * t);
}

inline long double dm_sidereal_lanczos(long double t, int a) {
  if (!(fabsl(t) < (long double)a)) return 0.0L;
  return dm_sidereal_sinc(t) * dm_sidereal_sinc(t / (long double)a);
}

// Empty string: fine.  Everything dm_sidereal_regrid refuses about the geometry.
inline std::string dm_sidereal_check(int nt_in, int ntime, int a, double phi0, double dphi, double min_share) {
  if (nt_in < 0) return "negative size";
  if (ntime < 1) return "ntime < 1";
  if (a < 1 || a > 8) return "a outside 1..8";
  if (!std::isfinite(phi0) || !std::isfinite(dphi) || !(dphi > 0.0)) return "phi0 or dphi not finite, or dphi <= 0";
  if (!((long double)(nt_in > 0 ? nt_in - 1 : 0) * (long double)dphi < 2.0L * dm_sidereal_pi()))
    return "(nt_in - 1) dphi >= 2 pi: a day is less than one turn";
  if (!(min_share > 0.0 && min_share <= 1.0)) return "min_share outside (0, 1]";
  const long double step = (2.0L * dm_sidereal_pi() / ntime) / (long double)dphi;
  const long double s = step > 1.0L ? step : 1.0L;
  if (2.0L * a * s + 1.0L > (long double)DM_SIDEREAL_MAX_TAPS)
    return "more than " + std::to_string(DM_SIDEREAL_MAX_TAPS) + " taps per sample (2 a s + 1)";
  return std::string();
}

inline void dm_sidereal_geometry(int nt_in, int ntime, int a, double phi0, double dphi, dm_sidereal_geom* g) {
  const long double twopi = 2.0L * dm_sidereal_pi(), dp = (long double)dphi;
  const long double P = twopi / dp, step = (twopi / ntime) / dp;
  long double s = step > 1.0L ? step : 1.0L;
  if (fabsl(step - 1.0L) <= DM_SIDEREAL_SNAP) s = 1.0L;
  long double p0 = fmodl((long double)phi0, twopi);
  if (p0 < 0.0L) p0 += twopi;
  g->first.assign(ntime, 0);
  g->span.assign(ntime, 0);
  g->ntaps.assign(ntime, 0);
  g->a_all.assign(ntime, 0.0);
  g->s_all.assign(ntime, 0.0);
  std::vector<std::vector<long double>> cs(ntime);
  std::vector<int> turn(ntime, 0);
  int T = 0;
  for (int k = 0; k < ntime; ++k) {
    long double u = (twopi * k / ntime - p0) / dp;
    if (u < 0.0L) { u += P; turn[k] = 1; }
    const long double r = roundl(u);
    if (fabsl(u - r) <= DM_SIDEREAL_SNAP) {
      u = r;
      if (u >= P - DM_SIDEREAL_SNAP) { u = 0.0L; turn[k] = 2; }   // one turn on: the day's first sample
    }
    const long jlo = (long)ceill(u - a * s), jhi = (long)floorl(u + a * s);
    std::vector<long double> c;
    for (long j = jlo; j <= jhi; ++j) c.push_back(dm_sidereal_lanczos((u - (long double)j) / s, a));
    size_t b = 0, e = c.size();
    while (b < e && c[b] == 0.0L) ++b;
    while (e > b && c[e - 1] == 0.0L) --e;
    long double A = 0.0L, S = 0.0L;
    int nz = 0;
    for (size_t i = b; i < e; ++i) {
      A += fabsl(c[i]);
      S += c[i];
      nz += c[i] != 0.0L;
    }
    g->first[k] = (int)(jlo + (long)b);
    g->span[k] = (int)(e - b);
    g->ntaps[k] = nz;
    g->a_all[k] = (double)A;
    g->s_all[k] = (double)S;
    cs[k].assign(c.begin() + b, c.begin() + e);
    if ((int)(e - b) > T) T = (int)(e - b);
  }
  g->ntaps_max = T;
  g->coef.assign((size_t)(T > 0 ? T : 1) * ntime, 0.0);
  for (int k = 0; k < ntime; ++k)
    for (size_t t = 0; t < cs[k].size(); ++t) g->coef[t * ntime + k] = (double)cs[k][t];
  // tiles: runs of up to KT grid samples of one turn (u increases inside a tile) whose taps, clipped to the day, span
  // DM_SIDEREAL_SPAN input samples at the most
  g->tiles.clear();
  g->span_max = 1;
  for (int k0 = 0; k0 < ntime;) {
    int nk = 0;
    long lo = 0, hi = -1;
    while (k0 + nk < ntime && nk < DM_SIDEREAL_KT && turn[k0 + nk] == turn[k0]) {
      const int k = k0 + nk;
      long l = nk == 0 ? g->first[k] : lo, h = hi;
      if (g->first[k] < l) l = g->first[k];
      if ((long)g->first[k] + g->span[k] - 1 > h) h = (long)g->first[k] + g->span[k] - 1;
      long lc = l < 0 ? 0 : l, hc = h > nt_in - 1 ? nt_in - 1 : h;
      if (nk > 0 && hc - lc + 1 > DM_SIDEREAL_SPAN) break;
      lo = l;
      hi = h;
      ++nk;
    }
    const long lc = lo < 0 ? 0 : lo, hc = hi > nt_in - 1 ? nt_in - 1 : hi;
    const int njs = hc >= lc ? (int)(hc - lc + 1) : 0;
    g->tiles.push_back(k0);
    g->tiles.push_back(nk);
    g->tiles.push_back((int)lc);
    g->tiles.push_back(njs);
    if (njs > g->span_max) g->span_max = njs;
    k0 += nk;
  }
}
