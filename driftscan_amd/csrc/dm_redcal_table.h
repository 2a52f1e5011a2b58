// dm_redcal_table.h — host side of dm_redcal_solve: the solver's member factors with the "fewer
// than two" rule, the feed-major incidence table of the gain step, the split of the feeds over workgroups and the
// argument checks.  Plain C++ with no HIP in it, so a stand-alone program can compile and call it
// (scratch/redcal_table_check.cpp does, under the address and undefined-behaviour sanitizers); dm_redcal.hip includes
// the same text.
#pragma once

#include "dm_stack_table.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// One incidence of a feed a: member `row` = (a, partner) when side == 0, (partner, a) when side == 1, of class `cls`.
struct dm_redcal_inc {
  int row, partner, cls, side;
};
// the table is uploaded as it is and the kernels read an incidence as one int4: x = row, y = partner, z = cls, w = side
static_assert(sizeof(dm_redcal_inc) == 16 && offsetof(dm_redcal_inc, row) == 0 && offsetof(dm_redcal_inc, partner) == 4 &&
                  offsetof(dm_redcal_inc, cls) == 8 && offsetof(dm_redcal_inc, side) == 12,
              "dm_redcal_inc is the int4 (row, partner, cls, side) of the kernels");

struct dm_redcal_table {
  std::vector<double> yfac;          // (nmem) fw_i fw_j, 0 for an autocorrelation: the factor of the y step
  std::vector<double> gfac;          // (nmem) yfac, 0 on the members of an unconstrained class: gain step and chi^2
  std::vector<int> inc_off;          // (nfeed + 1)
  std::vector<dm_redcal_inc> inc;    // per feed, in member order, its members with gfac > 0
  int nconstrained = 0;              // classes with at least min_live (two) members of yfac > 0
};

// The factors and the incidence table for a checked class table (dm_stack_table_check) and feed weights >= 0 or null
// (ones).  A class constrains the gains when at least two of its members join different feeds of positive weight;
// every member of any other class gets gfac = 0 and is not listed.  A function of the table and the feed weights alone.
// min_live = 1 drops that rule (dm_modelcal_solve, section 4.21: against a given model a class of one member constrains
// its two feeds), so that gfac == yfac and every member of yfac > 0 is listed.
inline dm_redcal_table dm_redcal_build(int nfeed, int npairs, const int* class_off, const int* members,
                                       const double* feed_weight, int min_live = 2) {
  dm_redcal_table t;
  const int64_t nmem = npairs > 0 ? class_off[npairs] : 0;
  t.yfac.assign((size_t)nmem, 0.0);
  t.gfac.assign((size_t)nmem, 0.0);
  t.inc_off.assign((size_t)nfeed + 1, 0);
  for (int c = 0; c < npairs; ++c) {
    int live = 0;
    for (int k = class_off[c]; k < class_off[c + 1]; ++k) {
      const int i = members[2 * (int64_t)k], j = members[2 * (int64_t)k + 1];
      const double fac = feed_weight ? feed_weight[i] * feed_weight[j] : 1.0;
      if (i != j && fac > 0.0) {
        t.yfac[k] = fac;
        ++live;
      }
    }
    if (live < min_live) continue;
    ++t.nconstrained;
    for (int k = class_off[c]; k < class_off[c + 1]; ++k)
      if (t.yfac[k] > 0.0) {
        t.gfac[k] = t.yfac[k];
        ++t.inc_off[(size_t)members[2 * (int64_t)k] + 1];
        ++t.inc_off[(size_t)members[2 * (int64_t)k + 1] + 1];
      }
  }
  for (int a = 0; a < nfeed; ++a) t.inc_off[a + 1] += t.inc_off[a];
  t.inc.resize((size_t)t.inc_off[nfeed]);
  std::vector<int> at(t.inc_off.begin(), t.inc_off.end() - 1);
  for (int c = 0; c < npairs; ++c)
    for (int k = class_off[c]; k < class_off[c + 1]; ++k)
      if (t.gfac[k] > 0.0) {
        const int i = members[2 * (int64_t)k], j = members[2 * (int64_t)k + 1];
        t.inc[(size_t)at[i]++] = dm_redcal_inc{k, j, c, 0};
        t.inc[(size_t)at[j]++] = dm_redcal_inc{k, i, c, 1};
      }
  return t;
}

// The scalar arguments of dm_redcal_solve: an empty string when they are sound, else what is wrong.
inline std::string dm_redcal_args_check(double damping, double tol, int maxiter) {
  if (!(damping > 0.0 && damping <= 1.0)) return "damping must lie in (0, 1]";
  if (!(tol >= 0.0) || !std::isfinite(tol)) return "tol must be finite and not negative";
  if (maxiter < 1) return "maxiter must be at least 1";
  return "";
}

// Feed ranges of the workgroups of one (realisation, frequency, time tile) of the gain step: chunk q takes the feeds
// [chunk[q], chunk[q + 1]).  A feed is never cut (its sums stay inside one wave, so the split changes no bit); the cuts
// fall where the incidence count passes multiples of ninc / nchunks.  As dm_stack_chunks: about 2048 workgroups, at
// least 1024 incidences per chunk so that restaging the gains stays a small part of its traffic.
inline std::vector<int> dm_redcal_chunks(int nfeed, const int* inc_off, int64_t cells) {
  const int64_t ninc = nfeed > 0 ? inc_off[nfeed] : 0;
  int64_t want = cells > 0 ? (2048 + cells - 1) / cells : 1;
  if (want > ninc / 1024) want = ninc / 1024;
  if (want > nfeed) want = nfeed;
  if (want < 1) want = 1;
  std::vector<int> chunk(1, 0);
  for (int64_t q = 1; q < want; ++q) {
    const int64_t target = ninc * q / want;
    int a = chunk.back();
    while (a < nfeed && inc_off[a] < target) ++a;
    if (a > chunk.back() && a < nfeed) chunk.push_back(a);
  }
  chunk.push_back(nfeed);
  return chunk;
}
