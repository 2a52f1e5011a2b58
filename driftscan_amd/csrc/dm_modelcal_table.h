// dm_modelcal_table.h — host side of dm_modelcal_solve: the solution intervals and the
// argument checks.  Plain C++ with no HIP in it, so
// a stand-alone program can compile and call it; dm_modelcal.hip includes the same text.  The incidence table is
// dm_redcal_build(..., min_live = 1) of dm_redcal_table.h: without the "fewer than two" rule.
#pragma once

#include "dm_redcal_table.h"

constexpr int64_t DM_MODELCAL_LDS = DM_GAIN_LDS_SHARED;   // g of all feeds of one interval: two workgroups share a CU

// nint = ceil(ntime / interval); interval q holds the samples q L <= t < min((q + 1) L, ntime).
inline int64_t dm_modelcal_nint(int64_t ntime, int64_t interval) {
  return ntime > 0 && interval > 0 ? (ntime + interval - 1) / interval : 0;
}

// The scalar arguments of dm_modelcal_solve beyond the table: an empty string when they are sound, else what is wrong.
inline std::string dm_modelcal_args_check(int nfeed, int interval, double damping, double tol, int maxiter) {
  if (interval < 1) return "interval must be at least 1";
  if ((int64_t)nfeed * 16 + 64 > DM_MODELCAL_LDS)                // (64 bytes: the eight partial sums of chi^2)
    return "g of one interval for " + std::to_string(nfeed) + " feeds (" + std::to_string((int64_t)nfeed * 16) +
           " bytes) does not fit in the " + std::to_string(DM_MODELCAL_LDS) + " bytes of LDS a workgroup may take";
  return dm_redcal_args_check(damping, tol, maxiter);
}
