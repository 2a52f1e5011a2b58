// dm_feedpair.h — host code that the entries of the feed-pair chain share (dm_stack.hip, dm_redcal.hip, dm_modelcal.hip;
// DESIGN.md sections 4.17, 4.18 and 4.21): the refusal, the LDS attribute of a kernel that stages gains, and the
// iteration driver of the two solvers.  The checks with no HIP in them are in dm_stack_table.h.
#pragma once

#include "dm_common.h"
#include "dm_gain_table.h"

#include <string>

inline int dm_refuse(dm_ctx* ctx, const char* who, const std::string& what) {
  ctx->err = std::string(who) + ": " + what;
  return DM_EARG;
}

// A kernel whose dynamic LDS is past what two workgroups of a CU can share has to be allowed it.
template <typename K>
int dm_lds_attr(dm_ctx* ctx, K kernel, size_t lds) {
  if (lds > (size_t)DM_GAIN_LDS_SHARED)
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
  return DM_OK;
}

constexpr int DM_POLL_CHECK = 16;   // every so many iterations the host asks (without waiting) whether any problem is left

// Counter slots a solver of `maxiter` iterations sets aside for dm_poll_iterate (zeroed, on the device).
inline int dm_poll_slots(int maxiter) { return maxiter / DM_POLL_CHECK + 1; }

struct dm_poll_result {
  int rc = DM_OK;
  int k_last = 0;          // the last iteration launched
  bool all_done = false;   // a check landed with no problem left: the loop stopped early
};

// The iterations k = 1 .. maxiter of a solver whose kernels keep their own per-problem state: launch(k, count) queues
// iteration k on ctx->stream; where `count` is not null, the iteration adds to *count (a slot of `pending`) the problems
// that are not done after it.  Every DM_POLL_CHECK iterations, and with no check in flight, a slot is handed over and its
// download queued behind the launch; later iterations ask whether it has landed and never wait for it, so the stream
// stays full.  The loop ends at maxiter or once a landed counter is 0.  On an error the download in flight is abandoned.
template <typename Launch>
dm_poll_result dm_poll_iterate(dm_ctx* ctx, int maxiter, int* pending, Launch launch) {
  dm_poll_result r;
  const int* landed = nullptr;   // the host copy of the counter of the check in flight
  auto iterate = [&]() -> int {
    for (int k = 1; k <= maxiter && !r.all_done; ++k) {
      int* count = nullptr;
      if (k % DM_POLL_CHECK == 0 && !landed) count = pending + k / DM_POLL_CHECK;
      DM_TRY(launch(k, count));
      r.k_last = k;
      if (count) {
        const void* host = nullptr;
        DM_TRY(dm_download_queue(ctx, count, sizeof(int), &host));
        landed = static_cast<const int*>(host);
      } else if (landed && ctx->dl_ev && hipEventQuery(ctx->dl_ev) == hipSuccess) {   // asked, never waited for
        r.all_done = *landed == 0;
        DM_TRY(dm_download_wait(ctx));
        landed = nullptr;
      }
    }
    return DM_OK;
  };
  r.rc = iterate();
  if (r.rc != DM_OK)
    dm_download_abandon(ctx);
  else if (landed)
    r.rc = dm_download_wait(ctx);
  return r;
}
