// dm_stack_table.h — host-side checks of the feed-pair entries (dm_vis_stack and dm_vis_expand, DESIGN.md section 4.17;
// dm_redcal_solve, 4.18; dm_modelcal_solve, 4.21): the arguments they share, the class table of unstacked
// (per-feed-pair) visibilities, the split of the classes over workgroups and the overlap of buffers.  Plain
// C++ with no HIP in it, so a stand-alone program can compile and call it (scratch/stack_table_check.cpp does, under the
// address and undefined-behaviour sanitizers); dm_stack.hip includes the same text.
#pragma once

#include "dm_gain_table.h"

#include <cstdint>
#include <string>
#include <vector>

constexpr int DM_STACK_TILE_PLAIN = 16;   // time samples per tile when no gains are staged: 16 x 16 B = 256 bytes per row

// Time samples per workgroup tile: the tile of dm_ts_gain_apply when gains are staged in LDS (a function of nfeed alone),
// 16 without gains.  0: gains are given and not even one sample of them fits in LDS.
inline int dm_stack_tile(int64_t nfeed, bool has_g) { return has_g ? dm_gain_tile(nfeed) : DM_STACK_TILE_PLAIN; }

// The class table of dm_vis_stack / dm_vis_expand: class_off (npairs + 1) from 0, never decreasing and with no empty
// class; members (class_off[npairs], 2) feed indices in [0, nfeed).  Returns an empty string when the table is sound,
// else what is wrong with it.  The LDS condition applies only when gains are given.
inline std::string dm_stack_table_check(int nfeed, int npairs, const int* class_off, const int* members, bool has_g) {
  if (nfeed < 0 || npairs < 0) return "negative size";
  if (has_g && dm_gain_tile(nfeed) == 0)
    return "the g tile of one time sample for " + std::to_string(nfeed) + " feeds (" + std::to_string((int64_t)nfeed * 16) +
           " bytes) does not fit in the " + std::to_string(DM_GAIN_LDS_BYTES) + " bytes of LDS";
  if (npairs == 0) return "";
  if (!class_off || !members) return "null class table";
  if (class_off[0] != 0) return "class_off[0] must be 0";
  for (int c = 0; c < npairs; ++c) {
    if (class_off[c + 1] < class_off[c]) return "class_off decreases at class " + std::to_string(c);
    if (class_off[c + 1] == class_off[c]) return "class " + std::to_string(c) + " is empty";
  }
  const int64_t n = class_off[npairs];
  for (int64_t k = 0; k < 2 * n; ++k)
    if (members[k] < 0 || members[k] >= nfeed)
      return "member " + std::to_string(k / 2) + " names feed " + std::to_string(members[k]) + " of " + std::to_string(nfeed);
  return "";
}

// What every feed-pair entry checks first, in this order: the sizes and the strides between realisations (`rstride_min`,
// the smallest of them) are not negative; the realisations of the weights and of the model (w_nreal, m_nreal: null where
// the entry has none, or checks it itself) are 1 or nreal; the class table; the feed weights (null: ones) are not
// negative (a NaN is refused too).  Returns an empty string, or what is wrong.
inline std::string dm_pair_args_check(int nreal, int nf, int nfeed, int npairs, int ntime, int64_t rstride_min,
                                      const int* w_nreal, const int* m_nreal, const int* class_off, const int* members,
                                      bool has_g, const double* feed_weight) {
  if (nreal < 0 || nf < 0 || nfeed < 0 || npairs < 0 || ntime < 0 || rstride_min < 0) return "negative size";
  if (w_nreal && *w_nreal != 1 && *w_nreal != nreal) return "w_nreal must be 1 or nreal";
  if (m_nreal && *m_nreal != 1 && *m_nreal != nreal) return "m_nreal must be 1 or nreal";
  const std::string bad = dm_stack_table_check(nfeed, npairs, class_off, members, has_g);
  if (!bad.empty()) return bad;
  if (feed_weight)
    for (int a = 0; a < nfeed; ++a)
      if (!(feed_weight[a] >= 0.0)) return "feed weight " + std::to_string(a) + " is negative";
  return "";
}

// Class ranges of the workgroups of one (realisation, frequency, time tile): chunk q takes the classes
// [chunk[q], chunk[q + 1]).  A class is never cut (its sum stays inside one wave, so the split changes no bit); the cuts
// fall where the member count passes multiples of nmem / nchunks.  `cells` is the number of (realisation, frequency,
// tile) cells of the launch: few cells get many chunks so that about 2048 workgroups exist, and a chunk holds at least
// 1024 members so that restaging the gains stays a small part of its traffic.
inline std::vector<int> dm_stack_chunks(int npairs, const int* class_off, int64_t cells) {
  const int64_t nmem = npairs > 0 ? class_off[npairs] : 0;
  int64_t want = cells > 0 ? (2048 + cells - 1) / cells : 1;
  if (want > nmem / 1024) want = nmem / 1024;
  if (want > npairs) want = npairs;
  if (want < 1) want = 1;
  std::vector<int> chunk(1, 0);
  for (int64_t q = 1; q < want; ++q) {
    const int64_t target = nmem * q / want;
    int c = chunk.back();
    while (c < npairs && class_off[c] < target) ++c;
    if (c > chunk.back() && c < npairs) chunk.push_back(c);
  }
  chunk.push_back(npairs);
  return chunk;
}

// Whether two strided buffers can share a byte: each is `nreal` rows of `row` bytes, `stride` bytes apart, from address
// `a` / `b`.  The test is on the whole spans (first byte of the first row to last byte of the last), so it may refuse
// rows that merely interleave; it never accepts buffers that share an element.
inline bool dm_spans_overlap(uint64_t a, uint64_t a_row, uint64_t a_stride, uint64_t b, uint64_t b_row, uint64_t b_stride,
                             int64_t nreal) {
  if (nreal <= 0 || a_row == 0 || b_row == 0) return false;
  const uint64_t a_end = a + (uint64_t)(nreal - 1) * a_stride + a_row;
  const uint64_t b_end = b + (uint64_t)(nreal - 1) * b_stride + b_row;
  return a < b_end && b < a_end;
}

// One contiguous buffer of an entry, by the name its refusal uses; p may be null when bytes is 0.
struct dm_span {
  const void* p;
  uint64_t bytes;
  const char* name;
};

// That no output shares an element with an input or with an output before it: an empty string, or "<output> shares an
// element with <the other>" for the first pair that does (outputs in their order, against the inputs first).  A span of
// no bytes shares nothing.
inline std::string dm_spans_shared(const dm_span* in, int nin, const dm_span* out, int nout) {
  for (int o = 0; o < nout; ++o)
    for (int i = 0; i < nin + o; ++i) {
      const dm_span& other = i < nin ? in[i] : out[i - nin];
      if (dm_spans_overlap((uint64_t)out[o].p, out[o].bytes, 0, (uint64_t)other.p, other.bytes, 0, 1))
        return std::string(out[o].name) + " shares an element with " + other.name;
    }
  return "";
}
