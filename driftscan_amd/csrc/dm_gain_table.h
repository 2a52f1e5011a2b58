// dm_gain_table.h — host-side checks of dm_ts_gain_apply: the pair table and the choice of the
// time tile.  Plain C++ with no HIP in it, so a stand-alone program can compile and call it (scratch/gain_table_check.cpp
// does, under the address and undefined-behaviour sanitizers); dm_tsim.hip includes the same text.
#pragma once

#include <cstdint>
#include <string>

constexpr int64_t DM_GAIN_LDS_BYTES = 160 * 1024;   // LDS of one CU on gfx950: the most one workgroup can hold
constexpr int64_t DM_GAIN_LDS_SHARED = 64 * 1024;   // a tile of at most this leaves room for a second workgroup
constexpr int DM_GAIN_TILE_MAX = 16;                // time samples per tile: 16 x 16 B = one 256-byte row of LDS banks

// Time samples per workgroup tile for `nfeed` feeds: the largest power of two <= 16 whose g tile (nfeed x tile x 16 B)
// fits in 64 KiB; a single sample may take up to the whole 160 KiB.  0: not even one sample fits.  A function of nfeed
// alone, so the summation order of a class (which depends on the tile) never depends on the batch.
inline int dm_gain_tile(int64_t nfeed) {
  if (nfeed <= 0) return DM_GAIN_TILE_MAX;
  for (int tile = DM_GAIN_TILE_MAX; tile >= 1; tile >>= 1)
    if (nfeed * tile * 16 <= DM_GAIN_LDS_SHARED) return tile;
  return nfeed * 16 <= DM_GAIN_LDS_BYTES ? 1 : 0;
}

// The pair table of dm_ts_gain_apply: class_off (npairs + 1) ascending from 0, members (class_off[npairs], 2) feed
// indices.  Returns an empty string when the table is sound, else what is wrong with it: an empty class, a feed index
// outside [0, nfeed), offsets that do not start at 0, or an nfeed whose single-sample tile does not fit in LDS.
inline std::string dm_gain_table_check(int nfeed, int npairs, const int* class_off, const int* members) {
  if (nfeed < 0 || npairs < 0) return "negative size";
  if (dm_gain_tile(nfeed) == 0)
    return "the g tile of one time sample for " + std::to_string(nfeed) + " feeds (" + std::to_string((int64_t)nfeed * 16) +
           " bytes) does not fit in the " + std::to_string(DM_GAIN_LDS_BYTES) + " bytes of LDS";
  if (npairs == 0) return "";
  if (!class_off || !members) return "null pair table";
  if (class_off[0] != 0) return "class_off[0] must be 0";
  for (int c = 0; c < npairs; ++c)
    if (class_off[c + 1] <= class_off[c]) return "class " + std::to_string(c) + " is empty";
  const int64_t n = class_off[npairs];
  for (int64_t k = 0; k < 2 * n; ++k)
    if (members[k] < 0 || members[k] >= nfeed)
      return "member " + std::to_string(k / 2) + " names feed " + std::to_string(members[k]) + " of " + std::to_string(nfeed);
  return "";
}
