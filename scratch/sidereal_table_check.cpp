// The tap geometry of dm_sidereal_regrid (driftscan_amd/csrc/dm_sidereal_table.h) on the host alone, for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idriftscan_amd/csrc \
//       scratch/sidereal_table_check.cpp -o scratch/bin/sidereal_table_check
//   scratch/bin/sidereal_table_check NT_IN NTIME A PHI0 DPHI        (PHI0, DPHI as C99 hex floats)
// prints per grid sample "first span ntaps A_all S_all c..." (hex floats), then the tiles, span_max and T, or "bad <why>".
// scratch/sidereal_table_check.py builds it, runs it on the geometries of tests/sidereal_cases.py and compares every line
// with timestream.sidereal_taps_host.
#include "dm_sidereal_table.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int nt_in = atoi(argv[1]), ntime = atoi(argv[2]), a = atoi(argv[3]);
  const double phi0 = strtod(argv[4], nullptr), dphi = strtod(argv[5], nullptr);
  const std::string bad = dm_sidereal_check(nt_in, ntime, a, phi0, dphi, 1.0);
  if (!bad.empty()) {
    printf("bad %s\n", bad.c_str());
    return 1;
  }
  dm_sidereal_geom g;
  dm_sidereal_geometry(nt_in, ntime, a, phi0, dphi, &g);
  for (int k = 0; k < ntime; ++k) {
    printf("%d %d %d %a %a", g.first[k], g.span[k], g.ntaps[k], g.a_all[k], g.s_all[k]);
    for (int t = 0; t < g.span[k]; ++t) printf(" %a", g.coef[(size_t)t * ntime + k]);
    printf("\n");
  }
  printf("tiles");
  for (int v : g.tiles) printf(" %d", v);
  printf("\nspan_max %d T %d\n", g.span_max, g.ntaps_max);
  return 0;
}
