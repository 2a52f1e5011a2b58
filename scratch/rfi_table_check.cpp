// The argument check and the tables of dm_rfi_flag (driftscan_amd/csrc/dm_rfi_table.h) on the host alone, for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idriftscan_amd/csrc \
//       scratch/rfi_table_check.cpp -o scratch/bin/rfi_table_check
//   scratch/bin/rfi_table_check NT SEGMENT SIGMA CHI1 RHO NITER BASE MIN_GOOD ROW_SHARE M...   (reals as C99 hex floats)
// prints "H <H>", "g <g_0> ... <g_H>" and one line "t <it> ..." per iteration (hex floats), or "bad <why>".
// scratch/rfi_table_check.py builds it, runs it on the parameter sets of the tests and compares every number with
// timestream.rfi_tables_host.
#include "dm_rfi_table.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const int nt = atoi(argv[1]), segment = atoi(argv[2]);
  const double sigma = strtod(argv[3], nullptr), chi1 = strtod(argv[4], nullptr), rho = strtod(argv[5], nullptr);
  const int niter = atoi(argv[6]);
  const double base = strtod(argv[7], nullptr);
  const int min_good = atoi(argv[8]);
  const double row_share = strtod(argv[9], nullptr);
  std::vector<int> win;
  for (int i = 10; i < argc; ++i) win.push_back(atoi(argv[i]));
  const std::string bad = dm_rfi_check(nt, segment, sigma, (int)win.size(), win.empty() ? nullptr : win.data(), chi1, rho,
                                       niter, base, min_good, row_share);
  if (!bad.empty()) {
    printf("bad %s\n", bad.c_str());
    return 1;
  }
  dm_rfi_tables tb;
  dm_rfi_make_tables(sigma, (int)win.size(), win.data(), chi1, rho, niter, base, min_good, &tb);
  printf("H %d\ng", tb.H);
  for (int d = 0; d <= tb.H; ++d) printf(" %a", tb.g[d]);
  printf("\n");
  for (int it = 0; it < tb.niter; ++it) {
    printf("t %d", it);
    for (int i = 0; i < tb.nwin; ++i) printf(" %a", tb.t[it][i]);
    printf("\n");
  }
  return 0;
}
