// Stand-alone check of the host-side refusals of dm_ts_gain_apply (driftscan_amd/csrc/dm_gain_table.h), meant to be built
// with the address and undefined-behaviour sanitizers on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scratch/gain_table_check.cpp -o gain_table_check
// Every table is a heap allocation of exactly its size, so a read past a table's end is reported.
#include "../driftscan_amd/csrc/dm_gain_table.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;

static void expect(const char* what, int nfeed, const std::vector<int>& off, const std::vector<int>& mem, const char* needle) {
  const int npairs = off.empty() ? 0 : (int)off.size() - 1;
  const std::string r = dm_gain_table_check(nfeed, npairs, off.empty() ? nullptr : off.data(), mem.empty() ? nullptr : mem.data());
  const bool ok = needle ? r.find(needle) != std::string::npos : r.empty();
  std::printf("%-28s %s  [%s]\n", what, ok ? "ok  " : "FAIL", r.c_str());
  if (!ok) ++failures;
}

int main() {
  expect("sound table", 3, {0, 2, 3}, {0, 1, 1, 2, 2, 0}, nullptr);
  expect("single auto-correlation", 1, {0, 1}, {0, 0}, nullptr);
  expect("no classes", 5, {}, {}, nullptr);
  expect("empty class", 3, {0, 2, 2}, {0, 1, 1, 2}, "class 1 is empty");
  expect("empty first class", 3, {0, 0, 1}, {0, 1}, "class 0 is empty");
  expect("descending offsets", 3, {0, 2, 1}, {0, 1, 1, 2}, "class 1 is empty");
  expect("feed index = nfeed", 3, {0, 1, 2}, {0, 1, 3, 2}, "names feed 3 of 3");
  expect("negative feed index", 3, {0, 1, 2}, {0, -1, 1, 2}, "names feed -1");
  expect("offsets not from 0", 3, {1, 2, 3}, {0, 1, 1, 2, 0, 2}, "class_off[0]");
  expect("null members", 3, {0, 1}, {}, "null pair table");
  expect("nfeed past the LDS", 10241, {0, 1}, {0, 0}, "does not fit");
  expect("nfeed at the LDS", 10240, {0, 1}, {10239, 0}, nullptr);
  // a long line: the largest tables the tests use
  const int n = 4200;
  std::vector<int> off{0, n - 1}, mem;
  for (int i = 0; i + 1 < n; ++i) { mem.push_back(i + 1); mem.push_back(i); }
  expect("line of 4200 feeds", n, off, mem, nullptr);
  const int tiles[][2] = {{1, 16}, {256, 16}, {257, 8}, {512, 8}, {513, 4}, {1024, 4}, {1025, 2}, {2048, 2}, {2049, 1},
                          {4096, 1}, {4097, 1}, {10240, 1}, {10241, 0}};
  for (const auto& t : tiles)
    if (dm_gain_tile(t[0]) != t[1]) { std::printf("tile(%d) = %d, not %d\n", t[0], dm_gain_tile(t[0]), t[1]); ++failures; }
  std::printf("%d failures\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
