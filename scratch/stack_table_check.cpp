// Stand-alone check of the host-side refusals and the workgroup split of dm_vis_stack / dm_vis_expand
// (driftscan_amd/csrc/dm_stack_table.h), meant to be built with the address and undefined-behaviour sanitizers on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scratch/stack_table_check.cpp -o stack_table_check
// Every table is a heap allocation of exactly its size, so a read past a table's end is reported.
#include "../driftscan_amd/csrc/dm_stack_table.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static int failures = 0;

static void expect(const char* what, int nfeed, const std::vector<int>& off, const std::vector<int>& mem, bool has_g,
                   const char* needle) {
  const int npairs = off.empty() ? 0 : (int)off.size() - 1;
  const std::string r =
      dm_stack_table_check(nfeed, npairs, off.empty() ? nullptr : off.data(), mem.empty() ? nullptr : mem.data(), has_g);
  const bool ok = needle ? r.find(needle) != std::string::npos : r.empty();
  std::printf("%-34s %s  [%s]\n", what, ok ? "ok  " : "FAIL", r.c_str());
  if (!ok) ++failures;
}

// the chunks cover [0, npairs) in ascending, non-empty class ranges
static void chunks_sound(const char* what, const std::vector<int>& off, int64_t cells) {
  const int npairs = (int)off.size() - 1;
  const std::vector<int> c = dm_stack_chunks(npairs, off.data(), cells);
  bool ok = c.size() >= 2 && c.front() == 0 && c.back() == npairs;
  for (size_t q = 0; ok && q + 1 < c.size(); ++q) ok = c[q] < c[q + 1];
  std::printf("%-34s %s  [%zu chunks for %lld cells]\n", what, ok ? "ok  " : "FAIL", c.size() - 1, (long long)cells);
  if (!ok) ++failures;
}

int main() {
  expect("sound table", 3, {0, 2, 3}, {0, 1, 1, 2, 2, 0}, true, nullptr);
  expect("single auto-correlation", 1, {0, 1}, {0, 0}, false, nullptr);
  expect("no classes", 5, {}, {}, true, nullptr);
  expect("empty class", 3, {0, 2, 2}, {0, 1, 1, 2}, true, "class 1 is empty");
  expect("empty first class", 3, {0, 0, 1}, {0, 1}, false, "class 0 is empty");
  expect("descending offsets", 3, {0, 2, 1}, {0, 1, 1, 2}, false, "class_off decreases at class 1");
  expect("feed index = nfeed", 3, {0, 1, 2}, {0, 1, 3, 2}, true, "names feed 3 of 3");
  expect("negative feed index", 3, {0, 1, 2}, {0, -1, 1, 2}, false, "names feed -1");
  expect("offsets not from 0", 3, {1, 2, 3}, {0, 1, 1, 2, 0, 2}, true, "class_off[0]");
  expect("null members", 3, {0, 1}, {}, false, "null class table");
  expect("negative nfeed", -1, {0, 1}, {0, 0}, false, "negative size");
  expect("nfeed past the LDS, with gains", 10241, {0, 1}, {0, 0}, true, "does not fit");
  expect("nfeed past the LDS, no gains", 10241, {0, 1}, {10240, 0}, false, nullptr);
  expect("nfeed at the LDS", 10240, {0, 1}, {10239, 0}, true, nullptr);
  if (dm_stack_tile(512, true) != 8 || dm_stack_tile(512, false) != 16 || dm_stack_tile(10241, true) != 0 ||
      dm_stack_tile(10241, false) != 16) {
    std::printf("dm_stack_tile FAIL\n");
    ++failures;
  }
  // splits: one class, classes of one, a long class among short ones, random lengths, few and many cells
  chunks_sound("one class", {0, 5000}, 1);
  std::vector<int> ones(1, 0);
  for (int c = 1; c <= 20000; ++c) ones.push_back(c);
  chunks_sound("20000 classes of one, 1 cell", ones, 1);
  chunks_sound("20000 classes of one, 4096 cells", ones, 4096);
  std::vector<int> mixed{0, 100000};
  for (int c = 0; c < 3000; ++c) mixed.push_back(mixed.back() + 1);
  chunks_sound("a long class before short ones", mixed, 3);
  std::mt19937 rng(1);
  for (int trial = 0; trial < 50; ++trial) {
    std::vector<int> off(1, 0);
    const int npairs = 1 + (int)(rng() % 4000);
    for (int c = 0; c < npairs; ++c) off.push_back(off.back() + 1 + (int)(rng() % 300));
    chunks_sound("random lengths", off, 1 + (int64_t)(rng() % 600));
  }
  chunks_sound("no cells", {0, 3, 4}, 0);
  // span overlap
  struct { uint64_t a, ar, as, b, br, bs; int64_t n; bool want; } spans[] = {
      {1000, 100, 100, 1100, 100, 100, 1, false}, {1000, 100, 100, 1099, 100, 100, 1, true},
      {1000, 100, 400, 1100, 100, 400, 3, true},  {1000, 100, 100, 1300, 50, 50, 3, false},
      {1000, 0, 0, 1000, 100, 100, 2, false},     {1000, 100, 100, 1000, 100, 100, 0, false}};
  for (const auto& s : spans)
    if (dm_spans_overlap(s.a, s.ar, s.as, s.b, s.br, s.bs, s.n) != s.want) {
      std::printf("dm_spans_overlap FAIL at a = %llu, b = %llu\n", (unsigned long long)s.a, (unsigned long long)s.b);
      ++failures;
    }
  // the arguments the feed-pair entries share: each refusal once, in the order of the checks, and a sound call
  {
    const std::vector<int> off{0, 2, 3}, mem{0, 1, 1, 2, 0, 2}, empty_class{0, 2, 2};
    const std::vector<double> fw{1.0, 0.0, 2.0}, fw_neg{1.0, -0.5, 2.0}, fw_nan{1.0, 1.0, std::nan("")};
    const int one = 1, two = 2, three = 3;
    struct {
      const char* what;
      int nreal, ntime;
      int64_t rstride;
      const int *w_nreal, *m_nreal, *off;
      const double* fw;
      const char* needle;
    } args[] = {{"sound, nothing optional", 2, 5, 0, nullptr, nullptr, off.data(), nullptr, nullptr},
                {"sound, w and model per realisation", 2, 5, 64, &two, &two, off.data(), fw.data(), nullptr},
                {"sound, w and model shared", 2, 5, 64, &one, &one, off.data(), fw.data(), nullptr},
                {"negative ntime", 2, -1, 0, nullptr, nullptr, off.data(), nullptr, "negative size"},
                {"negative stride", 2, 5, -1, nullptr, nullptr, off.data(), nullptr, "negative size"},
                {"w_nreal 3 of 2", 2, 5, 0, &three, &two, off.data(), nullptr, "w_nreal must be 1 or nreal"},
                {"m_nreal 3 of 2", 2, 5, 0, &two, &three, off.data(), nullptr, "m_nreal must be 1 or nreal"},
                {"an empty class", 2, 5, 0, nullptr, nullptr, empty_class.data(), nullptr, "class 1 is empty"},
                {"a negative feed weight", 2, 5, 0, nullptr, nullptr, off.data(), fw_neg.data(), "feed weight 1 is negative"},
                {"a NaN feed weight", 2, 5, 0, nullptr, nullptr, off.data(), fw_nan.data(), "feed weight 2 is negative"}};
    for (const auto& a : args) {
      const std::string r = dm_pair_args_check(a.nreal, 1, 3, 2, a.ntime, a.rstride, a.w_nreal, a.m_nreal, a.off, mem.data(), true, a.fw);
      const bool ok = a.needle ? r == a.needle : r.empty();
      std::printf("%-34s %s  [%s]\n", a.what, ok ? "ok  " : "FAIL", r.c_str());
      if (!ok) ++failures;
    }
  }
  // named spans: disjoint, an output on an input, an output on an earlier output, zero-length spans anywhere
  {
    std::vector<char> buf(400);
    const char* b = buf.data();
    struct {
      const char* what;
      dm_span in[2], out[2];
      const char* want;
    } cases[] = {{"disjoint", {{b, 100, "vis"}, {b + 100, 100, "w"}}, {{b + 200, 100, "g"}, {b + 300, 100, "y"}}, ""},
                 {"g ends inside w", {{b, 100, "vis"}, {b + 150, 100, "w"}}, {{b + 100, 51, "g"}, {b + 300, 100, "y"}},
                  "g shares an element with w"},
                 {"y begins inside g", {{b, 100, "vis"}, {b + 100, 100, "w"}}, {{b + 200, 100, "g"}, {b + 299, 100, "y"}},
                  "y shares an element with g"},
                 {"inputs may overlap", {{b, 100, "vis"}, {b + 50, 100, "w"}}, {{b + 200, 100, "g"}, {b + 300, 100, "y"}}, ""},
                 {"zero-length spans", {{b + 250, 0, "vis"}, {nullptr, 0, "w"}}, {{b + 200, 100, "g"}, {b + 210, 0, "y"}}, ""}};
    for (const auto& c : cases) {
      const std::string r = dm_spans_shared(c.in, 2, c.out, 2);
      const bool ok = r == c.want;
      std::printf("%-34s %s  [%s]\n", c.what, ok ? "ok  " : "FAIL", r.c_str());
      if (!ok) ++failures;
    }
    if (!dm_spans_shared(nullptr, 0, nullptr, 0).empty()) {
      std::printf("dm_spans_shared of nothing FAIL\n");
      ++failures;
    }
  }
  std::printf("%d failures\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
