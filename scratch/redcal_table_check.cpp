// Stand-alone check of the host side of dm_redcal_solve (driftscan_amd/csrc/dm_redcal_table.h): the member factors with
// the "fewer than two" rule, the feed-major incidence table, the argument checks and the split of the feeds, and of
// dm_modelcal_solve (dm_modelcal_table.h: the same table without that rule, the intervals, its argument checks), meant to be
// built with the address and undefined-behaviour sanitizers on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scratch/redcal_table_check.cpp -o redcal_table_check
// Every table is a heap allocation of exactly its size, so a read past a table's end is reported.
#include "../driftscan_amd/csrc/dm_modelcal_table.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int failures = 0;

static void check(const char* what, bool ok) {
  std::printf("%-52s %s\n", what, ok ? "ok  " : "FAIL");
  if (!ok) ++failures;
}

// What the kernels rely on: inc_off ascends from 0 to the number of incidences, every constrained member is listed once
// under each of its two feeds, in member order, with the right partner, class and side, and nothing else is listed.
static bool table_sound(int nfeed, const std::vector<int>& off, const std::vector<int>& mem, const std::vector<double>& fw,
                        int min_live = 2) {
  const int npairs = (int)off.size() - 1;
  const dm_redcal_table t = dm_redcal_build(nfeed, npairs, off.data(), mem.data(), fw.empty() ? nullptr : fw.data(), min_live);
  const int nmem = off.back();
  if ((int)t.yfac.size() != nmem || (int)t.gfac.size() != nmem || (int)t.inc_off.size() != nfeed + 1) return false;
  if (t.inc_off[0] != 0 || t.inc_off[nfeed] != (int)t.inc.size()) return false;
  std::vector<int> cls((size_t)nmem);
  int constrained = 0;
  for (int c = 0; c < npairs; ++c) {
    int live = 0;
    for (int k = off[c]; k < off[c + 1]; ++k) {
      cls[k] = c;
      const int i = mem[2 * k], j = mem[2 * k + 1];
      const double fac = fw.empty() ? 1.0 : fw[i] * fw[j];
      const double want = i != j ? fac : 0.0;
      if (t.yfac[k] != want) return false;
      live += want > 0.0;
    }
    constrained += live >= min_live;
    for (int k = off[c]; k < off[c + 1]; ++k)
      if (t.gfac[k] != (live >= min_live ? t.yfac[k] : 0.0)) return false;
  }
  if (constrained != t.nconstrained) return false;
  std::vector<int> seen((size_t)nmem, 0);
  for (int a = 0; a < nfeed; ++a) {
    if (t.inc_off[a + 1] < t.inc_off[a]) return false;
    int before = -1;
    for (int k = t.inc_off[a]; k < t.inc_off[a + 1]; ++k) {
      const dm_redcal_inc& e = t.inc[k];
      if (e.row <= before || e.row >= nmem || !(t.gfac[e.row] > 0.0) || e.cls != cls[e.row]) return false;
      before = e.row;
      const int i = mem[2 * e.row], j = mem[2 * e.row + 1];
      if (e.side == 0 ? (i != a || e.partner != j) : (e.side != 1 || j != a || e.partner != i)) return false;
      ++seen[e.row];
    }
  }
  for (int k = 0; k < nmem; ++k)
    if (seen[k] != (t.gfac[k] > 0.0 ? 2 : 0)) return false;
  // the split covers [0, nfeed) in ascending, non-empty feed ranges, for few and many cells
  for (int64_t cells : {0, 1, 7, 4096}) {
    const std::vector<int> c = dm_redcal_chunks(nfeed, t.inc_off.data(), cells);
    if (c.size() < 2 || c.front() != 0 || c.back() != nfeed) return false;
    for (size_t q = 0; q + 1 < c.size(); ++q)
      if (c[q] >= c[q + 1] && nfeed > 0) return false;
  }
  return true;
}

int main() {
  // the 3-feed line: autos, the two nearest-neighbour pairs (constrained), the long baseline alone (not)
  const std::vector<int> off3{0, 3, 5, 6}, mem3{0, 0, 1, 1, 2, 2, 1, 0, 2, 1, 2, 0};
  check("3-feed line", table_sound(3, off3, mem3, {}));
  {
    const dm_redcal_table t = dm_redcal_build(3, 3, off3.data(), mem3.data(), nullptr);
    check("3-feed line: one constrained class, 4 incidences", t.nconstrained == 1 && t.inc.size() == 4 && t.gfac[5] == 0.0 &&
                                                                  t.yfac[5] == 1.0 && t.yfac[0] == 0.0);
    const double fw[3] = {1.0, 0.0, 2.0};
    const dm_redcal_table d = dm_redcal_build(3, 3, off3.data(), mem3.data(), fw);
    check("3-feed line, middle feed dead: nothing constrained", d.nconstrained == 0 && d.inc.empty() && d.yfac[5] == 2.0);
  }
  check("two feeds: nothing constrained", table_sound(2, {0, 2, 3, 4}, {0, 0, 1, 1, 1, 0, 0, 1}, {}));
  check("one autocorrelation", table_sound(1, {0, 1}, {0, 0}, {}));
  std::mt19937 rng(3);
  for (int trial = 0; trial < 60; ++trial) {
    const int nfeed = 1 + (int)(rng() % 400), npairs = 1 + (int)(rng() % 300);
    std::vector<int> off(1, 0), mem;
    for (int c = 0; c < npairs; ++c) off.push_back(off.back() + 1 + (int)(rng() % (trial % 3 ? 6 : 200)));
    for (int k = 0; k < 2 * off.back(); ++k) mem.push_back((int)(rng() % nfeed));
    std::vector<double> fw;
    if (trial % 2)
      for (int a = 0; a < nfeed; ++a) fw.push_back(rng() % 5 ? 0.5 + (rng() % 100) / 100.0 : 0.0);
    check("random table", table_sound(nfeed, off, mem, fw));
    check("random table, every class of a live member counts", table_sound(nfeed, off, mem, fw, 1));
  }
  {  // a table that needs several chunks: 600 feeds, 40000 members
    const int nfeed = 600;
    std::vector<int> off(1, 0), mem;
    for (int c = 0; c < 400; ++c) off.push_back(off.back() + 100);
    for (int k = 0; k < 2 * off.back(); ++k) mem.push_back((int)(rng() % nfeed));
    check("40000 members of 600 feeds", table_sound(nfeed, off, mem, {}));
    const dm_redcal_table t = dm_redcal_build(nfeed, 400, off.data(), mem.data(), nullptr);
    check("  ... split into more than one chunk for one cell", dm_redcal_chunks(nfeed, t.inc_off.data(), 1).size() > 2);
  }
  {  // without the "fewer than two" rule (dm_modelcal_solve): the long baseline of the 3-feed line and a single cross pair count
    const dm_redcal_table t = dm_redcal_build(3, 3, off3.data(), mem3.data(), nullptr, 1);
    check("3-feed line, min_live 1: two classes, 6 incidences", t.nconstrained == 2 && t.inc.size() == 6 && t.gfac[5] == 1.0 &&
                                                                    t.gfac[0] == 0.0);
    check("two feeds, min_live 1", table_sound(2, {0, 2, 3, 4}, {0, 0, 1, 1, 1, 0, 0, 1}, {}, 1));
    check("intervals", dm_modelcal_nint(150, 64) == 3 && dm_modelcal_nint(17, 4) == 5 && dm_modelcal_nint(5, 1) == 5 &&
                           dm_modelcal_nint(3, 100) == 1 && dm_modelcal_nint(0, 4) == 0);
    check("modelcal: sound arguments", dm_modelcal_args_check(4092, 1, 0.5, 1e-10, 500).empty());
    check("modelcal: interval 0", dm_modelcal_args_check(12, 0, 0.5, 1e-10, 500).find("interval") != std::string::npos);
    check("modelcal: 4093 feeds", dm_modelcal_args_check(4093, 16, 0.5, 1e-10, 500).find("does not fit") != std::string::npos);
    check("modelcal: damping 0", dm_modelcal_args_check(12, 16, 0.0, 1e-10, 500).find("damping") != std::string::npos);
  }
  {  // the table goes to the device as it is: an incidence read as four ints is (row, partner, cls, side)
    const dm_redcal_table t = dm_redcal_build(3, 3, off3.data(), mem3.data(), nullptr, 1);
    std::vector<int> flat(4 * t.inc.size());
    std::memcpy(flat.data(), t.inc.data(), flat.size() * sizeof(int));
    bool same = !t.inc.empty();
    for (size_t k = 0; k < t.inc.size(); ++k)
      same = same && flat[4 * k] == t.inc[k].row && flat[4 * k + 1] == t.inc[k].partner && flat[4 * k + 2] == t.inc[k].cls &&
             flat[4 * k + 3] == t.inc[k].side;
    check("an incidence is the int4 (row, partner, cls, side)", same);
  }
  {  // the opening of the two solvers: the shared argument check and the spans of dm_redcal_solve
    const int two = 2, three = 3;
    const double dead[3] = {1.0, 0.0, 1.0}, minus[3] = {1.0, 1.0, -1.0};
    auto open = [&](int nreal, int64_t rs, const int* wn, const int* mn, const double* fw) {
      return dm_pair_args_check(nreal, 1, 3, 3, 5, rs, wn, mn, off3.data(), mem3.data(), true, fw);
    };
    check("solver opening: sound", open(2, 0, &two, &two, dead).empty() && open(2, 0, nullptr, nullptr, nullptr).empty());
    check("solver opening: negative size", open(-1, 0, nullptr, nullptr, nullptr) == "negative size" &&
                                               open(2, -1, nullptr, nullptr, nullptr) == "negative size");
    check("solver opening: w_nreal", open(2, 0, &three, &two, nullptr) == "w_nreal must be 1 or nreal");
    check("solver opening: m_nreal", open(2, 0, &two, &three, nullptr) == "m_nreal must be 1 or nreal");
    check("solver opening: feed weight", open(2, 0, nullptr, nullptr, minus) == "feed weight 2 is negative");
    std::vector<char> buf(1000);
    const char* b = buf.data();
    const dm_span in[3] = {{b, 300, "vis"}, {nullptr, 0, "w"}, {nullptr, 0, "g0"}};
    const dm_span apart[5] = {{b + 300, 100, "g"}, {b + 400, 100, "y"}, {b + 500, 20, "iters"}, {b + 520, 40, "step"}, {b + 560, 40, "chi2"}};
    const dm_span on_vis[5] = {{b + 300, 100, "g"}, {b + 299, 100, "y"}, {b + 500, 20, "iters"}, {b + 520, 40, "step"}, {b + 560, 40, "chi2"}};
    const dm_span on_out[5] = {{b + 300, 100, "g"}, {b + 400, 100, "y"}, {b + 500, 20, "iters"}, {b + 519, 40, "step"}, {b + 560, 40, "chi2"}};
    const dm_span none[5] = {{b, 0, "g"}, {b, 0, "y"}, {b, 0, "iters"}, {b, 0, "step"}, {b, 0, "chi2"}};
    check("spans: disjoint", dm_spans_shared(in, 3, apart, 5).empty());
    check("spans: y on vis (the input is named first)", dm_spans_shared(in, 3, on_vis, 5) == "y shares an element with vis");
    check("spans: step on iters", dm_spans_shared(in, 3, on_out, 5) == "step shares an element with iters");
    check("spans: zero-length outputs", dm_spans_shared(in, 3, none, 5).empty());
  }
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  check("sound arguments", dm_redcal_args_check(0.4, 1e-10, 500).empty() && dm_redcal_args_check(1.0, 0.0, 1).empty());
  check("damping 0", dm_redcal_args_check(0.0, 1e-10, 500).find("damping") != std::string::npos);
  check("damping above 1", dm_redcal_args_check(1.0000001, 1e-10, 500).find("damping") != std::string::npos);
  check("damping NaN", dm_redcal_args_check(nan, 1e-10, 500).find("damping") != std::string::npos);
  check("tol negative", dm_redcal_args_check(0.4, -1e-300, 500).find("tol") != std::string::npos);
  check("tol infinite", dm_redcal_args_check(0.4, inf, 500).find("tol") != std::string::npos);
  check("tol NaN", dm_redcal_args_check(0.4, nan, 500).find("tol") != std::string::npos);
  check("maxiter 0", dm_redcal_args_check(0.4, 1e-10, 0).find("maxiter") != std::string::npos);
  std::printf("%d failures\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
