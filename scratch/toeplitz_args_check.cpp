// Stand-alone check of the host-side sizing and argument checks of dm_toeplitz_solve (driftscan_amd/csrc/dm_toeplitz_args.h),
// meant for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scratch/toeplitz_args_check.cpp -o /tmp/tzc && /tmp/tzc
#include "../driftscan_amd/csrc/dm_toeplitz_args.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
      ++failures;                                                  \
    }                                                              \
  } while (0)

int main() {
  int dummy = 0;
  const void* p = &dummy;
  // the limit: the largest nrhs fits, one more does not, for every order that fits at all
  for (int n = 1; n <= 4000; ++n) {
    const int most = dm_toeplitz_max_rhs_of(n);
    CHECK(most >= 0);
    if (most > 0 && most < 65535) {
      CHECK(dm_toeplitz_lds(n, most) <= DM_TOEPLITZ_LDS_BYTES);
      CHECK(dm_toeplitz_lds(n, most + 1) > DM_TOEPLITZ_LDS_BYTES);
    }
    if (most == 0) CHECK(dm_toeplitz_lds(n, 1) > DM_TOEPLITZ_LDS_BYTES);
    CHECK(dm_toeplitz_check(n, most > 0 ? most : 1, 1, p, p, p).empty() == (most > 0));
    CHECK(!dm_toeplitz_check(n, most + 1, 1, p, p, p).empty());
  }
  CHECK(dm_toeplitz_max_rhs_of(1025) == 7 && dm_toeplitz_max_rhs_of(2049) == 2);
  CHECK(dm_toeplitz_max_rhs_of(3410) == 1 && dm_toeplitz_max_rhs_of(3411) == 0);
  CHECK(dm_toeplitz_max_rhs_of(0) == 0 && dm_toeplitz_max_rhs_of(-5) == 0 && dm_toeplitz_max_rhs_of(2147483647) == 0);
  // 8 right-hand sides of order 1025 exceed the limit by the vectors alone
  CHECK((2 + 8) * 1025 * 16 > DM_TOEPLITZ_LDS_BYTES);
  // refusals
  CHECK(!dm_toeplitz_check(0, 1, 1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(-1, 1, 1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(4, 0, 1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(4, -3, 1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(4, 1, -1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(4, 1, 1, nullptr, p, p).empty());
  CHECK(!dm_toeplitz_check(4, 1, 1, p, nullptr, p).empty());
  CHECK(!dm_toeplitz_check(4, 1, 1, p, p, nullptr).empty());
  CHECK(!dm_toeplitz_check(2147483647, 1, 1, p, p, p).empty());
  CHECK(!dm_toeplitz_check(4, 2147483647, 1, p, p, p).empty());
  // accepted
  CHECK(dm_toeplitz_check(4, 1, 0, nullptr, nullptr, nullptr).empty());   // batch = 0 is a no-op
  CHECK(dm_toeplitz_check(1, 1, 2147483647, p, p, p).empty());
  CHECK(dm_toeplitz_check(257, 8, 100000, p, p, p).empty());
  // dm_toeplitz_solve_diag: nrhs = 0 allowed (b null or not), diag required, the same limits otherwise
  CHECK(dm_toeplitz_check_diag(4, 0, 1, p, nullptr, p, p).empty());
  CHECK(dm_toeplitz_check_diag(4, 0, 1, p, p, p, p).empty());
  CHECK(dm_toeplitz_check_diag(4, 1, 1, p, p, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, -1, 1, p, p, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 1, 1, p, nullptr, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 0, 1, p, p, nullptr, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 0, 1, nullptr, p, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 0, 1, p, p, p, nullptr).empty());
  CHECK(!dm_toeplitz_check_diag(0, 0, 1, p, p, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 0, -1, p, p, p, p).empty());
  CHECK(dm_toeplitz_check_diag(4, 0, 0, nullptr, nullptr, nullptr, nullptr).empty());
  CHECK(!dm_toeplitz_check_diag(4, dm_toeplitz_max_rhs_of(4) + 1, 1, p, p, p, p).empty());
  CHECK(dm_toeplitz_check_diag(5117, 0, 1, p, nullptr, p, p).empty() && dm_toeplitz_lds(5117, 0) <= DM_TOEPLITZ_LDS_BYTES);
  CHECK(!dm_toeplitz_check_diag(5118, 0, 1, p, nullptr, p, p).empty() && dm_toeplitz_lds(5118, 0) > DM_TOEPLITZ_LDS_BYTES);
  CHECK(!dm_toeplitz_check_diag(2147483647, 0, 1, p, nullptr, p, p).empty());
  CHECK(!dm_toeplitz_check_diag(4, 2147483647, 1, p, p, p, p).empty());
  std::printf(failures ? "%d checks failed\n" : "toeplitz argument checks ok\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
