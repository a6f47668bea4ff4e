// Host-only check of csrc/jacobi_schedule.h (no HIP, no GPU): the tournament a Jacobi sweep walks.  For p = 1 .. 9, 64 and a few
// larger sizes: every unordered pair of rows occurs exactly once per sweep, the pairs of a step are disjoint, every index lies in
// [0, p) with i < j, and the step and pair counts are what the launch uses.  Built with -fsanitize=address,undefined and run as a
// child process by tests/test_tsvm_cpu.py; exit status 0 = every check held.
#include "jacobi_schedule.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
    }                               \
  } while (0)

static void check(int p) {
  const int steps = jacobi_steps(p), pairs = jacobi_pairs(p);
  CHECK(steps == (p < 2 ? 0 : (p % 2 ? p : p - 1)), "p = %d: %d steps", p, steps);
  CHECK(pairs == (p < 2 ? 0 : p / 2), "p = %d: %d pairs", p, pairs);
  std::vector<int> met((size_t)p * p, 0);  // exactly p * p: the sanitizer sees an index past it
  for (int t = 0; t < steps; ++t) {
    std::vector<int> used((size_t)p, 0);
    for (int k = 0; k < pairs; ++k) {
      int i = -1, j = -1;
      jacobi_pair(p, t, k, &i, &j);
      CHECK(0 <= i && i < j && j < p, "p = %d step %d pair %d: (%d, %d) out of range", p, t, k, i, j);
      if (!(0 <= i && i < j && j < p)) continue;
      CHECK(!used[i] && !used[j], "p = %d step %d: row %d or %d sits in two pairs", p, t, i, j);
      used[i] = used[j] = 1;
      ++met[(size_t)i * p + j];
    }
  }
  for (int i = 0; i < p; ++i)
    for (int j = i + 1; j < p; ++j) CHECK(met[(size_t)i * p + j] == 1, "p = %d: pair (%d, %d) met %d times", p, i, j, met[(size_t)i * p + j]);
}

int main() {
  for (int p = 1; p <= 9; ++p) check(p);
  for (int p : {64, 65, 96, 767, 768}) check(p);
  if (failures) {
    fprintf(stderr, "jacobi_schedule_check: %d failures\n", failures);
    return 1;
  }
  printf("jacobi_schedule_check: ok\n");
  return 0;
}
