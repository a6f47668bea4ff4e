// The round-robin tournament a Jacobi sweep walks (csrc/jacobi.hip): every unordered pair of the p rows exactly once per sweep, the
// pairs of a step disjoint.  No HIP in here: tests/helpers/jacobi_schedule_check.cpp compiles it with the host compiler.
//
// The circle method on n = p rounded up to even: player n - 1 stays, the others rotate.  Step t in [0, n - 1) seats
//   slot 0:        n - 1            against  t
//   slot k >= 1:   (t + k) mod (n - 1)  against  (t - k) mod (n - 1)
// For odd p player n - 1 = p does not exist: slot 0 is the bye, so a step has floor(p / 2) real pairs in either case, and the real
// pair `pair` of a step sits in slot pair + (p & 1).
#pragma once

#if defined(__HIPCC__)
#define JACOBI_HD __host__ __device__
#else
#define JACOBI_HD
#endif

// steps per sweep: p - 1 for even p, p for odd p, 0 for p < 2
JACOBI_HD static inline int jacobi_steps(int p) { return p < 2 ? 0 : (p & 1) ? p : p - 1; }
// pairs per step
JACOBI_HD static inline int jacobi_pairs(int p) { return p < 2 ? 0 : p >> 1; }

// rows (i < j) of pair `pair` in [0, jacobi_pairs(p)) of step `step` in [0, jacobi_steps(p))
JACOBI_HD static inline void jacobi_pair(int p, int step, int pair, int* i, int* j) {
  const int n = p + (p & 1), ring = n - 1;
  const int k = pair + (p & 1);
  int a, b;
  if (k == 0) {
    a = n - 1;
    b = step;
  } else {
    a = (step + k) % ring;
    b = (step + ring - k) % ring;
  }
  *i = a < b ? a : b;
  *j = a < b ? b : a;
}
