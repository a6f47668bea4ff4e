// csrc/attention_keep.h checked on the host against a brute-force walk over positions: for every geometry, mode and prefix pair
// the kept 128-position tiles (forward, dQ) and the kept 32-position blocks (the streamed side of the fused dK / dV /
// bias-gradient kernel) are exactly the units that hold a kept query position, in rising order, and "no limit" is every unit
// in place -- the gap units between text and image positions included, which is what the kernels walked before the limit existed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attention_keep.h"

static int fails = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      if (fails++ < 20) { std::printf("FAIL %s:%d  ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                       \
  } while (0)

// units of [org, lim) that hold a kept position, by brute force
static std::vector<int> brute(int n0, int n1, int pos1, int k0, int k1, int org, int lim, int unit) {
  const bool all = k0 <= 0 && k1 <= 0;
  const int kt = all ? n0 : (k0 < n0 ? k0 : n0), ki = all ? n1 : (k1 < n1 ? k1 : n1);
  std::vector<int> out;
  const int full = (lim - org + unit - 1) / unit;
  for (int u = 0; u < full; ++u) {
    bool any = all;  // no limit: every unit, as the kernels always walked them
    for (int p = org + u * unit; p < org + (u + 1) * unit && p < lim && !any; ++p)
      any = (p < kt) || (p >= pos1 && p < pos1 + ki);
    if (any) out.push_back(u);
  }
  return out;
}

static void check_run(const att_keep_run_t& r, const std::vector<int>& want, int full, const char* what, int n0, int n1, int pos1,
                      int k0, int k1) {
  CHECK(r.n == (int)want.size(), "%s n0=%d n1=%d pos1=%d keep=(%d,%d): %d units, want %zu", what, n0, n1, pos1, k0, k1, r.n, want.size());
  for (int i = 0; i < r.n && i < (int)want.size(); ++i)
    CHECK(att_keep_unit(r, i) == want[i], "%s n0=%d n1=%d pos1=%d keep=(%d,%d): unit %d is %d, want %d", what, n0, n1, pos1, k0, k1, i,
          att_keep_unit(r, i), want[i]);
  for (int u = 0; u < full; ++u) {
    bool in = false;
    for (int w : want) in = in || w == u;
    CHECK(att_keep_has(r, u) == in, "%s n0=%d n1=%d pos1=%d keep=(%d,%d): has(%d)", what, n0, n1, pos1, k0, k1, u);
  }
}

int main() {
  const int n0s[] = {0, 1, 8, 40, 64, 65, 100, 130, 200};
  const int n1s[] = {0, 1, 31, 88, 145, 197, 577, 901};
  const int ks[] = {0, 1, 2, 31, 32, 33, 40, 127, 128, 129, 145, 500, 100000};
  long cases = 0;
  for (int n0 : n0s)
    for (int n1 : n1s)
      for (int gap = 0; gap <= 136; gap += 8) {
        const int pos1 = (n0 + 7) / 8 * 8 + gap;
        if (gap > 16 && gap != 64 && gap != 136) continue;
        if (n0 + n1 == 0) continue;
        const int NP = pos1 + n1;
        for (int k0 : ks)
          for (int k1 : ks) {
            ++cases;
            const att_keep_t k = att_keep_limits(n0, n1, pos1, k0, k1);
            CHECK(k.qt >= 0 && k.qt <= n0 && k.qe >= pos1 && k.qe <= NP, "limits n0=%d n1=%d keep=(%d,%d): %d %d", n0, n1, k0, k1, k.qt, k.qe);
            if (k0 <= 0 && k1 <= 0) CHECK(k.qt == n0 && k.qe == NP, "no limit is every position");
            // JOINT: one part from position 0
            for (int unit : {128, 32}) {
              const int full = (NP + unit - 1) / unit;
              check_run(att_keep_run(n0, n1, pos1, k0, k1, true, 0, unit, full), brute(n0, n1, pos1, k0, k1, 0, NP, unit), full,
                        unit == 128 ? "joint tiles" : "joint blocks", n0, n1, pos1, k0, k1);
            }
            check_run(att_keep_tiles(n0, n1, pos1, k0, k1, 0), brute(n0, n1, pos1, k0, k1, 0, NP, 128), (NP + 127) / 128,
                      "joint launch", n0, n1, pos1, k0, k1);
            // SEPARATE: the text part from 0, the image part from pos1; the launch numbers text tiles first
            const int f0 = (n0 + 31) / 32, f1 = (n1 + 31) / 32;
            const std::vector<int> b0 = brute(n0, n1, pos1, k0, k1, 0, n0, 32), b1 = brute(n0, n1, pos1, k0, k1, pos1, NP, 32);
            check_run(att_keep_run(n0, n1, pos1, k0, k1, false, 0, 32, f0), b0, f0, "text blocks", n0, n1, pos1, k0, k1);
            check_run(att_keep_run(n0, n1, pos1, k0, k1, false, 1, 32, f1), b1, f1, "image blocks", n0, n1, pos1, k0, k1);
            const int nt0 = (n0 + 127) / 128, nt1 = (n1 + 127) / 128;
            std::vector<int> tiles = brute(n0, n1, pos1, k0, k1, 0, n0, 128);
            for (int u : brute(n0, n1, pos1, k0, k1, pos1, NP, 128)) tiles.push_back(nt0 + u);
            check_run(att_keep_tiles(n0, n1, pos1, k0, k1, 1), tiles, nt0 + nt1, "separate launch", n0, n1, pos1, k0, k1);
            // the anchor of a part is a kept position of that part, and exists exactly when the part keeps a query
            const int parts[3][2] = {{0, NP}, {0, n0}, {pos1, NP}};
            for (const auto& pt : parts) {
              bool any = false;
              for (int p = pt[0]; p < pt[1]; ++p) any = any || ((p < n0 || p >= pos1) && att_keep_pos(k, pos1, p));
              const int a = att_keep_anchor(k, pos1, pt[0], pt[1]);
              CHECK((a >= 0) == any, "anchor n0=%d n1=%d pos1=%d keep=(%d,%d) part [%d,%d): %d", n0, n1, pos1, k0, k1, pt[0], pt[1], a);
              if (a >= 0) CHECK(a >= pt[0] && a < pt[1] && att_keep_pos(k, pos1, a) && (a < n0 || a >= pos1), "anchor %d is not a kept position", a);
            }
          }
      }
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("attention keep ok (%ld cases)\n", cases);
  return 0;
}
