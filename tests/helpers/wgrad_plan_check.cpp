// Host-side check of csrc/wgrad_plan.h (the slice plan of vlm_gemm_wgrad_batch / vlm_gemm_wgrad_grouped), compiled by
// tests/test_wgrad_plan_cpu.py with the host compiler under AddressSanitizer + UBSan.  No HIP, no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "wgrad_plan.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static const uint64_t WS_FLOATS = (96ull << 20) / 4;  // ops.SPLITK_WS_BYTES
static long n_plans = 0, n_refused = 0;

// every property the kernel and the reduce launch rely on, for one planned set
static void check_plan(int n, const wgrad_plan_in_t* in, int cus, const wgrad_plan_t& pl) {
  // each (problem, tile, K step) is covered by exactly one item: walk the grid the way the kernel decodes it
  std::vector<std::vector<int>> cover(n);
  for (int g = 0; g < n; ++g) cover[g].assign((size_t)in[g].tiles * in[g].ksteps, 0);
  CHECK(pl.items >= 1 && pl.items <= cus);
  for (int item = 0; item < pl.items; ++item) {
    int g = 0;  // the kernel's scalar compares; empty groups own no item and share their successor's item0
    for (int i = 1; i < n; ++i)
      if (item >= pl.g[i].item0) g = i;
    while (in[g].tiles == 0 || in[g].ksteps == 0) { CHECK(g > 0); --g; }  // (the callers pass live groups only)
    const int local = item - pl.g[g].item0;
    CHECK(local >= 0);
    const int split = local / in[g].tiles, tile = local - split * in[g].tiles;
    CHECK(split < pl.g[g].splits);
    for (int k = split * pl.g[g].kps; k < (split + 1) * pl.g[g].kps && k < in[g].ksteps; ++k) ++cover[g][(size_t)tile * in[g].ksteps + k];
  }
  int items = 0, slices = 0;
  uint64_t floats = 0;
  for (int g = 0; g < n; ++g) {
    for (int c : cover[g]) CHECK(c == 1);
    const wgrad_plan_group_t& G = pl.g[g];
    CHECK(G.item0 == items && G.slice0 == slices && G.ws_base == floats);  // disjoint, in order, no gap
    if (in[g].tiles == 0 || in[g].ksteps == 0) {
      CHECK(G.splits == 0);
      continue;
    }
    CHECK(G.kps >= 4 && (G.kps & 1) == 0);
    CHECK(G.splits >= 1 && (long)G.splits * G.kps >= in[g].ksteps && (long)(G.splits - 1) * G.kps < in[g].ksteps);
    items += G.splits * in[g].tiles;
    slices += G.splits;
    floats += (uint64_t)G.splits * in[g].mn;
  }
  CHECK(items == pl.items && slices == pl.slices && floats == pl.ws_floats);
  // slices of different problems do not overlap in the workspace
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b) {
      const uint64_t a0 = pl.g[a].ws_base, a1 = a0 + (uint64_t)pl.g[a].splits * in[a].mn;
      const uint64_t b0 = pl.g[b].ws_base, b1 = b0 + (uint64_t)pl.g[b].splits * in[b].mn;
      CHECK(a1 <= b0 || b1 <= a0);
    }
  CHECK(pl.ws_floats <= WS_FLOATS);
}

static int run(int n, const wgrad_plan_in_t* in, int cus, wgrad_plan_t* pl, uint64_t ws = WS_FLOATS) {
  const int rc = wgrad_plan(n, in, cus, ws, pl);
  CHECK(rc == 0 || rc == 1);
  long tiles = 0;
  for (int g = 0; g < n; ++g)
    if (in[g].ksteps > 0) tiles += in[g].tiles;
  if (tiles > cus || tiles == 0) CHECK(rc == 1);  // refused: more tiles than the budget
  if (rc == 0) {
    check_plan(n, in, cus, *pl);
    ++n_plans;
    // ... and refused when the workspace is one float short of the plan
    wgrad_plan_t q;
    CHECK(pl->ws_floats >= 1 && wgrad_plan(n, in, cus, pl->ws_floats - 1, &q) == 1);
    CHECK(wgrad_plan(n, in, cus, pl->ws_floats, &q) == 0 && q.items == pl->items);
  } else {
    ++n_refused;
  }
  return rc;
}

static wgrad_plan_in_t prob(int tiles, int T) { return wgrad_plan_in_t{tiles, (T + 31) / 32, (uint64_t)tiles * 65536}; }

// The rule vlm_gemm_wgrad_grouped had before the planner existed, written out: `rows` token rows per group of ONE M x N shape
// with ntile tiles, one round of `cus` workgroups.  Returns false where it did not offer the launch.
static bool parent_rule(int n, const int* rows, int ntile, int cus, int* splits_out, int* kps_out) {
  long total_steps = 0;
  int live = 0;
  for (int g = 0; g < n; ++g)
    if (rows[g] > 0) { total_steps += (rows[g] + 31) / 32; ++live; }
  if (live == 0 || (long)live * ntile > cus) return false;
  long target = (total_steps * ntile + cus - 1) / cus;
  if (target < 16) target = 16;
  for (;; target += 2) {
    long items = 0;
    for (int g = 0; g < n; ++g)
      if (rows[g] > 0) items += (((rows[g] + 31) / 32 + target - 1) / target) * ntile;
    if (items <= cus) break;
  }
  for (int g = 0; g < n; ++g) {
    splits_out[g] = kps_out[g] = 0;
    if (rows[g] == 0) continue;
    const int nk = (rows[g] + 31) / 32;
    int splits = (int)((nk + target - 1) / target);
    int kps = (nk + splits - 1) / splits;
    kps += kps & 1;
    if (kps < 4) kps = 4;
    splits_out[g] = (nk + kps - 1) / kps;
    kps_out[g] = kps;
  }
  return true;
}

int main() {
  const int budgets[4] = {256, 248, 128, 64};
  wgrad_plan_t pl;

  // the base block (fc2 36, fc1 36, proj 9, qkv 27 tiles) at the two token counts of the flagship step
  for (int T : {54296, 13574}) {
    const wgrad_plan_in_t blk[4] = {prob(36, T), prob(36, T), prob(9, T), prob(27, T)};
    CHECK(run(4, blk, 256, &pl) == 0);
    CHECK(pl.items == 216 && pl.slices == 8);  // 108 tiles x 2 slices
    for (int g = 0; g < 4; ++g) CHECK(pl.g[g].splits == 2 && pl.g[g].kps == (T == 54296 ? 850 : 214));
    CHECK(pl.ws_floats == 216ull * 65536);
    CHECK(run(4, blk, 248, &pl) == 0 && pl.items == 216);
    CHECK(run(4, blk, 128, &pl) == 0 && pl.items == 108);  // one slice per tile is all the budget leaves
    CHECK(run(4, blk, 64, &pl) == 1);                      // 108 tiles on 64 CUs: not offered
    // fc2 + fc1 + proj alone: 81 tiles x 3 slices
    CHECK(run(3, blk, 256, &pl) == 0 && pl.items == 243 && pl.slices == 9);
  }

  // one to four problems of 1..36 tiles, T from 33 to 60 000 (multiples of 32 and not), every budget
  const int tile_sets[][4] = {{1, 0, 0, 0},   {36, 0, 0, 0},  {7, 0, 0, 0},   {1, 1, 0, 0},   {36, 1, 0, 0},  {3, 12, 0, 0},
                              {36, 36, 0, 0}, {1, 2, 3, 0},   {9, 27, 36, 0}, {36, 36, 36, 0}, {1, 1, 1, 1},   {36, 36, 9, 27},
                              {2, 3, 5, 7},   {36, 36, 36, 36}, {12, 4, 4, 1}, {35, 17, 1, 11}};
  const int Ts[] = {33, 64, 100, 511, 512, 513, 1000, 2048, 2077, 4099, 8191, 13574, 20000, 32768, 54296, 59999, 60000};
  for (const auto& ts : tile_sets)
    for (int T : Ts)
      for (int cus : budgets) {
        wgrad_plan_in_t in[4];
        int n = 0;
        while (n < 4 && ts[n] > 0) { in[n] = prob(ts[n], T); ++n; }
        run(n, in, cus, &pl);
      }
  // every tile count 1..36 for a single problem and for a pair, a coarse sweep of T
  for (int t = 1; t <= 36; ++t)
    for (int T = 33; T <= 60000; T += 1777)
      for (int cus : budgets) {
        const wgrad_plan_in_t one[1] = {prob(t, T)};
        CHECK(run(1, one, cus, &pl) == 0);  // 36 tiles fit every budget
        const wgrad_plan_in_t two[2] = {prob(t, T), prob(37 - t, T)};
        CHECK(run(2, two, cus, &pl) == 0);
      }
  // argument refusals
  {
    const wgrad_plan_in_t one[1] = {prob(4, 4096)};
    CHECK(wgrad_plan(0, one, 256, WS_FLOATS, &pl) == 1 && wgrad_plan(5, one, 256, WS_FLOATS, &pl) == 1);
    CHECK(wgrad_plan(1, one, 0, WS_FLOATS, &pl) == 1 && wgrad_plan(1, one, 256, 0, &pl) == 1);
    const wgrad_plan_in_t big[1] = {wgrad_plan_in_t{257, 128, 257ull * 65536}};
    CHECK(wgrad_plan(1, big, 256, ~0ull, &pl) == 1);
  }

  // the row-range form (vlm_gemm_wgrad_grouped): the shapes of tests/test_kernels_gpu.py::test_gemm_wgrad_grouped give the slice
  // counts the rule gave before it moved into the planner
  struct { int n; int rows[4]; int M, N; } grouped[] = {
      {2, {3520, 6000, 0, 0}, 768, 768}, {2, {880, 12694, 0, 0}, 2304, 768}, {2, {40, 577, 0, 0}, 256, 512},
      {2, {0, 900, 0, 0}, 768, 256},     {2, {900, 0, 0, 0}, 768, 256},      {4, {130, 70, 333, 64}, 256, 256}};
  for (const auto& c : grouped)
    for (int cus : budgets) {
      const int ntile = ((c.M + 255) / 256) * (c.N / 256);
      int want_splits[4], want_kps[4];
      const bool offered = parent_rule(c.n, c.rows, ntile, cus, want_splits, want_kps);
      wgrad_plan_in_t in[4];
      int live = 0, idx[4];
      for (int g = 0; g < c.n; ++g)  // the entry point passes the groups that have rows
        if (c.rows[g] > 0) { idx[live] = g; in[live++] = wgrad_plan_in_t{ntile, (c.rows[g] + 31) / 32, (uint64_t)c.M * c.N}; }
      const int rc = run(live, in, cus, &pl);
      CHECK((rc == 0) == offered);
      if (rc) continue;
      int slice0 = 0;
      for (int i = 0; i < live; ++i) {
        CHECK(pl.g[i].splits == want_splits[idx[i]] && pl.g[i].kps == want_kps[idx[i]]);
        CHECK(pl.g[i].slice0 == slice0 && pl.g[i].ws_base == (uint64_t)slice0 * c.M * c.N);  // the [slice][M][N] layout it had
        slice0 += pl.g[i].splits;
      }
    }
  CHECK(n_plans > 1000 && n_refused > 50);
  printf("wgrad plan ok: %ld plans, %ld refusals\n", n_plans, n_refused);
  return 0;
}
