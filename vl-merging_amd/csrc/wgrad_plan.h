// The slice plan of a grouped weight-gradient launch (gemm.hip: vlm_gemm_wgrad_batch, vlm_gemm_wgrad_grouped), host side only.
// A group is one reduction over token rows into one M x N weight gradient, cut into 256x256 output tiles and, along the
// reduction, into 32-row K steps.  A launch deals (slice, tile) items to workgroups: group g owns items
// [item0, item0 + splits * tiles), slice-major with the tile fastest, and slice s of it covers K steps [s * kps, (s + 1) * kps)
// of the group's own reduction.  Every slice stores its fp32 tiles into the workspace at ws_base + s * M * N floats, and the
// reduce launch adds a group's slices into its gradient.
// The rule: the smallest step target, counted up in twos from the launch's mean (at least 16 steps per slice), for which all
// items fit the CU budget in ONE round; a group's slices are then evened out, kps even (the kernel's K loop is unrolled by
// two) and >= 4 (its pipeline depth).
// Compiles without HIP (tests/helpers/wgrad_plan_check.cpp does so).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define WGRAD_PLAN_MAX_GROUPS 4
#define WGRAD_PLAN_MIN_STEPS 16  // K steps per slice below which a slice is mostly prologue and epilogue

struct wgrad_plan_in_t {
  int tiles;         // 256x256 output tiles of the group (0: the group is empty and takes no part)
  int ksteps;        // 32-row K steps of its reduction, the ragged last one included
  uint64_t mn;       // floats of one slice: M * N
};

struct wgrad_plan_group_t {
  int kps, splits;   // K steps per slice (even, >= 4), slices (splits * kps >= ksteps > (splits - 1) * kps)
  int item0;         // first item of the group in the launch's grid
  int slice0;        // slices of the groups before it
  uint64_t ws_base;  // floats before the group's first slice in the workspace
};

struct wgrad_plan_t {
  wgrad_plan_group_t g[WGRAD_PLAN_MAX_GROUPS];
  int items;           // workgroups of the launch, <= cus
  int slices;          // all groups' slices
  uint64_t ws_floats;  // sum of splits * mn
};

// 0: planned.  1: not offered -- no live group, more tiles than `cus` workgroups, or a workspace smaller than the plan's slices.
static inline int wgrad_plan(int n, const wgrad_plan_in_t* in, int cus, uint64_t ws_floats, wgrad_plan_t* out) {
  if (n < 1 || n > WGRAD_PLAN_MAX_GROUPS || cus < 1) return 1;
  long tiles = 0, work = 0;
  for (int g = 0; g < n; ++g) {
    if (in[g].tiles < 0 || in[g].ksteps < 0) return 1;
    if (in[g].tiles == 0 || in[g].ksteps == 0) continue;
    tiles += in[g].tiles;
    work += (long)in[g].ksteps * in[g].tiles;
  }
  if (tiles == 0 || tiles > cus) return 1;  // more tiles than one round holds: the plain path's own split rules apply
  long target = (work + cus - 1) / cus;
  if (target < WGRAD_PLAN_MIN_STEPS) target = WGRAD_PLAN_MIN_STEPS;
  for (;; target += 2) {  // ends: with one slice per group the items are the tiles
    long items = 0;
    for (int g = 0; g < n; ++g)
      if (in[g].tiles > 0 && in[g].ksteps > 0) items += ((in[g].ksteps + target - 1) / target) * in[g].tiles;
    if (items <= cus) break;
  }
  out->items = out->slices = 0;
  out->ws_floats = 0;
  for (int g = 0; g < n; ++g) {
    wgrad_plan_group_t& G = out->g[g];
    G = wgrad_plan_group_t{0, 0, out->items, out->slices, out->ws_floats};
    if (in[g].tiles == 0 || in[g].ksteps == 0) continue;
    const int nk = in[g].ksteps;
    int splits = (int)((nk + target - 1) / target);
    int kps = (nk + splits - 1) / splits;
    kps += kps & 1;
    if (kps < 4) kps = 4;
    splits = (nk + kps - 1) / kps;
    G.kps = kps;
    G.splits = splits;
    out->items += splits * in[g].tiles;
    out->slices += splits;
    out->ws_floats += (uint64_t)splits * in[g].mn;
  }
  return out->ws_floats > ws_floats ? 1 : 0;
}
