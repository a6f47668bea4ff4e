// The Gram rule that Model Stock (stock.hip) and the spherical merge (sphere.hip) reduce with: per job of S sources the sums
// sq[S] and dot[S (S - 1) / 2] of the task vectors, step 2 of the Model Stock rule (include/vlm_hip.h).  This file holds what a
// thread adds per element and what a chunk leaves per wave; the pinned order behind that -- the wave fold, the record per chunk,
// the run of chunks, the fold of a job's records -- is chunk_records.h's.  Generic over the job type (fields base, src, n_src,
// n_elem) and over whether the job has a base: without one, chunk_stream hands elem() c = +0.0 and W - (+0.0) is W, bit for bit.
// Device code only.  -ffp-contract=off and the __d*_rn forms: one rounding per operation, no FMA.
#pragma once
#include "vlm_common.h"
#include "chunk_walk.h"
#include "chunk_records.h"

#define STOCK_THREADS CHUNK_THREADS
#define STOCK_PAIRS VLM_PAIRSTATS_PAIRS
#define STOCK_SUMS VLM_STOCK_SUMS      // a record: sq[4], then dot[6]
#define STOCK_FOLD_THREADS 64          // lanes 0 .. 9 add one sum each; lane 0 then does step 3

static_assert(STOCK_PAIRS == VLM_MERGE_MAX_SRC * (VLM_MERGE_MAX_SRC - 1) / 2, "one slot per pair");
static_assert(STOCK_SUMS == 10, "a record is four squared norms and six dot products");

// A thread's sums over one chunk, for a job of S sources: NP = S (S - 1) / 2 pairs, pair (a, b) at b (b - 1) / 2 + a < NP.
template <int S>
struct stock_acc_t {
  static constexpr int NP = S * (S - 1) / 2;
  static constexpr int NPA = NP > 0 ? NP : 1;
  double sq[S], dot[NPA];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < S; ++m) sq[m] = 0.0;
#pragma unroll
    for (int p = 0; p < NPA; ++p) dot[p] = 0.0;
  }
};

// Steps 1-2 as chunk_stream's rule: elem() adds one element to the thread's sums and returns nothing worth storing.
template <int S>
struct stock_reduce_rule {
  stock_acc_t<S>& n;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    double xd[S];
#pragma unroll
    for (int m = 0; m < S; ++m) {
      xd[m] = (double)__fsub_rn(wv[m], c);                                         // step 1
      n.sq[m] = __dadd_rn(n.sq[m], __dmul_rn(xd[m], xd[m]));                       // step 2
    }
#pragma unroll
    for (int b = 1; b < S; ++b) {
#pragma unroll
      for (int a = 0; a < b; ++a) {
        const int p = b * (b - 1) / 2 + a;
        n.dot[p] = __dadd_rn(n.dot[p], __dmul_rn(xd[a], xd[b]));
      }
    }
    return 0.0f;
  }
};

// does a job of S sources have the sum at `slot` (0 .. STOCK_SUMS)?
__device__ __forceinline__ bool stock_slot_used(int slot, int S) {
  return slot < VLM_MERGE_MAX_SRC ? slot < S : slot - VLM_MERGE_MAX_SRC < S * (S - 1) / 2;
}

// one chunk's sums, then their wave sums into red[wave][slot] (lane 0 writes; the slots are a record's order)
template <int S, bool BASE = true, class Job>
__device__ __forceinline__ void stock_chunk(const Job& j, uint64_t start4, double* red) {
  stock_acc_t<S> n;
  n.clear();
  stock_reduce_rule<S> rule{n};
  chunk_stream<S, BASE, false>(j, start4, rule);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* r = red + wave * STOCK_SUMS;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const double v = chunk_wave_sum(n.sq[m]);
    if (lane == 0) r[m] = v;
  }
#pragma unroll
  for (int p = 0; p < stock_acc_t<S>::NP; ++p) {
    const double v = chunk_wave_sum(n.dot[p]);
    if (lane == 0) r[VLM_MERGE_MAX_SRC + p] = v;
  }
}
