// What ties.hip and dare.hip share per element and per workgroup: steps 3-5 of the TIES rule (include/vlm_hip.h) on entries
// tt_m that a kernel has already trimmed (TIES: by magnitude, DARE: by its Philox mask), the per-thread counters, their
// flush (integer atomics only), and the contiguous run of chunks a workgroup owns.  Device code only.
#pragma once
#include "vlm_common.h"
#include "chunk_plan.h"

typedef unsigned long long u64_t;

struct ties_counts_t {
  uint32_t c[VLM_TIES_COUNTERS];  // kept[0..3], conflict, empty
};

// Steps 3-5 on tt[0 .. NSRC): elect the sign by comparison of the sum, mean of the agreeing entries, dst = c + lam * d.
// Counts `conflict` (a positive and a negative entry among tt) and `empty` (nothing agrees).
template <int NSRC>
__device__ __forceinline__ float ties_elect(float c, const float* tt, float lam, ties_counts_t& n) {
  float s = 0.0f;
  bool has_pos = false, has_neg = false;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    s = __fadd_rn(s, tt[m]);                                             // step 3
    has_pos |= tt[m] > 0.0f;
    has_neg |= tt[m] < 0.0f;
  }
  float num = 0.0f;
  int cnt = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {                                       // step 4
    const bool agree = (s > 0.0f && tt[m] > 0.0f) || (s < 0.0f && tt[m] < 0.0f);
    if (agree) {
      num = __fadd_rn(num, tt[m]);
      ++cnt;
    }
  }
  const float d = cnt > 0 ? __fdiv_rn(num, (float)cnt) : 0.0f;
  n.c[VLM_MERGE_MAX_SRC] += (has_pos && has_neg) ? 1u : 0u;
  n.c[VLM_MERGE_MAX_SRC + 1] += cnt == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(lam, d));                                // step 5
}

// the contiguous run of chunks this workgroup owns
__device__ __forceinline__ void ties_my_chunks(uint64_t n_chunks, uint64_t* c0, uint64_t* c1) {
  const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
  *c0 = (uint64_t)blockIdx.x * per;
  uint64_t e = *c0 + per;
  *c1 = e < n_chunks ? e : n_chunks;
}

// in-workgroup reduction of the six counters, then one 64-bit atomic per counter; `red` holds (CHUNK_THREADS / 64) x
// VLM_TIES_COUNTERS entries of LDS
__device__ __forceinline__ void ties_flush_counts(ties_counts_t& n, u64_t* red, u64_t* counters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < VLM_TIES_COUNTERS; ++k) {
    uint32_t v = n.c[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave * VLM_TIES_COUNTERS + k] = v;
    n.c[k] = 0;
  }
  __syncthreads();
  if (threadIdx.x < VLM_TIES_COUNTERS) {
    u64_t t = 0;
    for (int wv = 0; wv < CHUNK_THREADS / 64; ++wv) t += red[wv * VLM_TIES_COUNTERS + threadIdx.x];
    if (t) __hip_atomic_fetch_add(&counters[threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
}
