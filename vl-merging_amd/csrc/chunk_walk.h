// The device skeleton of the merge family (merge.hip, ties.hip, dare.hip, pairstats.hip, band.hip, della.hip), stated once; a
// method's file holds only its rule.
//   with_nsrc      the one dispatch over a job's source count, 1 .. VLM_MERGE_MAX_SRC
//   chunk_stream   the streaming body of one 16-KiB chunk (chunk_plan.h): loads, the rule per element, store, ragged tail
//   chunk_run      the contiguous run of chunks a workgroup owns, with "entering job" / "leaving job" callbacks
// and what ties.hip, dare.hip, band.hip and della.hip share per element and per workgroup: the combine rule (LINEAR: the sum;
// TIES: steps 3-5 of the TIES rule, include/vlm_hip.h) on entries tt_m that a kernel has already trimmed (TIES, band: by
// magnitude; DARE, DELLA: by their Philox masks), the per-thread counters, their flush (integer atomics only) and their clear,
// and the view of a counter plan's workspace (dare.hip, tall.hip).  What the reducers share is chunk_records.h.
// Device code only.
#pragma once
#include "vlm_common.h"
#include "chunk_plan.h"
#include <type_traits>

typedef unsigned long long u64_t;

// A run flushes at the latest after 2^19 chunks of one job.  2^19 chunks x 4096 keys < 2^32: the 32-bit LDS bins of a histogram
// pass cannot wrap between flushes; a thread counts at most 16 per chunk: 2^23 per thread, 2^29 in the 64-lane wave sum of
// chunk_flush_counts (32-bit).
#define CHUNK_FLUSH_CHUNKS (1u << 19)

// f(std::integral_constant<int, n_src>): the job's source count as a compile-time constant
template <class F>
__device__ __forceinline__ void with_nsrc(int n_src, F&& f) {
  switch (n_src) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

struct chunk_no_prep {  // what a rule's prep() returns when a float4 needs no preparation
};

// The chunk at start4 of job j (fields dst, base, src, n_elem): 4 float4 per thread, strided by the block so every wave
// instruction is 1 KiB contiguous; non-temporal 16-B loads and stores (the streams are touched once; docs/experiments.md,
// "Merge kernel: grid and cache policy").  Every load of the thread's 4 float4, of all NSRC sources and (BASE) of the base, is
// issued before the first use.  Then per float4 `rule.prep(idx4)` (DARE: the Philox blocks of float4 idx4, computed while the
// loads are in flight) and per element `rule.elem(state, c, base, w)` with c the element's place in its float4 and w its NSRC
// source values; STORE: what elem returns is the output.  The ragged tail (thread t < chunk_tail_len: element 4 n4 + t) goes
// through the same rule, with the state of float4 n4 and c = t.
// No __restrict__: DARE's dst may be its base or a source exactly.  Every load of a float4 precedes its store in program
// order.  Without BASE no load from j.base is formed (LERP and MEAN jobs may have base == NULL) and elem sees base = 0.
template <int NSRC, bool BASE, bool STORE, class Job, class Rule>
__device__ __forceinline__ void chunk_stream(const Job& j, uint64_t start4, Rule& rule) {
  const uint64_t n4 = j.n_elem >> 2;
  f32x4* dst = nullptr;  // a job type without a dst field (pair statistics) streams with STORE = false
  if constexpr (STORE) dst = reinterpret_cast<f32x4*>(j.dst);
  const f32x4* base = BASE ? reinterpret_cast<const f32x4*>(j.base) : nullptr;
  const f32x4* s[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) s[m] = reinterpret_cast<const f32x4*>(j.src[m]);
  f32x4 v[4][NSRC];
  f32x4 b[4];
  uint64_t idx[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    idx[u] = start4 + threadIdx.x + u * CHUNK_THREADS;
    if (idx[u] < n4) {
#pragma unroll
      for (int m = 0; m < NSRC; ++m) v[u][m] = __builtin_nontemporal_load(&s[m][idx[u]]);
      if (BASE) b[u] = __builtin_nontemporal_load(&base[idx[u]]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (idx[u] < n4) {
      const auto st = rule.prep(idx[u]);
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float w[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) w[m] = v[u][m][c];
        o[c] = rule.elem(st, c, BASE ? b[u][c] : 0.0f, w);
      }
      if (STORE) __builtin_nontemporal_store(o, &dst[idx[u]]);
    }
  }
  if (threadIdx.x < chunk_tail_len(start4, j.n_elem)) {
    const uint64_t i = (n4 << 2) + threadIdx.x;
    float w[NSRC];
#pragma unroll
    for (int m = 0; m < NSRC; ++m) w[m] = reinterpret_cast<const float*>(j.src[m])[i];
    const float bt = BASE ? reinterpret_cast<const float*>(j.base)[i] : 0.0f;
    const float o = rule.elem(rule.prep(n4), (int)threadIdx.x, bt, w);
    if constexpr (STORE) reinterpret_cast<float*>(j.dst)[i] = o;
  }
}

// The contiguous run of chunks this workgroup owns: false when it owns none.
__device__ __forceinline__ bool chunk_my_run(uint64_t n_chunks, uint64_t* c0, uint64_t* c1) {
  const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
  *c0 = (uint64_t)blockIdx.x * per;
  const uint64_t e = *c0 + per;
  *c1 = e < n_chunks ? e : n_chunks;
  return *c0 < *c1;
}

// Walks the non-empty run [c0, c1): enter(job index) loads the job's scalars, body(job, start4) streams one chunk, leave(job
// index) flushes what the run gathered for the job -- when the run leaves the job, after CHUNK_FLUSH_CHUNKS chunks inside one
// job (then the same job is entered again), and at the end of the run.  body gets a COPY of the job: its fields are loaded in
// one batch before body dispatches on them, not field by field behind the dispatch and again behind every store (the
// workspace is written by the kernels that walk it, so the compiler may not keep a job's fields across a store).
template <class Job, class Enter, class Body, class Leave>
__device__ __forceinline__ void chunk_run(const chunk_t* chunks, const Job* jobs, uint64_t c0, uint64_t c1, Enter&& enter,
                                          Body&& body, Leave&& leave) {
  uint32_t cur = 0xffffffffu, since = 0;
  for (uint64_t c = c0; c < c1; ++c) {
    const chunk_t ck = chunks[c];  // block-uniform => scalar loads
    if (ck.job != cur || since >= CHUNK_FLUSH_CHUNKS) {
      if (cur != 0xffffffffu) leave(cur);
      cur = ck.job;
      since = 0;
      enter(cur);
    }
    ++since;
    const Job j = jobs[cur];
    body(j, (uint64_t)ck.start4);
  }
  leave(cur);
}

struct ties_counts_t {
  uint32_t c[VLM_TIES_COUNTERS];  // kept[0..3], conflict, empty: what TIES, DARE and DELLA count per job
};
#define TIES_CONFLICT VLM_MERGE_MAX_SRC
#define TIES_EMPTY (VLM_MERGE_MAX_SRC + 1)

// How the trimmed entries tt[0 .. NSRC) of an element become its output, for every method that trims or drops (ties.hip, dare.hip,
// band.hip, della.hip).  Both rules bump the two counters they are handed: `conflict` (a positive and a negative entry among tt)
// and `empty` (nothing contributes).
#define COMBINE_LINEAR 0
#define COMBINE_TIES 1
static_assert(VLM_DARE_LINEAR == COMBINE_LINEAR && VLM_BAND_LINEAR == COMBINE_LINEAR && VLM_DELLA_LINEAR == COMBINE_LINEAR &&
                  VLM_DARE_TIES == COMBINE_TIES && VLM_BAND_TIES == COMBINE_TIES && VLM_DELLA_TIES == COMBINE_TIES,
              "one MODE serves the three methods' mode fields");

// Steps 3-5 of the TIES rule: elect the sign by comparison of the sum, mean of the agreeing entries, dst = c + lam * d; `empty`:
// nothing agrees.
template <int NSRC>
__device__ __forceinline__ float ties_elect(float c, const float* tt, float lam, uint32_t& conflict, uint32_t& empty) {
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
  conflict += (has_pos && has_neg) ? 1u : 0u;
  empty += cnt == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(lam, d));                                // step 5
}

// COMBINE_TIES: ties_elect.  COMBINE_LINEAR: d = ((0 + tt_0) + tt_1) + ..., dst = c + lam * d; `empty`: no entry was kept
// (`any` counts the kept ones -- a kept entry may be zero).
template <int NSRC, int MODE>
__device__ __forceinline__ float combine(float c, const float* tt, int any, float lam, uint32_t& conflict, uint32_t& empty) {
  if (MODE == COMBINE_TIES) return ties_elect<NSRC>(c, tt, lam, conflict, empty);
  float d = 0.0f;
  bool has_pos = false, has_neg = false;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    d = __fadd_rn(d, tt[m]);
    has_pos |= tt[m] > 0.0f;
    has_neg |= tt[m] < 0.0f;
  }
  conflict += (has_pos && has_neg) ? 1u : 0u;
  empty += any == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(lam, d));
}

// A counter plan's workspace (chunk_plan.h: counts_layout) as the kernels of dare.hip and tall.hip see it.
template <class Hdr, class Job>
struct counts_view_t {
  const Hdr* hdr;
  const Job* jobs;
  const chunk_t* chunks;
  u64_t* counters;
};

template <class Hdr, class Job>
__device__ __forceinline__ counts_view_t<Hdr, Job> counts_view(unsigned char* ws) {
  counts_view_t<Hdr, Job> v;
  v.hdr = reinterpret_cast<const Hdr*>(ws);
  v.jobs = reinterpret_cast<const Job*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

// the body of DARE's, TALL's and DELLA's clear launch: the counters of every job start the run at zero
__device__ __forceinline__ void chunk_clear_counts(u64_t* counters, uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * CHUNK_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * CHUNK_THREADS)
    counters[i] = 0;
}

// in-workgroup reduction of a method's N counters (TIES and DARE: six, the band merge: ten), then one 64-bit atomic per
// counter; `red` holds (CHUNK_THREADS / 64) x N entries of LDS
template <int N>
__device__ __forceinline__ void chunk_flush_counts(uint32_t (&c)[N], u64_t* red, u64_t* counters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    uint32_t v = c[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave * N + k] = v;
    c[k] = 0;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    u64_t t = 0;
    for (int wv = 0; wv < CHUNK_THREADS / 64; ++wv) t += red[wv * N + threadIdx.x];
    if (t) __hip_atomic_fetch_add(&counters[threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
}
