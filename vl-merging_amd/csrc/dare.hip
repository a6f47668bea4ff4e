// DARE merge (drop and rescale; Yu et al. 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no DARE.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/dare_restatement.py; the kernel is held to that restatement bit for bit.
//
// The mask is never stored: the draw of (seed, stream, source, element) is one word of a Philox4x32-10 block (philox.h), and
// one block serves one float4 of one source.  So the pass is the task-vector merge's traffic, 4 (S + 1) B read and 4 B written
// per element, plus ten Philox rounds per float4 and source on the VALU.
//   vlm_dare_clear_kernel   a tiny launch: the counters of every job start the run at zero.
//   vlm_dare_apply_kernel   one launch over the plan's 16-KiB chunk table (chunk_plan.h), the shape of vlm_ties_apply_kernel:
//                           a workgroup owns a CONTIGUOUS run of chunks, 16-B non-temporal loads and stores, steps 1-5 of the
//                           rule, and the per-job counters flushed (64-bit integer atomics) when the run leaves a job.
// Steps 4-5 (both modes) are chunk_walk.h's combine rule, shared with ties.hip, band.hip and della.hip.  Integer counters
// only, so nothing depends on the order workgroups run in.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
// This file holds the rule (dare_elem, the draws) and its own per-job check; the walker, the run loop and the workspace's view
// are chunk_walk.h's, the counter plan (layout, upload, the two-launch run) and the family's host checks chunk_plan.h's.
#include "vlm_common.h"
#include "philox.h"
#include "chunk_walk.h"  // the chunk walker, the run loop, the combine rule and the counters: the whole family's

#define DARE_THREADS CHUNK_THREADS
#define DARE_APPLY_BLOCKS_PER_CU 12   // vlm_ties_apply_kernel's rule; not A/B-measured against other values (docs/experiments.md, "DARE merge")

static_assert(VLM_DARE_COUNTERS == VLM_TIES_COUNTERS, "dare.hip counts into chunk_walk.h's ties_counts_t");

typedef counts_view_t<vlm_dare_header_t, vlm_dare_job_t> dare_view_t;

// what a job's scalars come to, workgroup-uniform
struct dare_param_t {
  uint64_t seed;       // the Philox key
  uint32_t stream;
  uint32_t below;      // keep_below's low word
  bool keep_all;       // keep_below == 2^32
  float rescale, lam;
};

// steps 1 and 3-5 for one element whose draws are u[0 .. NSRC)
template <int NSRC, int MODE>
__device__ __forceinline__ float dare_elem(float c, const float* wv, const uint32_t* u, const dare_param_t& p, ties_counts_t& n) {
  float tt[NSRC];
  int any = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float t = __fsub_rn(wv[m], c);                                 // step 1
    const bool kept = p.keep_all || u[m] < p.below;                      // step 3: (uint64) u < keep_below
    tt[m] = kept ? __fmul_rn(t, p.rescale) : 0.0f;
    n.c[m] += kept ? 1u : 0u;
    any += kept ? 1 : 0;
  }
  return combine<NSRC, MODE>(c, tt, any, p.lam, n.c[TIES_CONFLICT], n.c[TIES_EMPTY]);  // steps 4-5 (chunk_walk.h)
}

// The rule as chunk_stream's rule (chunk_walk.h).  Step 2: prep draws one Philox block per source for float4 idx4, and element c
// of that float4 takes word c -- so the ragged tail's element 4 n4 + t takes word t of the block of float4 n4.
template <int NSRC, int MODE>
struct dare_rule {
  struct draw_t {
    philox4_t r[NSRC];
  };
  const dare_param_t& p;
  ties_counts_t& n;
  __device__ __forceinline__ draw_t prep(uint64_t idx4) const {
    draw_t d;
#pragma unroll
    for (int m = 0; m < NSRC; ++m) d.r[m] = dare_draw4(p.seed, p.stream, (uint32_t)m, (uint32_t)idx4);
    return d;
  }
  __device__ __forceinline__ float elem(const draw_t& d, int c, float base, const float* wv) const {
    uint32_t uu[NSRC];
#pragma unroll
    for (int m = 0; m < NSRC; ++m) uu[m] = philox_word(d.r[m], (uint32_t)c);
    return dare_elem<NSRC, MODE>(base, wv, uu, p, n);
  }
};

__global__ __launch_bounds__(DARE_THREADS) void vlm_dare_clear_kernel(unsigned char* __restrict__ ws) {
  const dare_view_t w = counts_view<vlm_dare_header_t, vlm_dare_job_t>(ws);
  chunk_clear_counts(w.counters, w.hdr->n_jobs * VLM_DARE_COUNTERS);
}

__global__ __launch_bounds__(DARE_THREADS) void vlm_dare_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(DARE_THREADS / 64) * VLM_DARE_COUNTERS];
  const dare_view_t w = counts_view<vlm_dare_header_t, vlm_dare_job_t>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_DARE_COUNTERS; ++k) n.c[k] = 0;
  dare_param_t p = {0, 0, 0, false, 1.0f, 0.0f};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_dare_job_t& jn = w.jobs[cur];
        p.seed = jn.seed;
        p.stream = jn.stream;
        p.below = (uint32_t)jn.keep_below;
        p.keep_all = (jn.keep_below >> 32) != 0;
        p.rescale = jn.rescale;
        p.lam = jn.lam;
      },
      [&](const vlm_dare_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          if (j.mode == VLM_DARE_TIES) {
            dare_rule<S(), VLM_DARE_TIES> rule{p, n};
            chunk_stream<S(), true, true>(j, start4, rule);
          } else {
            dare_rule<S(), VLM_DARE_LINEAR> rule{p, n};
            chunk_stream<S(), true, true>(j, start4, rule);
          }
        });
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_DARE_COUNTERS); });
}

extern "C" size_t vlm_dare_plan_bytes(int n_jobs, uint64_t total_elems) {
  return counts_plan_bytes<vlm_dare_header_t, vlm_dare_job_t>(n_jobs, total_elems, VLM_DARE_COUNTERS);
}

extern "C" int vlm_dare_plan_upload(const vlm_dare_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return counts_plan_upload<vlm_dare_header_t, VLM_DARE_COUNTERS>(jobs, n_jobs, workspace, workspace_bytes, stream, [](const vlm_dare_job_t& j) {
    if (j.mode != VLM_DARE_LINEAR && j.mode != VLM_DARE_TIES) return VLM_ERR_ARG;
    if (j.keep_below < 1 || j.keep_below > (1ull << 32)) return VLM_ERR_ARG;
    return chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);
  });
}

extern "C" int vlm_dare_run(void* workspace, void* stream) {
  return counts_run(workspace, stream, vlm_dare_clear_kernel, vlm_dare_apply_kernel, chunk_grid(DARE_APPLY_BLOCKS_PER_CU));
}
