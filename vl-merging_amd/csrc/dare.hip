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
// This file holds the rule (dare_elem, the draws) and the workspace layout; the walker, the run loop and the host checks are
// chunk_walk.h's and chunk_plan.h's, as in ties.hip.
#include "vlm_common.h"
#include "philox.h"
#include "chunk_walk.h"  // the chunk walker, the run loop, the combine rule and the counters: the whole family's

#define DARE_THREADS CHUNK_THREADS
#define DARE_APPLY_BLOCKS_PER_CU 12   // vlm_ties_apply_kernel's rule; not A/B-measured against other values (docs/experiments.md, "DARE merge")

static_assert(VLM_DARE_COUNTERS == VLM_TIES_COUNTERS, "dare.hip counts into chunk_walk.h's ties_counts_t");

struct dare_view_t {
  const vlm_dare_header_t* hdr;
  const vlm_dare_job_t* jobs;
  const chunk_t* chunks;
  u64_t* counters;
};

__device__ __forceinline__ dare_view_t dare_view(unsigned char* ws) {
  dare_view_t v;
  v.hdr = reinterpret_cast<const vlm_dare_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_dare_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

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
  const dare_view_t w = dare_view(ws);
  chunk_clear_counts(w.counters, w.hdr->n_jobs * VLM_DARE_COUNTERS);
}

__global__ __launch_bounds__(DARE_THREADS) void vlm_dare_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(DARE_THREADS / 64) * VLM_DARE_COUNTERS];
  const dare_view_t w = dare_view(ws);
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

// fills every offset of `h` for n_jobs jobs and n_chunks chunks; returns the total size
static size_t dare_layout(vlm_dare_header_t* h, uint64_t n_jobs, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(vlm_dare_header_t));
  h->n_jobs = n_jobs;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(vlm_dare_job_t));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  h->counters_off = at.take(n_jobs * VLM_DARE_COUNTERS * sizeof(uint64_t));
  return at.off;
}

extern "C" size_t vlm_dare_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  vlm_dare_header_t h;
  return dare_layout(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems));
}

extern "C" int vlm_dare_plan_upload(const vlm_dare_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_chunks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_dare_job_t& j = jobs[i];
    if (j.n_elem == 0 || (j.mode != VLM_DARE_LINEAR && j.mode != VLM_DARE_TIES)) return VLM_ERR_ARG;
    if (j.keep_below < 1 || j.keep_below > (1ull << 32)) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);
    if (rc != VLM_OK) return rc;
    n_chunks += chunks_of(j.n_elem);
  }
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  vlm_dare_header_t hdr;
  const size_t total = dare_layout(&hdr, (uint64_t)n_jobs, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the counters begin: they are device-made (every run zeroes them first)
  return chunk_upload(workspace, chunk_image(hdr, jobs, n_jobs, hdr.counters_off), 0, (hipStream_t)stream);
}

extern "C" int vlm_dare_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // two launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL(vlm_dare_clear_kernel, dim3(64), dim3(DARE_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_dare_apply_kernel, chunk_grid(DARE_APPLY_BLOCKS_PER_CU), dim3(DARE_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
