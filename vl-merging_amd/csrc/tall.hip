// Consensus merge with TALL masks (Wang et al., ICML 2024) over every output tensor of an all_moe -> ufo merge, and the reverse
// select that rebuilds one expert from the unified tensor, the central tensor and a packed mask.
// No reference site: the reference repository has neither.  The rule is written down in include/vlm_hip.h and restated in numpy
// by tests/tall_restatement.py; the kernel is held to that restatement bit for bit, mask words and padding bits included.
//
// The pass is the task-vector merge's traffic, 4 (S + 1) B read and 4 B written per element, plus S / 8 B of mask per element
// where a job asks for masks (RESTORE: 8 B + 1 / 8 B read, 4 B written).
//   vlm_tall_clear_kernel   a tiny launch: the counters of every job start the run at zero.
//   vlm_tall_apply_kernel   one launch over the plan's 16-KiB chunk table (chunk_plan.h), the shape of vlm_dare_apply_kernel: a
//                           workgroup owns a CONTIGUOUS run of chunks, 16-B non-temporal loads and stores (mask words: plain
//                           4-B stores, one per eight lanes), and the per-job
//                           counters flushed (64-bit integer atomics) when the run leaves a job.  Both ops, one kernel.
// The chunk body is not chunk_stream but mask_chunk (mask_chunk.h, shared with emr.hip; the slot every thread enters, the one
// lane that owns the ragged tail and the plain word store are explained there): this file gives it the rule per element, steps
// 1-5 and the restore select, and the counters.
// Integer counters only, so nothing depends on the order workgroups run in.  -ffp-contract=off and __f*_rn: one rounding per
// operation, no FMA.  The run loop and the workspace's view are chunk_walk.h's, the counter plan (layout, upload, the two-launch
// run) and the family's host checks chunk_plan.h's, as in dare.hip.
#include "vlm_common.h"
#include "chunk_walk.h"  // the run loop, the source-count dispatch and the counters: the whole family's
#include "mask_chunk.h"  // the chunk body of the methods with packed masks
#include "tall_mask.h"   // where an element's bit lives; the checks on a job's masks

#define TALL_THREADS CHUNK_THREADS
#define TALL_APPLY_BLOCKS_PER_CU 12   // vlm_dare_apply_kernel's rule; not A/B-measured against other values (docs/experiments.md, "Consensus merge")

static_assert(VLM_TALL_COUNTERS == VLM_TIES_COUNTERS, "tall.hip counts into chunk_walk.h's ties_counts_t");
#define TALL_SELECTED TIES_CONFLICT   // the slot behind kept[]: the elements with sel

typedef counts_view_t<vlm_tall_header_t, vlm_tall_job_t> tall_view_t;

// a job's scalars, workgroup-uniform
struct tall_param_t {
  int k;
  float tall_lambda, lam;
};

// Steps 1-5 for one element; bit m of `keep` = keep_m.
template <int NSRC>
__device__ __forceinline__ float tall_elem(float c, const float* wv, const tall_param_t& p, ties_counts_t& n, uint32_t& keep) {
  float x[NSRC];
  float d = 0.0f;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    x[m] = __fsub_rn(wv[m], c);                                          // step 1
    d = __fadd_rn(d, x[m]);                                              // step 2
  }
  int votes = 0;
  keep = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float r = __fsub_rn(d, x[m]);                                  // step 3
    const bool kept = fabsf(x[m]) >= __fmul_rn(p.tall_lambda, fabsf(r));
    keep |= (kept ? 1u : 0u) << m;
    n.c[m] += kept ? 1u : 0u;
    votes += kept ? 1 : 0;
  }
  const bool sel = votes >= p.k;                                         // step 4
  n.c[TALL_SELECTED] += sel ? 1u : 0u;
  n.c[TIES_EMPTY] += votes == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(p.lam, sel ? d : 0.0f));                 // step 5
}

// the restore rule for one element
__device__ __forceinline__ float tall_pick(bool bit, float u, float c, ties_counts_t& n) {
  n.c[0] += bit ? 1u : 0u;
  return bit ? u : c;
}

// what mask_chunk asks of a method: a job's scalars and the thread's counters, by reference
template <int NSRC>
struct tall_rule_t {
  const tall_param_t& p;
  ties_counts_t& n;
  __device__ __forceinline__ float elem(float c, const float* w, uint32_t& bits) { return tall_elem<NSRC>(c, w, p, n, bits); }
  __device__ __forceinline__ float pick(bool bit, float u, float c) { return tall_pick(bit, u, c, n); }
};

__global__ __launch_bounds__(TALL_THREADS) void vlm_tall_clear_kernel(unsigned char* __restrict__ ws) {
  const tall_view_t w = counts_view<vlm_tall_header_t, vlm_tall_job_t>(ws);
  chunk_clear_counts(w.counters, w.hdr->n_jobs * VLM_TALL_COUNTERS);
}

__global__ __launch_bounds__(TALL_THREADS) void vlm_tall_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(TALL_THREADS / 64) * VLM_TALL_COUNTERS];
  const tall_view_t w = counts_view<vlm_tall_header_t, vlm_tall_job_t>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_TALL_COUNTERS; ++k) n.c[k] = 0;
  tall_param_t p = {0, 0.0f, 0.0f};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_tall_job_t& jn = w.jobs[cur];
        p.k = jn.k;
        p.tall_lambda = jn.tall_lambda;
        p.lam = jn.lam;
      },
      [&](const vlm_tall_job_t& j, uint64_t start4) {
        if (j.op == VLM_TALL_RESTORE) {
          tall_rule_t<1> rule = {p, n};
          mask_chunk<1, MASK_RESTORE>(j, start4, rule);
        } else {
          with_nsrc(j.n_src, [&](auto S) {
            tall_rule_t<S()> rule = {p, n};
            if (j.mask[0]) mask_chunk<S(), MASK_WRITE>(j, start4, rule);
            else mask_chunk<S(), MASK_PLAIN>(j, start4, rule);
          });
        }
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_TALL_COUNTERS); });
}

extern "C" size_t vlm_tall_plan_bytes(int n_jobs, uint64_t total_elems) {
  return counts_plan_bytes<vlm_tall_header_t, vlm_tall_job_t>(n_jobs, total_elems, VLM_TALL_COUNTERS);
}

extern "C" int vlm_tall_plan_upload(const vlm_tall_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return counts_plan_upload<vlm_tall_header_t, VLM_TALL_COUNTERS>(jobs, n_jobs, workspace, workspace_bytes, stream, [](const vlm_tall_job_t& j) {
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);
    return rc == VLM_OK ? tall_job_check(j) : rc;
  });
}

extern "C" int vlm_tall_run(void* workspace, void* stream) {
  return counts_run(workspace, stream, vlm_tall_clear_kernel, vlm_tall_apply_kernel, chunk_grid(TALL_APPLY_BLOCKS_PER_CU));
}
