// TIES merge (trim, elect sign, disjoint mean; Yadav et al. 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no TIES.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/ties_restatement.py; the kernels are held to that restatement bit for bit.
//
// Trim needs, per (tensor, source), the K-th largest magnitude of the task vector t_m = W_m - c.  It is found exactly, on
// the device, by ties_select.h's radix select with ONE rank per source: three histogram launches
// (vlm_select_hist_kernel<ties_sel, PASS>), a bin pick after each (vlm_select_scan_kernel<ties_sel, PASS>), then
//   vlm_ties_apply_kernel       steps 1-5 of the rule with the thresholds read from the workspace, and the per-job counters.
// Integer counters only, so nothing depends on the order workgroups run in.  HBM-bound: every pass streams 4 (S + 1) B per
// element; the apply pass also writes 4 B.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
// This file holds what is TIES's own: what the select needs to know of its job and state (ties_sel), the element rule
// (ties_elem), the apply kernel and the checks on k.  The select, the workspace layout, the upload and the seven-launch run are
// ties_select.h's (shared with band.hip); the streaming body of a chunk, a workgroup's run loop with its flush cap, the
// source-count dispatch, steps 3-5 and the counters are chunk_walk.h's; the chunk table, the family's per-job checks, the host
// image, the upload and the grid rule are chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"   // the chunk walker, the run loop, the combine rule and the counters: the whole family's
#include "ties_select.h"  // the radix select, its workspace and its run: shared with band.hip

struct ties_sel {
  typedef vlm_ties_job_t job_t;
  typedef vlm_ties_header_t hdr_t;
  typedef vlm_ties_state_t state_t;
  static constexpr int RANKS = 1, COUNTERS = VLM_TIES_COUNTERS, RECORD_DOUBLES = 0;
  static constexpr bool ELEM_KEY = false;  // one unit per (job, source)
  static __device__ __forceinline__ u64_t want(const job_t& j, uint32_t m, int) { return j.k[m]; }
  static __device__ __forceinline__ bool none(const job_t&, uint32_t, int) { return false; }
  static __device__ __forceinline__ uint32_t key(const state_t& s, int) { return s.key; }
  static __device__ __forceinline__ u64_t rank(const state_t& s, int) { return s.rank; }
  static __device__ __forceinline__ void store(state_t& s, int, uint32_t key, u64_t left) { s = state_t{key, 0u, left}; }
  static bool mode_ok(const job_t&) { return true; }
  static bool ranks_ok(const job_t& j, int m) { return j.k[m] >= 1 && j.k[m] <= j.n_elem; }
};

template <int NSRC>
__device__ __forceinline__ float ties_elem(float c, const float* wv, const uint32_t* thr, float lam, ties_counts_t& n) {
  float tt[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float t = __fsub_rn(wv[m], c);                                 // step 1
    const bool kept = (__float_as_uint(t) & 0x7fffffffu) >= thr[m];      // step 2
    tt[m] = kept ? t : 0.0f;
    n.c[m] += kept ? 1u : 0u;
  }
  return ties_elect<NSRC>(c, tt, lam, n.c[TIES_CONFLICT], n.c[TIES_EMPTY]);  // steps 3-5 (chunk_walk.h)
}

// steps 1-5 as chunk_stream's rule
template <int NSRC>
struct ties_apply_rule {
  const uint32_t* thr;
  float lam;
  ties_counts_t& n;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
    return ties_elem<NSRC>(c, wv, thr, lam, n);
  }
};

__global__ __launch_bounds__(TIES_THREADS) void vlm_ties_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(TIES_THREADS / 64) * VLM_TIES_COUNTERS];
  const select_view_t<ties_sel> w = select_view<ties_sel>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_TIES_COUNTERS; ++k) n.c[k] = 0;
  uint32_t thr[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m)
          if (m < w.jobs[cur].n_src) thr[m] = w.state[w.unit0[cur] + m].key;
      },
      [&](const vlm_ties_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          ties_apply_rule<S()> rule{thr, j.lam, n};
          chunk_stream<S(), true, true>(j, start4, rule);
        });
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_TIES_COUNTERS); });
}

extern "C" size_t vlm_ties_plan_bytes(int n_jobs, uint64_t total_elems) { return select_plan_bytes<ties_sel>(n_jobs, total_elems); }

extern "C" int vlm_ties_plan_upload(const vlm_ties_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return select_plan_upload<ties_sel>(jobs, n_jobs, workspace, workspace_bytes, stream);
}

extern "C" int vlm_ties_run(void* workspace, void* stream) { return select_run<ties_sel>(workspace, stream, vlm_ties_apply_kernel); }
