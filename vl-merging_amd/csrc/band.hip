// Model Breadcrumbs merge (magnitude band trim; Davari & Belilovsky 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no such merge.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/band_restatement.py; the kernels are held to that restatement bit for bit.
//
// The trim needs, per (tensor, source), TWO order statistics of the task vector t_m = W_m - c: the k_hi-th and the k_lo-th largest
// magnitude.  Both come out of ONE radix select, ties_select.h's with TWO ranks per source (rank 0 is k_lo, rank 1 is k_hi), so a
// run streams the inputs four times as a TIES run does, not six: three histogram launches (vlm_select_hist_kernel<band_sel, PASS>),
// a pick of both bins after each (vlm_select_scan_kernel<band_sel, PASS>), then
//   vlm_band_apply_kernel       steps 1-4 of the rule with both thresholds read from the workspace, and the per-job counters.
// k_hi = 0 (no outliers) is the select's "no such rank": thr_hi is then SELECT_NO_RANK, above every key, and `key >= thr_hi` is
// false for every entry in the apply pass.
// Integer counters only, so nothing depends on the order workgroups run in.  HBM-bound: every pass streams 4 (S + 1) B per
// element; the apply pass also writes 4 B.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
// This file holds what is the band merge's own: what the select needs to know of its job and state (band_sel), the element rule
// (band_elem), the apply kernel and the checks on the mode and the ranks.  The select, the workspace layout, the upload and the
// seven-launch run are ties_select.h's (shared with ties.hip) -- the grids are the TIES ones: the histogram passes hold what the
// TIES passes hold, and the apply pass is resident three to a CU like vlm_ties_apply_kernel; no other grid was timed
// (docs/experiments.md, "Breadcrumbs merge").  The chunk walker, the run loop, the combine rule and the counter flush are
// chunk_walk.h's, the chunk table, the family's per-job checks, the upload and the grid rule chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "ties_select.h"

struct band_sel {
  typedef vlm_band_job_t job_t;
  typedef vlm_band_header_t hdr_t;
  typedef vlm_band_state_t state_t;
  static constexpr int RANKS = 2, COUNTERS = VLM_BAND_COUNTERS, RECORD_DOUBLES = 0;
  static constexpr bool ELEM_KEY = false;  // one unit per (job, source)
  static __device__ __forceinline__ u64_t want(const job_t& j, uint32_t m, int r) { return r == 0 ? j.k_lo[m] : j.k_hi[m]; }
  static __device__ __forceinline__ bool none(const job_t& j, uint32_t m, int r) { return r == 1 && j.k_hi[m] == 0; }
  static __device__ __forceinline__ uint32_t key(const state_t& s, int r) { return r == 0 ? s.key_lo : s.key_hi; }
  static __device__ __forceinline__ u64_t rank(const state_t& s, int r) { return r == 0 ? s.rank_lo : s.rank_hi; }
  static __device__ __forceinline__ void store(state_t& s, int r, uint32_t key, u64_t left) {
    (r == 0 ? s.key_lo : s.key_hi) = key;
    (r == 0 ? s.rank_lo : s.rank_hi) = left;
  }
  static bool mode_ok(const job_t& j) { return j.mode == VLM_BAND_LINEAR || j.mode == VLM_BAND_TIES; }
  static bool ranks_ok(const job_t& j, int m) { return j.k_hi[m] < j.k_lo[m] && j.k_lo[m] <= j.n_elem; }
};

// the ten counters of a job in their order in the workspace: kept[0..3], outlier[0..3], conflict, empty
struct band_counts_t {
  uint32_t c[VLM_BAND_COUNTERS];
};
#define BAND_CONFLICT (2 * VLM_MERGE_MAX_SRC)
#define BAND_EMPTY (2 * VLM_MERGE_MAX_SRC + 1)

template <int NSRC, int MODE>
__device__ __forceinline__ float band_elem(float c, const float* wv, const uint32_t* lo, const uint32_t* hi, float lam,
                                           band_counts_t& n) {
  float tt[NSRC];
  int any = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float t = __fsub_rn(wv[m], c);                                 // step 1
    const uint32_t key = __float_as_uint(t) & 0x7fffffffu;               // step 2
    const bool outl = key >= hi[m];
    const bool kept = key >= lo[m] && !outl;
    tt[m] = kept ? t : 0.0f;
    n.c[m] += kept ? 1u : 0u;
    n.c[VLM_MERGE_MAX_SRC + m] += outl ? 1u : 0u;
    any += kept ? 1 : 0;
  }
  return combine<NSRC, MODE>(c, tt, any, lam, n.c[BAND_CONFLICT], n.c[BAND_EMPTY]);  // steps 3-4 (chunk_walk.h)
}

// steps 1-4 as chunk_stream's rule
template <int NSRC, int MODE>
struct band_apply_rule {
  const uint32_t* lo;
  const uint32_t* hi;
  float lam;
  band_counts_t& n;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
    return band_elem<NSRC, MODE>(c, wv, lo, hi, lam, n);
  }
};

__global__ __launch_bounds__(TIES_THREADS) void vlm_band_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(TIES_THREADS / 64) * VLM_BAND_COUNTERS];
  const select_view_t<band_sel> w = select_view<band_sel>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  band_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_BAND_COUNTERS; ++k) n.c[k] = 0;
  uint32_t lo[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0}, hi[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m)
          if (m < w.jobs[cur].n_src) {
            lo[m] = w.state[w.unit0[cur] + m].key_lo;
            hi[m] = w.state[w.unit0[cur] + m].key_hi;
          }
      },
      [&](const vlm_band_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          if (j.mode == VLM_BAND_TIES) {
            band_apply_rule<S(), VLM_BAND_TIES> rule{lo, hi, j.lam, n};
            chunk_stream<S(), true, true>(j, start4, rule);
          } else {
            band_apply_rule<S(), VLM_BAND_LINEAR> rule{lo, hi, j.lam, n};
            chunk_stream<S(), true, true>(j, start4, rule);
          }
        });
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_BAND_COUNTERS); });
}

extern "C" size_t vlm_band_plan_bytes(int n_jobs, uint64_t total_elems) { return select_plan_bytes<band_sel>(n_jobs, total_elems); }

extern "C" int vlm_band_plan_upload(const vlm_band_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return select_plan_upload<band_sel>(jobs, n_jobs, workspace, workspace_bytes, stream);
}

extern "C" int vlm_band_run(void* workspace, void* stream) { return select_run<band_sel>(workspace, stream, vlm_band_apply_kernel); }
