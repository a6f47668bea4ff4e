// TIES merge (trim, elect sign, disjoint mean; Yadav et al. 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no TIES.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/ties_restatement.py; the kernels are held to that restatement bit for bit.
//
// Trim needs, per (tensor, source), the K-th largest magnitude of the task vector t_m = W_m - c.  It is found exactly, on
// the device, by a radix select over key(x) = bits(x) & 0x7fffffff in three passes of 11 + 10 + 10 bits:
//   vlm_ties_hist_kernel<PASS>  one launch over the plan's 16-KiB chunk table (chunk_plan.h).  A workgroup owns a
//                               CONTIGUOUS run of chunks, recomputes t_m from W_m and c (16-B non-temporal loads; the task vectors
//                               are never stored), counts the digit of every key that still matches the prefix found so far in
//                               LDS histograms (integer LDS atomics) and adds the non-empty bins to the (job, source) histogram in
//                               global memory (64-bit integer atomics) when its run leaves a job.
//   vlm_ties_scan_kernel<PASS>  a tiny launch: per (job, source) walks the histogram from the top bin down, picks the bin that holds
//                               the K-th largest key, extends the prefix, keeps the rank left inside that bin, and ZEROES the
//                               histogram for the next pass / the next run.
//   vlm_ties_apply_kernel       steps 1-5 of the rule with the thresholds read from the workspace, and the per-job counters.
// Integer counters only, so nothing depends on the order workgroups run in.  HBM-bound: every pass streams 4 (S + 1) B per
// element; the apply pass also writes 4 B.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
// This file holds the rules (ties_bin, ties_elem), the scan kernel and the workspace layout; the key, a pass's bins and the
// histogram flush are ties_select.h's, shared with band.hip's two-rank select.  The streaming body of a
// chunk, a workgroup's run loop with its flush cap, the source-count dispatch, steps 3-5 and the counters are chunk_walk.h's; the
// chunk table, the per-job checks, the host image, the upload and the grid rule are chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"  // the chunk walker, the run loop, steps 3-5 and the counters: shared with dare.hip (and merge.hip)
#include "ties_select.h"  // the constants, the unit, the key, a pass's bins and shift, the histogram flush: shared with band.hip

template <int PASS>
__device__ __forceinline__ void ties_bin(uint32_t key, uint32_t prefix, uint32_t* h) {
  if (PASS == 0) atomicAdd(&h[key >> 20], 1u);
  else if (PASS == 1) { if ((key >> 20) == (prefix >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u); }
  else { if ((key >> 10) == (prefix >> 10)) atomicAdd(&h[key & 1023u], 1u); }
}

// a histogram pass as chunk_stream's rule (chunk_walk.h): stores nothing, bins every source of an element
template <int PASS, int NSRC>
struct ties_hist_rule {
  const uint32_t* prefix;
  uint32_t* lds;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
#pragma unroll
    for (int m = 0; m < NSRC; ++m) ties_bin<PASS>(ties_key(wv[m], c), prefix[m], lds + m * TIES_BINS);
    return 0.0f;
  }
};

struct ties_view_t {
  const vlm_ties_header_t* hdr;
  const vlm_ties_job_t* jobs;
  const chunk_t* chunks;
  const uint32_t* unit0;
  const ties_unit_t* units;
  vlm_ties_state_t* state;
  u64_t* hist;
  u64_t* counters;
};

__device__ __forceinline__ ties_view_t ties_view(unsigned char* ws) {
  ties_view_t v;
  v.hdr = reinterpret_cast<const vlm_ties_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_ties_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.unit0 = reinterpret_cast<const uint32_t*>(ws + v.hdr->unit0_off);
  v.units = reinterpret_cast<const ties_unit_t*>(ws + v.hdr->units_off);
  v.state = reinterpret_cast<vlm_ties_state_t*>(ws + v.hdr->state_off);
  v.hist = reinterpret_cast<u64_t*>(ws + v.hdr->hist_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

template <int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_ties_hist_kernel(unsigned char* __restrict__ ws) {
  __shared__ uint32_t lds[VLM_MERGE_MAX_SRC * TIES_BINS];
  const ties_view_t w = ties_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  for (uint32_t i = threadIdx.x; i < VLM_MERGE_MAX_SRC * TIES_BINS; i += TIES_THREADS) lds[i] = 0;
  __syncthreads();
  uint32_t prefix[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        if (PASS > 0) {
#pragma unroll
          for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m)
            if (m < w.jobs[cur].n_src) prefix[m] = w.state[w.unit0[cur] + m].key;
        }
      },
      [&](const vlm_ties_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          ties_hist_rule<PASS, S()> rule{prefix, lds};
          chunk_stream<S(), true, false>(j, start4, rule);
        });
      },
      [&](uint32_t cur) { ties_flush<PASS>(lds, w.hist + (uint64_t)w.unit0[cur] * TIES_BINS, w.jobs[cur].n_src); });
}

// One workgroup per (job, source): find the bin that holds the rank-th largest key, walking down from the top bin.
template <int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_ties_scan_kernel(unsigned char* __restrict__ ws) {
  constexpr int PER = ties_bins<PASS>() / TIES_THREADS;  // bins per thread: 8 or 4
  __shared__ u64_t part[TIES_THREADS];
  __shared__ u64_t sel_before;
  __shared__ int sel;
  const ties_view_t w = ties_view(ws);
  const uint32_t n_units = w.hdr->n_units;
  for (uint32_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const ties_unit_t uj = w.units[unit];
    u64_t* h = w.hist + (uint64_t)unit * TIES_BINS;
    const u64_t rank = PASS == 0 ? w.jobs[uj.job].k[uj.m] : w.state[unit].rank;
    const uint32_t prefix = PASS == 0 ? 0u : w.state[unit].key;
    if (PASS == 0 && uj.m == 0 && threadIdx.x < VLM_TIES_COUNTERS)  // the counters of the job start every run at zero
      w.counters[(uint64_t)uj.job * VLM_TIES_COUNTERS + threadIdx.x] = 0;
    // thread t owns bins hi, hi-1, ..., hi-PER+1 with hi = BINS-1 - t*PER: thread order is descending key order
    const int hi = (int)ties_bins<PASS>() - 1 - (int)threadIdx.x * PER;
    u64_t local[PER];
    u64_t sum = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      local[q] = h[hi - q];
      h[hi - q] = 0;  // ready for the next pass and the next run
      sum += local[q];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64_t cum = 0;
      int t = 0;
      for (; t < TIES_THREADS - 1; ++t) {
        if (cum + part[t] >= rank) break;
        cum += part[t];
      }
      sel = t;
      sel_before = cum;
    }
    __syncthreads();
    if ((int)threadIdx.x == sel) {
      u64_t cum = sel_before;
      int q = 0;
      for (; q < PER - 1; ++q) {
        if (cum + local[q] >= rank) break;
        cum += local[q];
      }
      vlm_ties_state_t st;
      st.key = prefix | ((uint32_t)(hi - q) << ties_shift<PASS>());
      st.reserved = 0;
      st.rank = rank - cum;
      w.state[unit] = st;
    }
    __syncthreads();
  }
}

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
  return ties_elect<NSRC>(c, tt, lam, n);                                // steps 3-5 (chunk_walk.h)
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
  const ties_view_t w = ties_view(ws);
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

// fills every offset of `h` for n_jobs jobs, n_units (job, source) pairs and n_chunks chunks; returns the total size
static size_t ties_layout(vlm_ties_header_t* h, uint64_t n_jobs, uint64_t n_units, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(vlm_ties_header_t));
  h->n_jobs = n_jobs;
  h->n_units = n_units;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(vlm_ties_job_t));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  h->unit0_off = at.take(n_jobs * sizeof(uint32_t));
  h->units_off = at.take(n_units * sizeof(ties_unit_t));
  h->state_off = at.take(n_units * sizeof(vlm_ties_state_t));
  h->counters_off = at.take(n_jobs * VLM_TIES_COUNTERS * sizeof(uint64_t));
  h->hist_off = at.take(n_units * TIES_BINS * sizeof(uint64_t));
  return at.off;
}

extern "C" size_t vlm_ties_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  // upper bounds: chunks_bound, and every job has at most VLM_MERGE_MAX_SRC sources
  vlm_ties_header_t h;
  return ties_layout(&h, (uint64_t)n_jobs, (uint64_t)n_jobs * VLM_MERGE_MAX_SRC, chunks_bound(n_jobs, total_elems));
}

extern "C" int vlm_ties_plan_upload(const vlm_ties_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_chunks = 0, n_units = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_ties_job_t& j = jobs[i];
    if (j.n_elem == 0) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, true);
    if (rc != VLM_OK) return rc;
    for (int m = 0; m < j.n_src; ++m)
      if (j.k[m] < 1 || j.k[m] > j.n_elem) return VLM_ERR_ARG;
    n_chunks += chunks_of(j.n_elem);
    n_units += (uint64_t)j.n_src;
  }
  if (!chunk_count_ok(n_chunks) || n_units >= (1ull << 32)) return VLM_ERR_UNSUPPORTED;
  vlm_ties_header_t hdr;
  const size_t total = ties_layout(&hdr, (uint64_t)n_jobs, n_units, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the state begins: state, counters and histograms are device-made
  std::vector<unsigned char> img = chunk_image(hdr, jobs, n_jobs, hdr.state_off);
  uint32_t* unit0 = reinterpret_cast<uint32_t*>(img.data() + hdr.unit0_off);
  ties_unit_t* units = reinterpret_cast<ties_unit_t*>(img.data() + hdr.units_off);
  uint64_t u = 0;
  for (int i = 0; i < n_jobs; ++i) {
    unit0[i] = (uint32_t)u;
    for (int m = 0; m < jobs[i].n_src; ++m) {
      units[u].job = (uint32_t)i;
      units[u].m = (uint32_t)m;
      ++u;
    }
  }
  // the histograms start at zero; every scan launch leaves them at zero again
  return chunk_upload(workspace, img, total - hdr.state_off, (hipStream_t)stream);
}

extern "C" int vlm_ties_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(TIES_THREADS), hist_grid = chunk_grid(TIES_HIST_BLOCKS_PER_CU), scan_grid(TIES_SCAN_BLOCKS),
             apply_grid = chunk_grid(TIES_APPLY_BLOCKS_PER_CU);
  // seven launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL((vlm_ties_hist_kernel<0>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_ties_scan_kernel<0>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_ties_hist_kernel<1>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_ties_scan_kernel<1>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_ties_hist_kernel<2>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_ties_scan_kernel<2>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL(vlm_ties_apply_kernel, apply_grid, block, 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
