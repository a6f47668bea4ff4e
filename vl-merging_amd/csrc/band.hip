// Model Breadcrumbs merge (magnitude band trim; Davari & Belilovsky 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no such merge.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/band_restatement.py; the kernels are held to that restatement bit for bit.
//
// The trim needs, per (tensor, source), TWO order statistics of the task vector t_m = W_m - c: the k_hi-th and the k_lo-th largest
// magnitude.  Both come out of ONE radix select over key(x) = bits(x) & 0x7fffffff, the three passes of ties.hip (11 + 10 + 10
// bits), so a run streams the inputs four times as a TIES run does, not six:
//   vlm_band_hist_kernel<PASS>  ties.hip's histogram pass with two prefixes per source.  Pass 0 does not look at a rank: one
//                               2048-bin histogram per source serves both.  Passes 1 and 2 use 1024 bins per rank, so the two
//                               ranks' conditional histograms are the two halves of the source's 2048-bin slot (k_lo: bins
//                               0 .. 1023, k_hi: bins 1024 .. 2047) -- the LDS (32 KiB), the global histograms and the occupancy
//                               are those of the TIES pass.  A key that matches both prefixes (both ranks in one bin so far) is
//                               counted in both halves.
//   vlm_band_scan_kernel<PASS>  a tiny launch: per (job, source) walks down from the top bin for both ranks (two waves, one rank
//                               each), extends both prefixes, keeps both residual ranks and ZEROES the bins.
//   vlm_band_apply_kernel       steps 1-4 of the rule with both thresholds read from the workspace, and the per-job counters.
// k_hi = 0 (no outliers) is stated, not derived: the scan walks nothing for it and leaves the key 0x80000000.  No key reaches it
// (a key has 31 bits), so its prefix (0x800 after pass 0, 0x200000 after pass 1) matches nothing in passes 1 and 2 -- that half
// of the bins stays empty -- and `key >= thr_hi` is false for every entry in the apply pass.
// Integer counters only, so nothing depends on the order workgroups run in.  HBM-bound: every pass streams 4 (S + 1) B per
// element; the apply pass also writes 4 B.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
// This file holds the rules (band_bin, band_elem), the scan kernel and the workspace layout; the key, the
// bins of a pass and the histogram flush are ties_select.h's (shared with ties.hip), the chunk walker, the run loop and steps 3-4
// of the TIES mode and the counter flush chunk_walk.h's, the chunk table, the per-job checks, the upload and the grid rule chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "ties_select.h"

// The grids are the TIES ones (ties_select.h): the histogram passes hold what the TIES passes hold, and the apply pass is
// resident three to a CU like vlm_ties_apply_kernel.  No other grid was timed (docs/experiments.md, "Breadcrumbs merge").
#define BAND_HALF 1024u  // passes 1 and 2: k_lo's bins start at 0, k_hi's at BAND_HALF
#define BAND_NO_OUTLIER 0x80000000u  // thr_hi of k_hi = 0: above every key

template <int PASS>
__device__ __forceinline__ void band_bin(uint32_t key, uint32_t plo, uint32_t phi, uint32_t* h) {
  if (PASS == 0) atomicAdd(&h[key >> 20], 1u);
  else if (PASS == 1) {
    if ((key >> 20) == (plo >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u);
    if ((key >> 20) == (phi >> 20)) atomicAdd(&h[BAND_HALF + ((key >> 10) & 1023u)], 1u);
  } else {
    if ((key >> 10) == (plo >> 10)) atomicAdd(&h[key & 1023u], 1u);
    if ((key >> 10) == (phi >> 10)) atomicAdd(&h[BAND_HALF + (key & 1023u)], 1u);
  }
}

// a histogram pass as chunk_stream's rule (chunk_walk.h): stores nothing, bins every source of an element
template <int PASS, int NSRC>
struct band_hist_rule {
  const uint32_t* plo;
  const uint32_t* phi;
  uint32_t* lds;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
#pragma unroll
    for (int m = 0; m < NSRC; ++m) band_bin<PASS>(ties_key(wv[m], c), plo[m], phi[m], lds + m * TIES_BINS);
    return 0.0f;
  }
};

struct band_view_t {
  const vlm_band_header_t* hdr;
  const vlm_band_job_t* jobs;
  const chunk_t* chunks;
  const uint32_t* unit0;
  const ties_unit_t* units;
  vlm_band_state_t* state;
  u64_t* hist;
  u64_t* counters;
};

__device__ __forceinline__ band_view_t band_view(unsigned char* ws) {
  band_view_t v;
  v.hdr = reinterpret_cast<const vlm_band_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_band_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.unit0 = reinterpret_cast<const uint32_t*>(ws + v.hdr->unit0_off);
  v.units = reinterpret_cast<const ties_unit_t*>(ws + v.hdr->units_off);
  v.state = reinterpret_cast<vlm_band_state_t*>(ws + v.hdr->state_off);
  v.hist = reinterpret_cast<u64_t*>(ws + v.hdr->hist_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

template <int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_band_hist_kernel(unsigned char* __restrict__ ws) {
  __shared__ uint32_t lds[VLM_MERGE_MAX_SRC * TIES_BINS];
  const band_view_t w = band_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  for (uint32_t i = threadIdx.x; i < VLM_MERGE_MAX_SRC * TIES_BINS; i += TIES_THREADS) lds[i] = 0;
  __syncthreads();
  uint32_t plo[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0}, phi[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        if (PASS > 0) {
#pragma unroll
          for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m)
            if (m < w.jobs[cur].n_src) {
              plo[m] = w.state[w.unit0[cur] + m].key_lo;
              phi[m] = w.state[w.unit0[cur] + m].key_hi;
            }
        }
      },
      [&](const vlm_band_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          band_hist_rule<PASS, S()> rule{plo, phi, lds};
          chunk_stream<S(), true, false>(j, start4, rule);
        });
      },
      // every pass flushes the whole 2048-bin slot of a source: pass 0's one histogram, or the two halves of passes 1 and 2
      [&](uint32_t cur) { ties_flush<0>(lds, w.hist + (uint64_t)w.unit0[cur] * TIES_BINS, w.jobs[cur].n_src); });
}

// One workgroup per (job, source): find, for both ranks, the bin that holds the rank-th largest key, walking down from the top
// bin.  r = 0 is k_lo, r = 1 is k_hi; pass 0 walks the one histogram for both, passes 1 and 2 walk each rank's own half.
template <int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_band_scan_kernel(unsigned char* __restrict__ ws) {
  constexpr int PER = ties_bins<PASS>() / TIES_THREADS;  // bins per thread and histogram: 8 or 4
  constexpr int NH = PASS == 0 ? 1 : 2;                  // histograms in a unit's slot
  __shared__ u64_t part[NH][TIES_THREADS];
  __shared__ u64_t sel_before[2];
  __shared__ int sel[2];
  const band_view_t w = band_view(ws);
  const uint32_t n_units = w.hdr->n_units;
  for (uint32_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const ties_unit_t uj = w.units[unit];
    u64_t* h = w.hist + (uint64_t)unit * TIES_BINS;
    const vlm_band_state_t before = w.state[unit];
    const bool no_hi = w.jobs[uj.job].k_hi[uj.m] == 0;
    const u64_t rank[2] = {PASS == 0 ? w.jobs[uj.job].k_lo[uj.m] : before.rank_lo,
                           PASS == 0 ? w.jobs[uj.job].k_hi[uj.m] : before.rank_hi};
    const uint32_t prefix[2] = {PASS == 0 ? 0u : before.key_lo, PASS == 0 ? 0u : before.key_hi};
    if (PASS == 0 && uj.m == 0 && threadIdx.x < VLM_BAND_COUNTERS)  // the counters of the job start every run at zero
      w.counters[(uint64_t)uj.job * VLM_BAND_COUNTERS + threadIdx.x] = 0;
    // thread t owns bins hi, hi-1, ..., hi-PER+1 of each histogram, hi = BINS-1 - t*PER: thread order is descending key order
    const int hi = (int)ties_bins<PASS>() - 1 - (int)threadIdx.x * PER;
    u64_t local[NH][PER];
#pragma unroll
    for (int g = 0; g < NH; ++g) {
      u64_t sum = 0;
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        local[g][q] = h[g * BAND_HALF + hi - q];
        h[g * BAND_HALF + hi - q] = 0;  // ready for the next pass and the next run
        sum += local[g][q];
      }
      part[g][threadIdx.x] = sum;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {  // thread 0 walks for k_lo, thread 64 (another wave) for k_hi
      const int r = threadIdx.x >> 6, g = NH == 1 ? 0 : r;
      u64_t cum = 0;
      int t = 0;
      if (!(r == 1 && no_hi)) {  // k_hi = 0: nothing is walked
        for (; t < TIES_THREADS - 1; ++t) {
          if (cum + part[g][t] >= rank[r]) break;
          cum += part[g][t];
        }
      }
      sel[r] = t;
      sel_before[r] = cum;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if ((int)threadIdx.x == sel[r]) {
        const int g = NH == 1 ? 0 : r;
        u64_t cum = sel_before[r];
        int q = 0;
        for (; q < PER - 1; ++q) {
          if (cum + local[g][q] >= rank[r]) break;
          cum += local[g][q];
        }
        uint32_t key = prefix[r] | ((uint32_t)(hi - q) << ties_shift<PASS>());
        u64_t left = rank[r] - cum;
        if (r == 1 && no_hi) {
          key = BAND_NO_OUTLIER;
          left = 0;
        }
        if (r == 0) {
          w.state[unit].key_lo = key;
          w.state[unit].rank_lo = left;
        } else {
          w.state[unit].key_hi = key;
          w.state[unit].rank_hi = left;
        }
      }
    }
    __syncthreads();
  }
}

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
  if (MODE == VLM_BAND_TIES) {                                           // steps 3-4: the TIES rule's 3-5 (chunk_walk.h)
    ties_counts_t e = {};  // ties_elect counts this element's conflict and empty into the TIES slots
    const float o = ties_elect<NSRC>(c, tt, lam, e);
    n.c[BAND_CONFLICT] += e.c[VLM_MERGE_MAX_SRC];
    n.c[BAND_EMPTY] += e.c[VLM_MERGE_MAX_SRC + 1];
    return o;
  }
  float d = 0.0f;
  bool has_pos = false, has_neg = false;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {                                       // step 3, LINEAR
    d = __fadd_rn(d, tt[m]);
    has_pos |= tt[m] > 0.0f;
    has_neg |= tt[m] < 0.0f;
  }
  n.c[BAND_CONFLICT] += (has_pos && has_neg) ? 1u : 0u;
  n.c[BAND_EMPTY] += any == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(lam, d));                                // step 4
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
  const band_view_t w = band_view(ws);
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

// fills every offset of `h` for n_jobs jobs, n_units (job, source) pairs and n_chunks chunks; returns the total size
static size_t band_layout(vlm_band_header_t* h, uint64_t n_jobs, uint64_t n_units, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(vlm_band_header_t));
  h->n_jobs = n_jobs;
  h->n_units = n_units;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(vlm_band_job_t));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  h->unit0_off = at.take(n_jobs * sizeof(uint32_t));
  h->units_off = at.take(n_units * sizeof(ties_unit_t));
  h->state_off = at.take(n_units * sizeof(vlm_band_state_t));
  h->counters_off = at.take(n_jobs * VLM_BAND_COUNTERS * sizeof(uint64_t));
  h->hist_off = at.take(n_units * TIES_BINS * sizeof(uint64_t));
  return at.off;
}

extern "C" size_t vlm_band_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  // upper bounds: chunks_bound, and every job has at most VLM_MERGE_MAX_SRC sources
  vlm_band_header_t h;
  return band_layout(&h, (uint64_t)n_jobs, (uint64_t)n_jobs * VLM_MERGE_MAX_SRC, chunks_bound(n_jobs, total_elems));
}

extern "C" int vlm_band_plan_upload(const vlm_band_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_chunks = 0, n_units = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_band_job_t& j = jobs[i];
    if (j.n_elem == 0 || (j.mode != VLM_BAND_LINEAR && j.mode != VLM_BAND_TIES)) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, true);
    if (rc != VLM_OK) return rc;
    for (int m = 0; m < j.n_src; ++m)
      if (j.k_hi[m] >= j.k_lo[m] || j.k_lo[m] > j.n_elem) return VLM_ERR_ARG;
    n_chunks += chunks_of(j.n_elem);
    n_units += (uint64_t)j.n_src;
  }
  if (!chunk_count_ok(n_chunks) || n_units >= (1ull << 32)) return VLM_ERR_UNSUPPORTED;
  vlm_band_header_t hdr;
  const size_t total = band_layout(&hdr, (uint64_t)n_jobs, n_units, n_chunks);
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

extern "C" int vlm_band_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(TIES_THREADS), hist_grid = chunk_grid(TIES_HIST_BLOCKS_PER_CU), scan_grid(TIES_SCAN_BLOCKS),
             apply_grid = chunk_grid(TIES_APPLY_BLOCKS_PER_CU);
  // seven launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL((vlm_band_hist_kernel<0>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_band_scan_kernel<0>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_band_hist_kernel<1>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_band_scan_kernel<1>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_band_hist_kernel<2>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_band_scan_kernel<2>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL(vlm_band_apply_kernel, apply_grid, block, 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
