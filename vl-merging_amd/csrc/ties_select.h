// The radix select of ties.hip (one rank per source) and band.hip (two ranks per source), written once and instantiated per
// method: per (job, source) "unit" it finds, exactly and on the device, the RANKS wanted order statistics of
// key(x) = bits(x) & 0x7fffffff over the task vector t_m = W_m - c, in three passes of 11 + 10 + 10 bits.
//   vlm_select_hist_kernel<Sel, PASS>  one launch over the plan's 16-KiB chunk table (chunk_plan.h).  A workgroup owns a CONTIGUOUS
//                                      run of chunks, recomputes t_m from W_m and c (the task vectors are never stored), counts in
//                                      LDS (integer atomics) the digit of every key that still matches a prefix found so far, and
//                                      adds the non-empty bins to the unit's histogram in global memory (64-bit integer atomics)
//                                      when its run leaves a job.  Pass 0 looks at no rank: ONE 2048-bin histogram per source
//                                      serves all.  Passes 1 and 2 use 1024 bins per rank, rank r at SELECT_HALF * r of the
//                                      source's 2048-bin slot, so the LDS (32 KiB) does not grow with RANKS; a key that matches
//                                      two prefixes (both ranks in one bin so far) is counted in both halves.
//   vlm_select_scan_kernel<Sel, PASS>  a tiny launch: per unit one wave per rank walks that rank's histogram from the top bin down,
//                                      picks the bin that holds the rank-th largest key, extends the prefix, keeps the rank left
//                                      inside that bin -- and the workgroup ZEROES the bins for the next pass / the next run and,
//                                      in pass 0, the job's counters.
// "No such rank" (the band merge's k_hi = 0) is stated, not derived: the scan walks nothing for it and leaves the key
// SELECT_NO_RANK.  No key reaches it (a key has 31 bits), so its prefix (0x800 after pass 0, 0x200000 after pass 1) matches
// nothing in passes 1 and 2 -- that half of the bins stays empty -- and `key >= threshold` is false for every entry afterwards.
//
// A method gives a traits type Sel: job_t / hdr_t / state_t (include/vlm_hip.h; the headers are field for field the same),
// RANKS (1 or 2), COUNTERS, on the device want(job, m, r) (the rank asked for), none(job, m, r) (no such rank), key(state, r),
// rank(state, r), store(state, r, key, rank left), and on the host mode_ok(job) and ranks_ok(job, m), its own job checks.
// Everything below is then the method's but for its element rule and apply kernel.
//
// ELEM_KEY (sce.hip): the unit is the JOB, not the (job, source) pair -- the key is a function of the element's c and ALL its
// sources, Sel::elem_key<NSRC>(c, wv), one 2048-bin histogram per job in global memory and ONE per workgroup in LDS (8 KiB, not
// 32); m is 0 wherever the traits are asked.  RECORD_DOUBLES > 0: the header also has first_off (the first chunk of each job,
// host-made) and records_off (that many doubles per chunk, device-made), for a reduction that follows the select.  ties_sel and
// band_sel say false and 0 and get the kernels and the layout they had.
#pragma once
#include "vlm_common.h"
#include "chunk_walk.h"

#define TIES_THREADS CHUNK_THREADS  // the chunk walkers need the chunk's 256; the scan kernel uses the same block
#define TIES_BINS 2048u           // bins per source in LDS and in global memory (pass 0 uses all, passes 1 and 2 use 1024 per rank)
#define TIES_HIST_BLOCKS_PER_CU 4  // under 128 VGPRs: four workgroups (one wave per SIMD each) are resident per CU; 32 KiB LDS each
#define TIES_APPLY_BLOCKS_PER_CU 12  // three resident per CU (145 VGPRs): four even rounds
#define TIES_SCAN_BLOCKS 1024
// The three grid sizes above follow from the kernels' resident-workgroup counts (register and LDS use recorded by the build); none of
// them has been A/B-measured against other values (docs/experiments.md, "TIES merge", "Breadcrumbs merge").
#define SELECT_HALF 1024u            // passes 1 and 2: the bins of rank r start at SELECT_HALF * r
#define SELECT_NO_RANK 0x80000000u   // the threshold key of a rank that is not asked for: above every key

struct ties_unit_t {  // one (job, source) pair
  uint32_t job;
  uint32_t m;
};

template <int PASS>
__device__ __forceinline__ constexpr uint32_t ties_bins() { return PASS == 0 ? 2048u : 1024u; }
template <int PASS>
__device__ __forceinline__ constexpr int ties_shift() { return PASS == 0 ? 20 : (PASS == 1 ? 10 : 0); }

__device__ __forceinline__ uint32_t ties_key(float w, float c) { return __float_as_uint(__fsub_rn(w, c)) & 0x7fffffffu; }

// how many units a job has: one per source, or the job itself
template <class Sel>
__host__ __device__ __forceinline__ int select_units(const typename Sel::job_t& j) {
  if constexpr (Sel::ELEM_KEY) return 1;
  else return j.n_src;
}
template <class Sel>
constexpr int select_slots() { return Sel::ELEM_KEY ? 1 : VLM_MERGE_MAX_SRC; }  // histograms a workgroup holds in LDS

template <class Sel>
struct select_view_t {
  const typename Sel::hdr_t* hdr;
  const typename Sel::job_t* jobs;
  const chunk_t* chunks;
  const uint32_t* unit0;
  const ties_unit_t* units;
  typename Sel::state_t* state;
  u64_t* hist;
  u64_t* counters;
};

template <class Sel>
__device__ __forceinline__ select_view_t<Sel> select_view(unsigned char* ws) {
  select_view_t<Sel> v;
  v.hdr = reinterpret_cast<const typename Sel::hdr_t*>(ws);
  v.jobs = reinterpret_cast<const typename Sel::job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.unit0 = reinterpret_cast<const uint32_t*>(ws + v.hdr->unit0_off);
  v.units = reinterpret_cast<const ties_unit_t*>(ws + v.hdr->units_off);
  v.state = reinterpret_cast<typename Sel::state_t*>(ws + v.hdr->state_off);
  v.hist = reinterpret_cast<u64_t*>(ws + v.hdr->hist_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

// one key into a source's bins `h`; p0 / p1: the prefixes of rank 0 / rank 1 (p1 is not looked at with one rank)
template <int RANKS, int PASS>
__device__ __forceinline__ void select_bin(uint32_t key, uint32_t p0, uint32_t p1, uint32_t* h) {
  if (PASS == 0) atomicAdd(&h[key >> 20], 1u);
  else if (PASS == 1) {
    if ((key >> 20) == (p0 >> 20)) atomicAdd(&h[(key >> 10) & 1023u], 1u);
    if (RANKS > 1 && (key >> 20) == (p1 >> 20)) atomicAdd(&h[SELECT_HALF + ((key >> 10) & 1023u)], 1u);
  } else {
    if ((key >> 10) == (p0 >> 10)) atomicAdd(&h[key & 1023u], 1u);
    if (RANKS > 1 && (key >> 10) == (p1 >> 10)) atomicAdd(&h[SELECT_HALF + (key & 1023u)], 1u);
  }
}

// a histogram pass as chunk_stream's rule (chunk_walk.h): stores nothing, bins every source of an element
template <int RANKS, int PASS, int NSRC>
struct select_hist_rule {
  const uint32_t* p0;
  const uint32_t* p1;
  uint32_t* lds;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
#pragma unroll
    for (int m = 0; m < NSRC; ++m) select_bin<RANKS, PASS>(ties_key(wv[m], c), p0[m], p1[m], lds + m * TIES_BINS);
    return 0.0f;
  }
};

// the element-keyed pass: one key per element into the workgroup's one histogram
template <class Sel, int PASS, int NSRC>
struct select_elem_hist_rule {
  const uint32_t& p0;
  uint32_t* lds;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float c, const float* wv) const {
    select_bin<1, PASS>(Sel::template elem_key<NSRC>(c, wv), p0, 0u, lds);
    return 0.0f;
  }
};

// a workgroup's LDS histograms into a job's global ones: the first BINS bins of every source
template <uint32_t BINS>
__device__ __forceinline__ void select_flush(uint32_t* lds, u64_t* hist, int n_src) {
  __syncthreads();  // every LDS atomic of the run has landed
  for (int m = 0; m < n_src; ++m)
    for (uint32_t i = threadIdx.x; i < BINS; i += TIES_THREADS) {
      const uint32_t cnt = lds[m * TIES_BINS + i];
      if (cnt) {
        __hip_atomic_fetch_add(&hist[(uint64_t)m * TIES_BINS + i], (u64_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lds[m * TIES_BINS + i] = 0;
      }
    }
  __syncthreads();
}

template <class Sel, int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_select_hist_kernel(unsigned char* __restrict__ ws) {
  static_assert(Sel::RANKS == 1 || Sel::RANKS == 2, "a source's 2048-bin slot holds the 1024-bin halves of at most two ranks");
  static_assert(!Sel::ELEM_KEY || Sel::RANKS == 1, "the element-keyed rule bins for one rank");
  constexpr int SLOTS = select_slots<Sel>();
  // a run can have touched 1024 bins per source with one rank in passes 1 and 2, otherwise the whole slot
  constexpr uint32_t TOUCHED = PASS > 0 && Sel::RANKS == 1 ? ties_bins<PASS>() : TIES_BINS;
  __shared__ uint32_t lds[SLOTS * TIES_BINS];
  const select_view_t<Sel> w = select_view<Sel>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  for (uint32_t i = threadIdx.x; i < SLOTS * TIES_BINS; i += TIES_THREADS) lds[i] = 0;
  __syncthreads();
  // two named arrays, not p[RANKS][4]: the two-rank passes 1 and 2 then keep the registers they had (docs/experiments.md)
  uint32_t p0[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0}, p1[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        if (PASS > 0) {
#pragma unroll
          for (int m = 0; m < SLOTS; ++m)
            if (m < select_units<Sel>(w.jobs[cur])) {
              p0[m] = Sel::key(w.state[w.unit0[cur] + m], 0);
              if (Sel::RANKS > 1) p1[m] = Sel::key(w.state[w.unit0[cur] + m], 1);
            }
        }
      },
      [&](const typename Sel::job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          if constexpr (Sel::ELEM_KEY) {
            select_elem_hist_rule<Sel, PASS, S()> rule{p0[0], lds};
            chunk_stream<S(), true, false>(j, start4, rule);
          } else {
            select_hist_rule<Sel::RANKS, PASS, S()> rule{p0, p1, lds};
            chunk_stream<S(), true, false>(j, start4, rule);
          }
        });
      },
      [&](uint32_t cur) { select_flush<TOUCHED>(lds, w.hist + (uint64_t)w.unit0[cur] * TIES_BINS, select_units<Sel>(w.jobs[cur])); });
}

// One workgroup per unit: find, for every rank, the bin that holds the rank-th largest key, walking down from the top bin.
// Pass 0 walks the one histogram for all ranks, passes 1 and 2 walk each rank's own half.
template <class Sel, int PASS>
__global__ __launch_bounds__(TIES_THREADS) void vlm_select_scan_kernel(unsigned char* __restrict__ ws) {
  constexpr int R = Sel::RANKS;
  constexpr int PER = ties_bins<PASS>() / TIES_THREADS;  // bins per thread and histogram: 8 or 4
  constexpr int NH = PASS == 0 ? 1 : R;                  // histograms in a unit's slot
  __shared__ u64_t part[NH][TIES_THREADS];
  __shared__ u64_t sel_before[R];
  __shared__ int sel[R];
  const select_view_t<Sel> w = select_view<Sel>(ws);
  const uint32_t n_units = w.hdr->n_units;
  for (uint32_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    const ties_unit_t uj = w.units[unit];
    u64_t* h = w.hist + (uint64_t)unit * TIES_BINS;
    const typename Sel::state_t before = w.state[unit];
    u64_t rank[R];
    uint32_t prefix[R];
    bool none[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      rank[r] = PASS == 0 ? Sel::want(w.jobs[uj.job], uj.m, r) : Sel::rank(before, r);
      prefix[r] = PASS == 0 ? 0u : Sel::key(before, r);
      none[r] = Sel::none(w.jobs[uj.job], uj.m, r);
    }
    if (PASS == 0 && uj.m == 0 && threadIdx.x < Sel::COUNTERS)  // the counters of the job start every run at zero
      w.counters[(uint64_t)uj.job * Sel::COUNTERS + threadIdx.x] = 0;
    // thread t owns bins hi, hi-1, ..., hi-PER+1 of each histogram, hi = BINS-1 - t*PER: thread order is descending key order
    const int hi = (int)ties_bins<PASS>() - 1 - (int)threadIdx.x * PER;
    u64_t local[NH][PER];
#pragma unroll
    for (int g = 0; g < NH; ++g) {
      u64_t sum = 0;
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        local[g][q] = h[g * SELECT_HALF + hi - q];
        h[g * SELECT_HALF + hi - q] = 0;  // ready for the next pass and the next run
        sum += local[g][q];
      }
      part[g][threadIdx.x] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (threadIdx.x == 64u * r) {  // the first thread of wave r walks for rank r
        const int g = NH == 1 ? 0 : r;
        u64_t cum = 0;
        int t = 0;
        if (!none[r]) {  // no such rank: nothing is walked
          for (; t < TIES_THREADS - 1; ++t) {
            if (cum + part[g][t] >= rank[r]) break;
            cum += part[g][t];
          }
        }
        sel[r] = t;
        sel_before[r] = cum;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
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
        if (none[r]) {
          key = SELECT_NO_RANK;
          left = 0;
        }
        Sel::store(w.state[unit], r, key, left);
      }
    }
    __syncthreads();
  }
}

// fills every offset of `h` for n_jobs jobs, n_units (job, source) pairs and n_chunks chunks; returns the total size
template <class Sel>
static size_t select_layout(typename Sel::hdr_t* h, uint64_t n_jobs, uint64_t n_units, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(typename Sel::hdr_t));
  h->n_jobs = n_jobs;
  h->n_units = n_units;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(typename Sel::job_t));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  h->unit0_off = at.take(n_jobs * sizeof(uint32_t));
  h->units_off = at.take(n_units * sizeof(ties_unit_t));
  if constexpr (Sel::RECORD_DOUBLES > 0) h->first_off = at.take((n_jobs + 1) * sizeof(uint64_t));  // host-made: before the state
  h->state_off = at.take(n_units * sizeof(typename Sel::state_t));
  h->counters_off = at.take(n_jobs * Sel::COUNTERS * sizeof(uint64_t));
  h->hist_off = at.take(n_units * TIES_BINS * sizeof(uint64_t));
  if constexpr (Sel::RECORD_DOUBLES > 0) h->records_off = at.take(n_chunks * Sel::RECORD_DOUBLES * sizeof(double));
  return at.off;
}

template <class Sel>
static size_t select_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  // upper bounds: chunks_bound, and every job has at most VLM_MERGE_MAX_SRC sources (element-keyed: one unit)
  typename Sel::hdr_t h;
  return select_layout<Sel>(&h, (uint64_t)n_jobs, (uint64_t)n_jobs * select_slots<Sel>(), chunks_bound(n_jobs, total_elems));
}

template <class Sel>
static int select_plan_upload(const typename Sel::job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_chunks = 0, n_units = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const typename Sel::job_t& j = jobs[i];
    if (j.n_elem == 0 || !Sel::mode_ok(j)) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, true);
    if (rc != VLM_OK) return rc;
    for (int m = 0; m < select_units<Sel>(j); ++m)
      if (!Sel::ranks_ok(j, m)) return VLM_ERR_ARG;
    n_chunks += chunks_of(j.n_elem);
    n_units += (uint64_t)select_units<Sel>(j);
  }
  if (!chunk_count_ok(n_chunks) || n_units >= (1ull << 32)) return VLM_ERR_UNSUPPORTED;
  typename Sel::hdr_t hdr;
  const size_t total = select_layout<Sel>(&hdr, (uint64_t)n_jobs, n_units, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the state begins: state, counters and histograms are device-made
  std::vector<unsigned char> img = chunk_image(hdr, jobs, n_jobs, hdr.state_off);
  uint32_t* unit0 = reinterpret_cast<uint32_t*>(img.data() + hdr.unit0_off);
  ties_unit_t* units = reinterpret_cast<ties_unit_t*>(img.data() + hdr.units_off);
  if constexpr (Sel::RECORD_DOUBLES > 0) chunk_first_fill(jobs, n_jobs, reinterpret_cast<uint64_t*>(img.data() + hdr.first_off));
  uint64_t u = 0;
  for (int i = 0; i < n_jobs; ++i) {
    unit0[i] = (uint32_t)u;
    for (int m = 0; m < select_units<Sel>(jobs[i]); ++m) {
      units[u].job = (uint32_t)i;
      units[u].m = (uint32_t)m;
      ++u;
    }
  }
  // the histograms start at zero; every scan launch leaves them at zero again
  return chunk_upload(workspace, img, total - hdr.state_off, (hipStream_t)stream);
}

// The select itself: three histogram passes, a bin pick after each.  Six launches, stream-ordered.
template <class Sel>
static void select_launches(unsigned char* ws, hipStream_t s, dim3 hist_grid) {
  const dim3 block(TIES_THREADS), scan_grid(TIES_SCAN_BLOCKS);
  hipLaunchKernelGGL((vlm_select_hist_kernel<Sel, 0>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_select_scan_kernel<Sel, 0>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_select_hist_kernel<Sel, 1>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_select_scan_kernel<Sel, 1>), scan_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_select_hist_kernel<Sel, 2>), hist_grid, block, 0, s, ws);
  hipLaunchKernelGGL((vlm_select_scan_kernel<Sel, 2>), scan_grid, block, 0, s, ws);
}

// the select, then the method's apply pass: seven launches, no host synchronisation -- the sizes of the plan live in the workspace
// header
template <class Sel>
static int select_run(void* workspace, void* stream, void (*apply_kernel)(unsigned char*)) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  select_launches<Sel>(ws, s, chunk_grid(TIES_HIST_BLOCKS_PER_CU));
  hipLaunchKernelGGL(apply_kernel, chunk_grid(TIES_APPLY_BLOCKS_PER_CU), dim3(TIES_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
