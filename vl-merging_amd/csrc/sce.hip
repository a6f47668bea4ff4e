// SCE merge (select, calculate, erase; Wan et al. 2024, "FuseChat"; mergekit's `sce`) over every output tensor of an all_moe -> ufo
// merge: keep the elements where the experts' task vectors differ most, weight each expert by the energy of its kept entries, drop
// the entries whose sign loses the election, take the weighted mean of the rest.
// No reference site: the reference repository has no such merge.  The rule, INCLUDING the order of every floating-point sum, is
// written down in include/vlm_hip.h and restated in numpy and python doubles by tests/sce_restatement.py; the kernels are held to
// that restatement bit for bit.
//
// The first method of the family that chains a select into a reduction into an apply pass, ordered by the stream alone:
//   vlm_select_hist_kernel<sce_sel, PASS>  ties_select.h's radix select with ONE unit per job and an ELEMENT key: key(var) of the
//   vlm_select_scan_kernel<sce_sel, PASS>  element's task vectors (steps 1-3), one 2048-bin histogram per workgroup (8 KiB of LDS)
//   vlm_sce_reduce_kernel   the chunk table again, the shape of vlm_stock_reduce_kernel: entering a job loads its threshold; per
//                           chunk sq[S] of the SELECTED entries in f64 (step 4), the wave fold by halves, the four waves added
//                           in order, one 32-byte record written at the chunk's index.  No atomics.
//   vlm_sce_fold_kernel     one workgroup per job at a time, one lane per source: the job's records added in chunk order; then
//                           lane 0 does step 5 in f64 and writes sq, tot and w[] beside the threshold: the job's whole result.
//   vlm_sce_apply_kernel    the chunk table once more: entering a job loads thr and w[]; steps 1-3 recomputed, steps 6-7, 16-B
//                           non-temporal loads and stores, the three counters flushed with chunk_flush_counts.
// Nine launches.  var and sel are recomputed by the reducer and the apply pass (nothing per element is stored between passes), so
// a run streams the inputs FIVE times, 4 (S + 1) B per element and pass, and writes 4 B per element once: that is the bound.
// -ffp-contract=off and the __f*_rn / __d*_rn forms: one rounding per operation, no FMA.
// This file holds what is SCE's own: what the select needs to know of its job and state (sce_sel), the variance key, the three
// kernels and the run.  The select, its six launches, the workspace layout and the upload are ties_select.h's (shared with ties.hip
// and band.hip); the reducer's wave and workgroup folds, its run and the fold of a job's records are chunk_records.h's (shared with
// stock.hip and sphere.hip); the chunk walker, the run loop and the counter flush are chunk_walk.h's; the chunk table, the family's
// per-job checks, the host image, the upload and the grid rule are chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "chunk_records.h"
#include "ties_select.h"

#define SCE_THREADS CHUNK_THREADS
#define SCE_WAVES (SCE_THREADS / 64)
#define SCE_SUMS VLM_MERGE_MAX_SRC  // a record: sq[4]
#define SCE_FOLD_THREADS 64         // lanes 0 .. 3 add one sum each; lane 0 then does step 5
// Workgroups per CU of the three grids.  Each starts from the kernel's resident-workgroup count as the build records it
// (tests/test_sce_cpu.py watches the registers and the LDS these counts assume) times a whole number of rounds, and each was then timed
// against its neighbours at base size, two alternating rounds in one visit (docs/experiments.md, "SCE merge"; a run is 1.057 ms):
//   histogram passes: 110 / 120 / 120 VGPRs (the 4 (S + 1) float4 a thread has in flight): FOUR workgroups (one wave per SIMD
//                     each) are resident per CU, as for the per-source passes of TIES.  The one histogram a workgroup holds takes
//                     8 KiB of LDS where theirs take 32, but the registers, not the LDS, bound the residency: it is not raised.
//                     One round.  Timed: 4 (kept) against 8 (+1.4 % of a run) and 12 (+1.8 %).
//   reducer:          114 VGPRs: four resident, three rounds (vlm_stock_reduce_kernel's 12 per CU).  Timed: 12 (kept) against 8
//                     (+0.7 %) and 24 (+0.2 %).
//   apply pass:       140 VGPRs: three resident, four rounds (TIES_APPLY_BLOCKS_PER_CU: the pass keeps counters as the TIES apply
//                     pass does, so a workgroup owns a run of chunks long enough to amortise its flush).  Timed: 12 (kept) against
//                     24 (-0.5 %: inside what two visits differ by, so the family's value stays) and 96 (+1.1 %).
#define SCE_HIST_BLOCKS_PER_CU 4
#define SCE_REDUCE_BLOCKS_PER_CU 12
#define SCE_APPLY_BLOCKS_PER_CU 12

static_assert(sizeof(vlm_sce_result_t) == 16 + (SCE_SUMS + 1) * 8 + SCE_SUMS * 4, "a result is the select's state, sq[4], tot and w[4]");
static_assert(sizeof(vlm_sce_header_t) == sizeof(vlm_ties_header_t) + 16 && offsetof(vlm_sce_header_t, hist_off) == offsetof(vlm_ties_header_t, hist_off),
              "the header is the select's, then first_off and records_off");

// Steps 1-2 for one element of a job of S sources: fills x[] and returns var.
template <int S>
__device__ __forceinline__ float sce_var(float c, const float* wv, float* x) {
  float sum = 0.0f;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    x[m] = __fsub_rn(wv[m], c);                                          // step 1
    sum = __fadd_rn(sum, x[m]);
  }
  const float mean = __fdiv_rn(sum, (float)S);                           // step 2
  float q = 0.0f;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const float e = __fsub_rn(x[m], mean);
    q = __fadd_rn(q, __fmul_rn(e, e));
  }
  return __fdiv_rn(q, (float)S);
}

struct sce_sel {
  typedef vlm_sce_job_t job_t;
  typedef vlm_sce_header_t hdr_t;
  typedef vlm_sce_result_t state_t;  // a job's selection state is the head of its result
  static constexpr int RANKS = 1, COUNTERS = VLM_SCE_COUNTERS, RECORD_DOUBLES = SCE_SUMS;
  static constexpr bool ELEM_KEY = true;  // one unit per job
  template <int S>
  static __device__ __forceinline__ uint32_t elem_key(float c, const float* wv) {
    float x[S];
    return __float_as_uint(sce_var<S>(c, wv, x)) & 0x7fffffffu;
  }
  static __device__ __forceinline__ u64_t want(const job_t& j, uint32_t, int) { return j.k; }
  static __device__ __forceinline__ bool none(const job_t&, uint32_t, int) { return false; }
  static __device__ __forceinline__ uint32_t key(const state_t& s, int) { return s.key; }
  static __device__ __forceinline__ u64_t rank(const state_t& s, int) { return s.rank; }
  static __device__ __forceinline__ void store(state_t& s, int, uint32_t key, u64_t left) {  // sq, tot and w are the fold's
    s.key = key;
    s.reserved = 0;
    s.rank = left;
  }
  static bool mode_ok(const job_t&) { return true; }
  static bool ranks_ok(const job_t& j, int) { return j.k >= 1 && j.k <= j.n_elem; }
};

struct sce_view_t {
  select_view_t<sce_sel> s;
  const uint64_t* first;
  double* records;  // [n_chunks][SCE_SUMS]
};

__device__ __forceinline__ sce_view_t sce_view(unsigned char* ws) {
  sce_view_t v;
  v.s = select_view<sce_sel>(ws);
  v.first = reinterpret_cast<const uint64_t*>(ws + v.s.hdr->first_off);
  v.records = reinterpret_cast<double*>(ws + v.s.hdr->records_off);
  return v;
}

// Steps 1-4 as chunk_stream's rule: elem() adds one element to the thread's sums and returns nothing worth storing.
template <int S>
struct sce_reduce_rule {
  const uint32_t& thr;  // workgroup-uniform: the job's, loaded on entering it
  double* sq;           // the thread's S sums
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    float x[S];
    const bool sel = (__float_as_uint(sce_var<S>(c, wv, x)) & 0x7fffffffu) >= thr;  // step 3
#pragma unroll
    for (int m = 0; m < S; ++m) {
      const double xd = (double)x[m];
      sq[m] = __dadd_rn(sq[m], sel ? __dmul_rn(xd, xd) : 0.0);           // step 4
    }
    return 0.0f;
  }
};

// one chunk's sums, then their wave sums into red[wave][m] (lane 0 writes)
template <int S>
__device__ __forceinline__ void sce_chunk(const vlm_sce_job_t& j, uint64_t start4, const uint32_t& thr, double* red) {
  double sq[S];
#pragma unroll
  for (int m = 0; m < S; ++m) sq[m] = 0.0;
  sce_reduce_rule<S> rule{thr, sq};
  chunk_stream<S, true, false>(j, start4, rule);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const double v = chunk_wave_sum(sq[m]);
    if (lane == 0) red[wave * SCE_SUMS + m] = v;
  }
}

__global__ __launch_bounds__(SCE_THREADS) void vlm_sce_reduce_kernel(unsigned char* __restrict__ ws) {
  const sce_view_t w = sce_view(ws);
  uint32_t thr = 0;  // the job's threshold, loaded on entering it
  chunk_reduce_run<SCE_SUMS>(
      w.s.chunks, w.s.jobs, w.s.hdr->n_chunks, w.first, w.records, [&](uint32_t cur) { thr = w.s.state[w.s.unit0[cur]].key; },
      [&](const vlm_sce_job_t& j, uint64_t start4, double* r) { with_nsrc(j.n_src, [&](auto S) { sce_chunk<S()>(j, start4, thr, r); }); },
      [](const vlm_sce_job_t& j, int k) { return k < j.n_src; });
}

__global__ __launch_bounds__(SCE_FOLD_THREADS) void vlm_sce_fold_kernel(unsigned char* __restrict__ ws) {
  __shared__ double sums[SCE_SUMS];
  const sce_view_t w = sce_view(ws);
  const int k = threadIdx.x;
  // a workgroup per job; the grid is fixed (the job count lives in the header, on the device), so it strides over the jobs
  for (uint64_t job = blockIdx.x; job < w.s.hdr->n_jobs; job += gridDim.x) {
    if (k < SCE_SUMS) {
      const double* rec = w.records + k;
      const uint64_t c0 = w.first[job], c1 = w.first[job + 1];
      double sum = 0.0;
      CHUNK_FOLD_RECORDS(sum, rec, SCE_SUMS, c0, c1);
      sums[k] = sum;
    }
    __syncthreads();
    if (k == 0) {  // step 5; the loops have compile-time bounds, so nothing is indexed at run time
      const int S = w.s.jobs[job].n_src;
      vlm_sce_result_t* out = &w.s.state[w.s.unit0[job]];
      double tot = 0.0;
#pragma unroll
      for (int m = 0; m < SCE_SUMS; ++m)
        if (m < S) tot = __dadd_rn(tot, sums[m]);
      const bool some = tot > 0.0;
      const float uniform = __double2float_rn(__ddiv_rn(1.0, (double)S));
#pragma unroll
      for (int m = 0; m < SCE_SUMS; ++m) {
        out->sq[m] = sums[m];
        out->w[m] = m < S ? (some ? __double2float_rn(__ddiv_rn(sums[m], tot)) : uniform) : 0.0f;
      }
      out->tot = tot;
    }
    __syncthreads();  // the next job's sums overwrite these
  }
}

struct sce_counts_t {
  uint32_t c[VLM_SCE_COUNTERS];  // kept, conflict, empty
};
#define SCE_KEPT 0
#define SCE_CONFLICT 1
#define SCE_EMPTY 2

// Steps 1-3 and 6-7 as chunk_stream's rule.
template <int S>
struct sce_apply_rule {
  const uint32_t& thr;  // workgroup-uniform: the job's, loaded on entering it
  const float* wgt;     // likewise: w[0 .. 4)
  float lam;
  sce_counts_t& n;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    float x[S], tt[S];
    const bool sel = (__float_as_uint(sce_var<S>(c, wv, x)) & 0x7fffffffu) >= thr;  // steps 1-3
    float s = 0.0f;
    bool has_pos = false, has_neg = false;
#pragma unroll
    for (int m = 0; m < S; ++m) {                                        // step 6
      tt[m] = sel ? x[m] : 0.0f;
      s = __fadd_rn(s, tt[m]);
      has_pos |= tt[m] > 0.0f;
      has_neg |= tt[m] < 0.0f;
    }
    float num = 0.0f, den = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int m = 0; m < S; ++m) {
      const bool agree = (s > 0.0f && tt[m] > 0.0f) || (s < 0.0f && tt[m] < 0.0f);
      if (agree) {
        num = __fadd_rn(num, __fmul_rn(wgt[m], tt[m]));
        den = __fadd_rn(den, wgt[m]);
        ++cnt;
      }
    }
    const float d = den > 0.0f ? __fdiv_rn(num, den) : 0.0f;
    n.c[SCE_KEPT] += sel ? 1u : 0u;
    n.c[SCE_CONFLICT] += (has_pos && has_neg) ? 1u : 0u;
    n.c[SCE_EMPTY] += cnt == 0 ? 1u : 0u;
    return __fadd_rn(c, __fmul_rn(lam, d));                              // step 7
  }
};

__global__ __launch_bounds__(SCE_THREADS) void vlm_sce_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[SCE_WAVES * VLM_SCE_COUNTERS];
  const select_view_t<sce_sel> w = select_view<sce_sel>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  sce_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_SCE_COUNTERS; ++k) n.c[k] = 0;
  uint32_t thr = 0;
  float wgt[VLM_MERGE_MAX_SRC] = {0.0f, 0.0f, 0.0f, 0.0f};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_sce_result_t& r = w.state[w.unit0[cur]];
        thr = r.key;
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) wgt[m] = r.w[m];
      },
      [&](const vlm_sce_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          sce_apply_rule<S()> rule{thr, wgt, j.lam, n};
          chunk_stream<S(), true, true>(j, start4, rule);
        });
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_SCE_COUNTERS); });
}

extern "C" size_t vlm_sce_plan_bytes(int n_jobs, uint64_t total_elems) { return select_plan_bytes<sce_sel>(n_jobs, total_elems); }

extern "C" int vlm_sce_plan_upload(const vlm_sce_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream) {
  return select_plan_upload<sce_sel>(jobs, n_jobs, workspace, workspace_bytes, stream);
}

extern "C" int vlm_sce_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // nine launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header, the threshold the
  // reducer reads in the state the last bin pick has written, the weights the apply pass reads in the result the fold has written
  const dim3 block(SCE_THREADS);
  select_launches<sce_sel>(ws, s, chunk_grid(SCE_HIST_BLOCKS_PER_CU));
  hipLaunchKernelGGL(vlm_sce_reduce_kernel, chunk_grid(SCE_REDUCE_BLOCKS_PER_CU), block, 0, s, ws);
  hipLaunchKernelGGL(vlm_sce_fold_kernel, chunk_grid(1), dim3(SCE_FOLD_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_sce_apply_kernel, chunk_grid(SCE_APPLY_BLOCKS_PER_CU), block, 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
