// Model Stock merge (Jang, Yun & Han, ECCV 2024) over every output tensor of an all_moe -> ufo merge: the angle between the
// experts' task vectors fixes, per tensor, how far their average is pulled back towards the central tensor.
// No reference site: the reference repository has no such merge.  The rule, INCLUDING the order of every floating-point sum, is
// written down in include/vlm_hip.h and restated in numpy and python doubles by tests/stock_restatement.py; the kernels are held
// to that restatement bit for bit.
//
// The first method of the family whose apply pass reads a scalar that a reduction over the same tensor makes on the device:
//   vlm_stock_reduce_kernel  one launch over the plan's chunk table (chunk_plan.h), dealt as vlm_pairstats_stream_kernel's.  Per
//                            chunk: sq[S] and dot[pairs] of the task vectors through chunk_stream<S, true, false>
//                            (chunk_walk.h) -- at most ten doubles per thread and no counts, so the pass is an HBM stream where
//                            the pair statistics are not --, the wave fold by halves, the four waves added in order, one 80-byte
//                            record written at the chunk's index.  The sums are vlm_pairstats_run's bytes.
//   vlm_stock_fold_kernel    one workgroup per job at a time, one thread per sum: the job's records added in chunk order; then
//                            one thread does step 3 in f64 and writes the job's whole vlm_stock_result_t.
//   vlm_stock_apply_kernel   the chunk table again, the shape of vlm_dare_apply_kernel: entering a job loads its `scale` from its
//                            result, steps 1 and 4 per element, 16-B non-temporal loads and stores.
// Three launches, ordered by the stream alone.  No atomics; every record and every result is overwritten by each run, so nothing
// is cleared.  -ffp-contract=off and the __f*_rn / __d*_rn forms: one rounding per operation, no FMA.
// This file holds step 3 and the apply rule; the reducer's rule is gram_reduce.h's (sphere.hip reduces with
// it too), its wave and workgroup folds, its run and the fold of a job's records chunk_records.h's; the walker and the run loop are
// chunk_walk.h's, the record plan (layout, upload; its view: chunk_records.h) and the host checks chunk_plan.h's, as in pairstats.hip.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "gram_reduce.h"

// Workgroups per CU of the reducer's grid (132 registers: three are resident, tests/test_stock_cpu.py watches the occupancy; forcing
// 128 for a fourth spills): measured at 8, 12, 16 and 24, docs/experiments.md, "Model Stock".
#define STOCK_REDUCE_BLOCKS_PER_CU 12
// The apply pass's: DARE's 12 per CU was timed against 24, 48 and 96; 96 (vlm_merge_kernel's value) is 5 % of a run faster.
#define STOCK_APPLY_BLOCKS_PER_CU 96

static_assert(STOCK_SUMS == 10 && sizeof(vlm_stock_result_t) == (STOCK_SUMS + STOCK_PAIRS + 2) * 8 + 8,
              "a result is the ten sums, six cosines, cos, t, scale and four reserved bytes");
static_assert(offsetof(vlm_stock_result_t, dot) == VLM_MERGE_MAX_SRC * 8, "a result begins as a record does");

// records: [n_chunks][STOCK_SUMS] doubles
typedef records_view_t<vlm_stock_header_t, vlm_stock_job_t, double, vlm_stock_result_t> stock_view_t;
__device__ __forceinline__ stock_view_t stock_view(unsigned char* ws) {
  return records_view<vlm_stock_header_t, vlm_stock_job_t, double, vlm_stock_result_t>(ws);
}

__global__ __launch_bounds__(STOCK_THREADS) void vlm_stock_reduce_kernel(unsigned char* __restrict__ ws) {
  const stock_view_t w = stock_view(ws);
  chunk_reduce_run<STOCK_SUMS>(
      w.chunks, w.jobs, w.hdr->n_chunks, w.first, w.records, [](uint32_t) {},
      [](const vlm_stock_job_t& j, uint64_t start4, double* r) { with_nsrc(j.n_src, [&](auto S) { stock_chunk<S()>(j, start4, r); }); },
      [](const vlm_stock_job_t& j, int k) { return stock_slot_used(k, j.n_src); });
}

// Step 3 for a job of S sources whose folded sums are s[0 .. STOCK_SUMS) (LDS): the whole result, written field by field (the
// loops have compile-time bounds, so nothing is indexed at run time and nothing lives in scratch).
__device__ __forceinline__ void stock_ratio(const double* s, int S, vlm_stock_result_t* out) {
#pragma unroll
  for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) out->sq[m] = s[m];
#pragma unroll
  for (int p = 0; p < STOCK_PAIRS; ++p) out->dot[p] = s[VLM_MERGE_MAX_SRC + p];
  double sum = 0.0;
#pragma unroll
  for (int b = 1; b < VLM_MERGE_MAX_SRC; ++b) {
#pragma unroll
    for (int a = 0; a < b; ++a) {  // p = b (b - 1) / 2 + a: the slots in order
      const int p = b * (b - 1) / 2 + a;
      double cp = 0.0;
      if (b < S) {
        const double den = __dsqrt_rn(__dmul_rn(s[a], s[b]));
        cp = den > 0.0 ? __ddiv_rn(s[VLM_MERGE_MAX_SRC + p], den) : 0.0;
        sum = __dadd_rn(sum, cp);
      }
      out->cos_pair[p] = cp;
    }
  }
  double cos = 0.0, t = 1.0;
  if (S > 1) {
    cos = __ddiv_rn(sum, (double)(S * (S - 1) / 2));
    const double cc = cos > 0.0 ? (cos < 1.0 ? cos : 1.0) : 0.0;
    t = __ddiv_rn(__dmul_rn((double)S, cc), __dadd_rn(1.0, __dmul_rn((double)(S - 1), cc)));
  }
  out->cos = cos;
  out->t = t;
  out->scale = __double2float_rn(__ddiv_rn(t, (double)S));
  out->reserved = 0;
}

__global__ __launch_bounds__(STOCK_FOLD_THREADS) void vlm_stock_fold_kernel(unsigned char* __restrict__ ws) {
  __shared__ double sums[STOCK_SUMS];
  const stock_view_t w = stock_view(ws);
  const int k = threadIdx.x;
  // a workgroup per job; the grid is fixed (the job count lives in the header, on the device), so it strides over the jobs
  for (uint64_t job = blockIdx.x; job < w.hdr->n_jobs; job += gridDim.x) {
    if (k < STOCK_SUMS) {
      const double* rec = w.records + k;
      const uint64_t c0 = w.first[job], c1 = w.first[job + 1];
      double sum = 0.0;
      CHUNK_FOLD_RECORDS(sum, rec, STOCK_SUMS, c0, c1);
      sums[k] = sum;
    }
    __syncthreads();
    if (k == 0) stock_ratio(sums, w.jobs[job].n_src, &w.results[job]);
    __syncthreads();  // the next job's sums overwrite these
  }
}

// Steps 1 and 4 as chunk_stream's rule.
template <int S>
struct stock_apply_rule {
  const float& scale;  // workgroup-uniform: the job's, loaded on entering it
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    float d = 0.0f;
#pragma unroll
    for (int m = 0; m < S; ++m) d = __fadd_rn(d, __fsub_rn(wv[m], c));
    return __fadd_rn(c, __fmul_rn(scale, d));
  }
};

__global__ __launch_bounds__(STOCK_THREADS) void vlm_stock_apply_kernel(unsigned char* __restrict__ ws) {
  const stock_view_t w = stock_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  float scale = 0.0f;
  chunk_run(
      w.chunks, w.jobs, c0, c1, [&](uint32_t cur) { scale = w.results[cur].scale; },
      [&](const vlm_stock_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          stock_apply_rule<S()> rule{scale};
          chunk_stream<S(), true, true>(j, start4, rule);
        });
      },
      [&](uint32_t) {});
}

extern "C" size_t vlm_stock_plan_bytes(int n_jobs, uint64_t total_elems) {
  return records_plan_bytes<vlm_stock_header_t, vlm_stock_job_t>(n_jobs, total_elems, STOCK_SUMS * sizeof(double), sizeof(vlm_stock_result_t));
}

extern "C" int vlm_stock_plan_upload(const vlm_stock_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return records_plan_upload<vlm_stock_header_t>(
      jobs, n_jobs, workspace, workspace_bytes, stream, STOCK_SUMS * sizeof(double), sizeof(vlm_stock_result_t),
      [](const vlm_stock_job_t& j) { return chunk_job_check(j, CHUNK_OVERLAP_NONE, true); });  // two passes read the inputs: dst may meet none of them
}

extern "C" int vlm_stock_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // three launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header, the scalars
  // the apply pass reads in the results the fold has written
  hipLaunchKernelGGL(vlm_stock_reduce_kernel, chunk_grid(STOCK_REDUCE_BLOCKS_PER_CU), dim3(STOCK_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_stock_fold_kernel, chunk_grid(1), dim3(STOCK_FOLD_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_stock_apply_kernel, chunk_grid(STOCK_APPLY_BLOCKS_PER_CU), dim3(STOCK_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
