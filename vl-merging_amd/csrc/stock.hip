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
// This file holds step 3, the apply rule and the workspace layout; the reducer's rule, its wave and workgroup folds and the fold
// of a job's records are gram_reduce.h's (sphere.hip reduces with them too); the walker, the run loop and the host checks are
// chunk_walk.h's and chunk_plan.h's, as in dare.hip and pairstats.hip.
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

struct stock_view_t {
  const vlm_stock_header_t* hdr;
  const vlm_stock_job_t* jobs;
  const chunk_t* chunks;
  const uint64_t* first;
  double* records;              // [n_chunks][STOCK_SUMS]
  vlm_stock_result_t* results;  // [n_jobs]
};

__device__ __forceinline__ stock_view_t stock_view(unsigned char* ws) {
  stock_view_t v;
  v.hdr = reinterpret_cast<const vlm_stock_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_stock_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.first = reinterpret_cast<const uint64_t*>(ws + v.hdr->first_off);
  v.records = reinterpret_cast<double*>(ws + v.hdr->records_off);
  v.results = reinterpret_cast<vlm_stock_result_t*>(ws + v.hdr->results_off);
  return v;
}

__global__ __launch_bounds__(STOCK_THREADS) void vlm_stock_reduce_kernel(unsigned char* __restrict__ ws) {
  // two buffers, used in turn: a chunk's wave sums are read behind ONE barrier while the next chunk's are written to the other
  __shared__ double red[2][STOCK_WAVES * STOCK_SUMS];
  const stock_view_t w = stock_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  uint64_t first = 0;
  int turn = 0;
  chunk_run(
      w.chunks, w.jobs, c0, c1, [&](uint32_t cur) { first = w.first[cur]; },
      [&](const vlm_stock_job_t& j, uint64_t start4) {
        double* r = red[turn];
        with_nsrc(j.n_src, [&](auto S) { stock_chunk<S()>(j, start4, r); });
        __syncthreads();
        stock_record(r, j.n_src, w.records, first, start4);  // ((w0 + w1) + w2) + w3 per sum, at the chunk's index
        turn ^= 1;
      },
      [&](uint32_t) {});
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
      STOCK_FOLD_RECORDS(sum, rec, c0, c1);  // a missing record adds +0.0: it changes no sum
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

// fills every offset of `h` for n_jobs jobs and n_chunks chunks; returns the total size
static size_t stock_layout(vlm_stock_header_t* h, uint64_t n_jobs, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(vlm_stock_header_t));
  h->n_jobs = n_jobs;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(vlm_stock_job_t));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  h->first_off = at.take((n_jobs + 1) * sizeof(uint64_t));
  h->records_off = at.take(n_chunks * STOCK_SUMS * sizeof(double));
  h->results_off = at.take(n_jobs * sizeof(vlm_stock_result_t));
  return at.off;
}

extern "C" size_t vlm_stock_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  vlm_stock_header_t h;
  return stock_layout(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems));
}

extern "C" int vlm_stock_plan_upload(const vlm_stock_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  std::vector<uint64_t> first((size_t)n_jobs + 1);
  uint64_t n_chunks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_stock_job_t& j = jobs[i];
    if (j.n_elem == 0) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, true);  // two passes read the inputs: dst may meet none of them
    if (rc != VLM_OK) return rc;
    first[i] = n_chunks;
    n_chunks += chunks_of(j.n_elem);
  }
  first[n_jobs] = n_chunks;
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  vlm_stock_header_t hdr;
  const size_t total = stock_layout(&hdr, (uint64_t)n_jobs, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the records begin: they and the results are device-made (every run overwrites all of them)
  std::vector<unsigned char> img = chunk_image(hdr, jobs, n_jobs, hdr.records_off);
  memcpy(img.data() + hdr.first_off, first.data(), first.size() * sizeof(uint64_t));
  return chunk_upload(workspace, img, 0, (hipStream_t)stream);
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
