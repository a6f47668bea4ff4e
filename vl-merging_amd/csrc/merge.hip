// Checkpoint-merge kernel (K12/K13/mean): one launch over every output tensor of an all_moe -> ufo merge.
// Reference: src/vilt/modules/vilt_module.py:533-638 (merge_weights), :640-746 (sum_task_vectors),
// :436-457 (regmean's bias / LayerNorm averages).
//
// Roofline: HBM-bound, 4 B written + 4*n_src B read per element, no reuse.  Work is cut into 16 KiB chunks
// (4096 floats) described by a device-resident table so that ONE grid covers all 168 tensors; each thread
// moves 16 B per access (global_load/store_dwordx4), all n_src loads of a 4-vector batch are issued before
// the first use.  Compiled with -ffp-contract=off and written with __fmul_rn/__fadd_rn so that no FMA is
// formed: the reference's CPU path rounds after the multiply and after every add (SURVEY.md 7 "hard parts").
// This file holds the three rules and the grid-stride kernel.  The streaming body of a chunk and the source-count dispatch are
// chunk_walk.h's; the chunk table, the per-job checks, the host image, the upload and the grid rule are chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"  // the chunk walker and the source-count dispatch, shared with ties.hip and dare.hip

struct merge_header_t {
  uint32_t n_jobs;
  uint32_t n_chunks;
  uint32_t jobs_off;    // byte offsets inside the workspace
  uint32_t chunks_off;
};

// The three rules, stated once: the vector body and the ragged tail both come here.  One rounding per operation, in this order.
template <int MODE, int NSRC>
__device__ __forceinline__ float merge_rule(const float* r, float base, const float* w) {
  float acc;
  if (MODE == VLM_MERGE_LERP) {
    acc = 0.0f;
#pragma unroll
    for (int m = 0; m < NSRC; ++m) acc = __fadd_rn(acc, __fmul_rn(r[m], w[m]));
  } else if (MODE == VLM_MERGE_TASKVEC) {
    acc = base;
#pragma unroll
    for (int m = 0; m < NSRC; ++m) acc = __fadd_rn(acc, __fmul_rn(r[m], __fsub_rn(w[m], acc)));
  } else {
    acc = 0.0f;
#pragma unroll
    for (int m = 0; m < NSRC; ++m) acc = __fadd_rn(acc, w[m]);
    acc = __fdiv_rn(acc, (float)NSRC);
  }
  return acc;
}

// merge_rule as chunk_stream's rule (chunk_walk.h): nothing to prepare per float4, the job's ratios in registers
template <int MODE, int NSRC>
struct merge_stream_rule {
  float r[NSRC];
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(chunk_no_prep, int, float base, const float* w) const {
    return merge_rule<MODE, NSRC>(r, base, w);
  }
};

// only a TASKVEC job has a base to load
template <int MODE>
__device__ __forceinline__ void merge_chunk_mode(const vlm_merge_job_t& j, uint64_t start4) {
  with_nsrc(j.n_src, [&](auto S) {
    merge_stream_rule<MODE, S()> rule;
#pragma unroll
    for (int m = 0; m < S(); ++m) rule.r[m] = j.ratio[m];
    chunk_stream<S(), MODE == VLM_MERGE_TASKVEC, true>(j, start4, rule);
  });
}

__global__ __launch_bounds__(CHUNK_THREADS) void vlm_merge_kernel(const unsigned char* __restrict__ ws) {
  const merge_header_t* hdr = reinterpret_cast<const merge_header_t*>(ws);
  const vlm_merge_job_t* jobs = reinterpret_cast<const vlm_merge_job_t*>(ws + hdr->jobs_off);
  const chunk_t* chunks = reinterpret_cast<const chunk_t*>(ws + hdr->chunks_off);
  const uint32_t n_chunks = hdr->n_chunks;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const chunk_t ck = chunks[c];
    const vlm_merge_job_t j = jobs[ck.job];  // block-uniform => scalar loads; a copy: what every variant reads is loaded before the dispatch
    const uint64_t start4 = ck.start4;
    if (j.mode == VLM_MERGE_LERP) merge_chunk_mode<VLM_MERGE_LERP>(j, start4);
    else if (j.mode == VLM_MERGE_TASKVEC) merge_chunk_mode<VLM_MERGE_TASKVEC>(j, start4);
    else merge_chunk_mode<VLM_MERGE_MEAN>(j, start4);
  }
}

// fills every offset of `h` for n_jobs jobs and n_chunks chunks; returns the total size
static size_t merge_layout(merge_header_t* h, uint64_t n_jobs, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(merge_header_t));
  h->n_jobs = (uint32_t)n_jobs;
  h->n_chunks = (uint32_t)n_chunks;
  h->jobs_off = (uint32_t)at.take(n_jobs * sizeof(vlm_merge_job_t));
  h->chunks_off = (uint32_t)at.take(n_chunks * sizeof(chunk_t));
  return at.off;
}

extern "C" size_t vlm_merge_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  merge_header_t h;
  return merge_layout(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems));
}

extern "C" int vlm_merge_plan_upload(const vlm_merge_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!jobs || n_jobs <= 0 || !workspace) return VLM_ERR_ARG;
  uint64_t n_chunks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_merge_job_t& j = jobs[i];
    if (j.mode < 0 || j.mode > VLM_MERGE_MEAN) return VLM_ERR_ARG;
    // pointers before the length; only a TASKVEC job needs its base
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_UNCHECKED, j.mode == VLM_MERGE_TASKVEC);
    if (rc != VLM_OK) return rc;
    n_chunks += chunks_of(j.n_elem);
  }
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  merge_header_t hdr;
  const size_t total = merge_layout(&hdr, (uint64_t)n_jobs, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  return chunk_upload(workspace, chunk_image(hdr, jobs, n_jobs, total), 0, (hipStream_t)stream);
}

extern "C" int vlm_merge_run(const void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  // 96 workgroups per CU (8 resident at a time) stride the chunk table: late-finishing workgroups do not hold a whole stride of
  // chunks back.  The sweep over grid size and cache policy is settled and recorded in docs/experiments.md ("Merge kernel: grid
  // and cache policy").
  hipLaunchKernelGGL(vlm_merge_kernel, chunk_grid(96), dim3(CHUNK_THREADS), 0, (hipStream_t)stream,
                     (const unsigned char*)workspace);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
