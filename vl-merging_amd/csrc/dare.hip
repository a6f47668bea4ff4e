// DARE merge (drop and rescale; Yu et al. 2023) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no DARE.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/dare_restatement.py; the kernel is held to that restatement bit for bit.
//
// The mask is never stored: the draw of (seed, stream, source, element) is one word of a Philox4x32-10 block (philox.h), and
// one block serves one float4 of one source.  So the pass is the task-vector merge's traffic, 4 (S + 1) B read and 4 B written
// per element, plus ten Philox rounds per float4 and source on the VALU.
//   vlm_dare_clear_kernel   a tiny launch: the counters of every job start the run at zero.
//   vlm_dare_apply_kernel   one launch over the plan's 16-KiB chunk table (chunk_plan.h), the shape of vlm_ties_apply_kernel:
//                           a workgroup owns a CONTIGUOUS run of chunks, 16-B non-temporal loads and stores, steps 1-5 of the
//                           rule, and the per-job counters flushed (64-bit integer atomics) when the run leaves a job.
// Steps 3-5 of VLM_DARE_TIES are ties_elem.h's, shared with ties.hip.  Integer counters only, so nothing depends on the order
// workgroups run in.  -ffp-contract=off and __f*_rn: one rounding per operation, no FMA.
#include "vlm_common.h"
#include "chunk_plan.h"
#include "philox.h"
#include "ties_elem.h"
#include <string.h>
#include <vector>

#define DARE_THREADS CHUNK_THREADS
#define DARE_FLUSH_CHUNKS (1u << 19)  // a thread counts at most 16 per chunk: 2^23 per thread, 2^29 in the 64-lane wave sum, between flushes (32-bit)
#define DARE_APPLY_BLOCKS_PER_CU 12   // vlm_ties_apply_kernel's rule; not A/B-measured against other values (docs/experiments.md, "DARE merge")

static_assert(VLM_DARE_COUNTERS == VLM_TIES_COUNTERS, "dare.hip flushes its counters with ties_elem.h's ties_flush_counts");

struct dare_view_t {
  const vlm_dare_header_t* hdr;
  const vlm_dare_job_t* jobs;
  const chunk_t* chunks;
  u64_t* counters;
};

__device__ __forceinline__ dare_view_t dare_view(unsigned char* ws) {
  dare_view_t v;
  v.hdr = reinterpret_cast<const vlm_dare_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_dare_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

// what a job's scalars come to, workgroup-uniform
struct dare_param_t {
  uint64_t seed;       // the Philox key
  uint32_t stream;
  uint32_t below;      // keep_below's low word
  bool keep_all;       // keep_below == 2^32
  float rescale, lam;
};

// steps 1 and 3-5 for one element whose draws are u[0 .. NSRC)
template <int NSRC, int MODE>
__device__ __forceinline__ float dare_elem(float c, const float* wv, const uint32_t* u, const dare_param_t& p, ties_counts_t& n) {
  float tt[NSRC];
  int any = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float t = __fsub_rn(wv[m], c);                                 // step 1
    const bool kept = p.keep_all || u[m] < p.below;                      // step 3: (uint64) u < keep_below
    tt[m] = kept ? __fmul_rn(t, p.rescale) : 0.0f;
    n.c[m] += kept ? 1u : 0u;
    any += kept ? 1 : 0;
  }
  if (MODE == VLM_DARE_TIES) return ties_elect<NSRC>(c, tt, p.lam, n);   // steps 4-5: the TIES rule's 3-5 (ties_elem.h)
  float d = 0.0f;
  bool has_pos = false, has_neg = false;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {                                       // step 4, LINEAR
    d = __fadd_rn(d, tt[m]);
    has_pos |= tt[m] > 0.0f;
    has_neg |= tt[m] < 0.0f;
  }
  n.c[VLM_MERGE_MAX_SRC] += (has_pos && has_neg) ? 1u : 0u;
  n.c[VLM_MERGE_MAX_SRC + 1] += any == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(p.lam, d));                              // step 5
}

template <int NSRC, int MODE>
__device__ __forceinline__ void dare_apply_vec(const vlm_dare_job_t& j, const dare_param_t& p, uint64_t start4, uint64_t n4,
                                               ties_counts_t& n) {
  // no __restrict__: dst may be base or a source exactly.  Every load of a float4 precedes its store in program order.
  f32x4* dst = reinterpret_cast<f32x4*>(j.dst);
  const f32x4* base = reinterpret_cast<const f32x4*>(j.base);
  const f32x4* s[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) s[m] = reinterpret_cast<const f32x4*>(j.src[m]);
  f32x4 v[4][NSRC];
  f32x4 b[4];
  uint64_t idx[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    idx[u] = start4 + threadIdx.x + u * DARE_THREADS;
    if (idx[u] < n4) {
#pragma unroll
      for (int m = 0; m < NSRC; ++m) v[u][m] = __builtin_nontemporal_load(&s[m][idx[u]]);
      b[u] = __builtin_nontemporal_load(&base[idx[u]]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (idx[u] < n4) {
      philox4_t r[NSRC];  // step 2: one block per float4 and source, computed while the loads are in flight
#pragma unroll
      for (int m = 0; m < NSRC; ++m) r[m] = dare_draw4(p.seed, p.stream, (uint32_t)m, (uint32_t)idx[u]);
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float wv[NSRC];
        uint32_t uu[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) {
          wv[m] = v[u][m][c];
          uu[m] = r[m].w[c];
        }
        o[c] = dare_elem<NSRC, MODE>(b[u][c], wv, uu, p, n);
      }
      __builtin_nontemporal_store(o, &dst[idx[u]]);
    }
  }
}

// element i = 4 n4 + t of the ragged end: word t of the block of float4 n4
template <int NSRC, int MODE>
__device__ __forceinline__ void dare_apply_tail(const vlm_dare_job_t& j, const dare_param_t& p, uint64_t n4, uint32_t t,
                                                ties_counts_t& n) {
  const uint64_t i = (n4 << 2) + t;
  float wv[NSRC];
  uint32_t uu[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    wv[m] = reinterpret_cast<const float*>(j.src[m])[i];
    const philox4_t r = dare_draw4(p.seed, p.stream, (uint32_t)m, (uint32_t)n4);
    uu[m] = t == 0 ? r.w[0] : (t == 1 ? r.w[1] : r.w[2]);  // t < 4 and t < n_elem % 4 <= 3
  }
  const float c = reinterpret_cast<const float*>(j.base)[i];
  reinterpret_cast<float*>(j.dst)[i] = dare_elem<NSRC, MODE>(c, wv, uu, p, n);
}

template <int NSRC, int MODE>
__device__ __forceinline__ void dare_chunk(const vlm_dare_job_t& j, const dare_param_t& p, uint64_t start4, ties_counts_t& n) {
  const uint64_t n4 = j.n_elem >> 2;
  dare_apply_vec<NSRC, MODE>(j, p, start4, n4, n);
  if (threadIdx.x < chunk_tail_len(start4, j.n_elem)) dare_apply_tail<NSRC, MODE>(j, p, n4, threadIdx.x, n);
}

__global__ __launch_bounds__(DARE_THREADS) void vlm_dare_clear_kernel(unsigned char* __restrict__ ws) {
  const dare_view_t w = dare_view(ws);
  const uint64_t total = w.hdr->n_jobs * VLM_DARE_COUNTERS;
  for (uint64_t i = (uint64_t)blockIdx.x * DARE_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * DARE_THREADS)
    w.counters[i] = 0;
}

__global__ __launch_bounds__(DARE_THREADS) void vlm_dare_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(DARE_THREADS / 64) * VLM_DARE_COUNTERS];
  const dare_view_t w = dare_view(ws);
  uint64_t c0, c1;
  ties_my_chunks(w.hdr->n_chunks, &c0, &c1);
  if (c0 >= c1) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_DARE_COUNTERS; ++k) n.c[k] = 0;
  uint32_t cur = 0xffffffffu, since = 0;
  dare_param_t p = {0, 0, 0, false, 1.0f, 0.0f};
  for (uint64_t c = c0; c < c1; ++c) {
    const chunk_t ck = w.chunks[c];  // block-uniform => scalar loads
    if (ck.job != cur || since >= DARE_FLUSH_CHUNKS) {
      if (cur != 0xffffffffu) ties_flush_counts(n, red, w.counters + (uint64_t)cur * VLM_DARE_COUNTERS);
      cur = ck.job;
      since = 0;
      const vlm_dare_job_t& jn = w.jobs[cur];
      p.seed = jn.seed;
      p.stream = jn.stream;
      p.below = (uint32_t)jn.keep_below;
      p.keep_all = (jn.keep_below >> 32) != 0;
      p.rescale = jn.rescale;
      p.lam = jn.lam;
    }
    ++since;
    const vlm_dare_job_t& j = w.jobs[cur];
    const uint64_t start4 = ck.start4;
    if (j.mode == VLM_DARE_TIES) {
      switch (j.n_src) {
        case 1: dare_chunk<1, VLM_DARE_TIES>(j, p, start4, n); break;
        case 2: dare_chunk<2, VLM_DARE_TIES>(j, p, start4, n); break;
        case 3: dare_chunk<3, VLM_DARE_TIES>(j, p, start4, n); break;
        default: dare_chunk<4, VLM_DARE_TIES>(j, p, start4, n); break;
      }
    } else {
      switch (j.n_src) {
        case 1: dare_chunk<1, VLM_DARE_LINEAR>(j, p, start4, n); break;
        case 2: dare_chunk<2, VLM_DARE_LINEAR>(j, p, start4, n); break;
        case 3: dare_chunk<3, VLM_DARE_LINEAR>(j, p, start4, n); break;
        default: dare_chunk<4, VLM_DARE_LINEAR>(j, p, start4, n); break;
      }
    }
  }
  ties_flush_counts(n, red, w.counters + (uint64_t)cur * VLM_DARE_COUNTERS);
}

// fills every offset of `h` for n_jobs jobs and n_chunks chunks; returns the total size
static size_t dare_layout(vlm_dare_header_t* h, uint64_t n_jobs, uint64_t n_chunks) {
  h->n_jobs = n_jobs;
  h->n_chunks = n_chunks;
  size_t off = chunk_align_up(sizeof(vlm_dare_header_t), 256);
  h->jobs_off = off;     off += chunk_align_up(n_jobs * sizeof(vlm_dare_job_t), 256);
  h->chunks_off = off;   off += chunk_align_up(n_chunks * sizeof(chunk_t), 256);
  h->counters_off = off; off += chunk_align_up(n_jobs * VLM_DARE_COUNTERS * sizeof(uint64_t), 256);
  return off;
}

extern "C" size_t vlm_dare_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  vlm_dare_header_t h;
  return dare_layout(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems));
}

// dst against one input: exactly the same range is fine (the pass is elementwise), any other meeting of the byte ranges
// [a, a + 4 n) and [b, b + 4 n) is not
static bool dare_partial_overlap(const void* a, const void* b, uint64_t n_elem) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  if (x == y) return false;
  const uint64_t bytes = n_elem * 4;
  return x < y ? (y - x) < bytes : (x - y) < bytes;
}

extern "C" int vlm_dare_plan_upload(const vlm_dare_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_chunks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_dare_job_t& j = jobs[i];
    if (j.n_src < 1 || j.n_src > VLM_MERGE_MAX_SRC || !j.dst || !j.base || j.n_elem == 0) return VLM_ERR_ARG;
    if (j.mode != VLM_DARE_LINEAR && j.mode != VLM_DARE_TIES) return VLM_ERR_ARG;
    if (j.keep_below < 1 || j.keep_below > (1ull << 32)) return VLM_ERR_ARG;
    if (!chunk_len_ok(j.n_elem)) return VLM_ERR_UNSUPPORTED;  // before the byte ranges are formed
    if (!chunk_ptr_ok(j.dst) || !chunk_ptr_ok(j.base) || dare_partial_overlap(j.dst, j.base, j.n_elem)) return VLM_ERR_ARG;
    for (int m = 0; m < j.n_src; ++m)
      if (!chunk_ptr_ok(j.src[m]) || dare_partial_overlap(j.dst, j.src[m], j.n_elem)) return VLM_ERR_ARG;
    n_chunks += chunks_of(j.n_elem);
  }
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  vlm_dare_header_t hdr;
  const size_t total = dare_layout(&hdr, (uint64_t)n_jobs, n_chunks);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the counters begin: they are device-made (every run zeroes them first)
  const size_t img_bytes = hdr.counters_off;
  std::vector<unsigned char> img(img_bytes, 0);
  memcpy(img.data(), &hdr, sizeof(hdr));
  memcpy(img.data() + hdr.jobs_off, jobs, (size_t)n_jobs * sizeof(vlm_dare_job_t));
  chunk_table_fill(reinterpret_cast<chunk_t*>(img.data() + hdr.chunks_off), jobs, n_jobs);
  return chunk_upload(workspace, img.data(), img_bytes, (hipStream_t)stream);
}

extern "C" int vlm_dare_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  int cus = vlm_device_cus();
  if (cus <= 0) cus = 256;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // two launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL(vlm_dare_clear_kernel, dim3(64), dim3(DARE_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_dare_apply_kernel, dim3(cus * DARE_APPLY_BLOCKS_PER_CU), dim3(DARE_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
