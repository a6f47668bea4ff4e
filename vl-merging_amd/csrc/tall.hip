// Consensus merge with TALL masks (Wang et al., ICML 2024) over every output tensor of an all_moe -> ufo merge, and the reverse
// select that rebuilds one expert from the unified tensor, the central tensor and a packed mask.
// No reference site: the reference repository has neither.  The rule is written down in include/vlm_hip.h and restated in numpy
// by tests/tall_restatement.py; the kernel is held to that restatement bit for bit, mask words and padding bits included.
//
// The pass is the task-vector merge's traffic, 4 (S + 1) B read and 4 B written per element, plus S / 8 B of mask per element
// where a job asks for masks (RESTORE: 8 B + 1 / 8 B read, 4 B written).
//   vlm_tall_clear_kernel   a tiny launch: the counters of every job start the run at zero.
//   vlm_tall_apply_kernel   one launch over the plan's 16-KiB chunk table (chunk_plan.h), the shape of vlm_dare_apply_kernel: a
//                           workgroup owns a CONTIGUOUS run of chunks, 16-B non-temporal loads and stores (mask words: plain
//                           4-B stores, one per eight lanes), and the per-job
//                           counters flushed (64-bit integer atomics) when the run leaves a job.  Both ops, one kernel.
// The chunk body is this file's own, not chunk_stream: the mask words need the lanes of a wave to talk to each other, and
// chunk_stream computes under `if (idx < n4)`.  Here a float4 SLOT is walked by the whole workgroup: a lane whose float4 lies
// past the end computes nothing and contributes a zero nibble, and the eight lanes that hold one word's nibbles (tall_mask.h)
// fold them with three __shfl_xor steps that every lane of the wave executes.  The ragged tail is not a separate path of
// threads 0 .. 2: it is the partial float4 n4, handled by the ONE lane that stands at n4, so its bits enter the same fold as its
// neighbours' and the tensor's last word -- float4 lanes, tail bits, zero padding -- is written once, by one lane.  Where n4 lies
// just behind the tail chunk's last float4 the chunk walks a fifth slot for it (tall_has_tail_slot).
// Integer counters only, so nothing depends on the order workgroups run in.  -ffp-contract=off and __f*_rn: one rounding per
// operation, no FMA.  The run loop and the workspace's view are chunk_walk.h's, the counter plan (layout, upload, the two-launch
// run) and the family's host checks chunk_plan.h's, as in dare.hip.
#include "vlm_common.h"
#include "chunk_walk.h"  // the run loop, the source-count dispatch and the counters: the whole family's
#include "tall_mask.h"   // where an element's bit lives; the checks on a job's masks

#define TALL_THREADS CHUNK_THREADS
#define TALL_APPLY_BLOCKS_PER_CU 12   // vlm_dare_apply_kernel's rule; not A/B-measured against other values (docs/experiments.md, "Consensus merge")

static_assert(VLM_TALL_COUNTERS == VLM_TIES_COUNTERS, "tall.hip counts into chunk_walk.h's ties_counts_t");
#define TALL_SELECTED TIES_CONFLICT   // the slot behind kept[]: the elements with sel

// what a chunk does, a compile-time constant of its body
#define TALL_PLAIN 0     // CONSENSUS without masks
#define TALL_MASKS 1     // CONSENSUS, one mask per source written
#define TALL_RESTORE 2   // RESTORE: one mask read

typedef counts_view_t<vlm_tall_header_t, vlm_tall_job_t> tall_view_t;

// a job's scalars, workgroup-uniform
struct tall_param_t {
  int k;
  float tall_lambda, lam;
};

// Steps 1-5 for one element; bit m of `keep` = keep_m.
template <int NSRC>
__device__ __forceinline__ float tall_elem(float c, const float* wv, const tall_param_t& p, ties_counts_t& n, uint32_t& keep) {
  float x[NSRC];
  float d = 0.0f;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    x[m] = __fsub_rn(wv[m], c);                                          // step 1
    d = __fadd_rn(d, x[m]);                                              // step 2
  }
  int votes = 0;
  keep = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    const float r = __fsub_rn(d, x[m]);                                  // step 3
    const bool kept = fabsf(x[m]) >= __fmul_rn(p.tall_lambda, fabsf(r));
    keep |= (kept ? 1u : 0u) << m;
    n.c[m] += kept ? 1u : 0u;
    votes += kept ? 1 : 0;
  }
  const bool sel = votes >= p.k;                                         // step 4
  n.c[TALL_SELECTED] += sel ? 1u : 0u;
  n.c[TIES_EMPTY] += votes == 0 ? 1u : 0u;
  return __fadd_rn(c, __fmul_rn(p.lam, sel ? d : 0.0f));                 // step 5
}

// the restore rule for one element
__device__ __forceinline__ float tall_pick(bool bit, float u, float c, ties_counts_t& n) {
  n.c[0] += bit ? 1u : 0u;
  return bit ? u : c;
}

// One float4 slot of a chunk, entered by EVERY thread of the workgroup.  `have`: float4 idx lies inside the tensor and v (one
// float4 per source) and b (the base) hold it.  The lane with idx == n4 of a tensor with a ragged tail handles the tail's
// elements 4 n4 + t, t < tail, as the partial float4 it is.  Every other lane past the end does nothing but take part in the
// cross-lane steps, with zero bits.
template <int NSRC, int KIND>
__device__ __forceinline__ void tall_slot(const vlm_tall_job_t& j, uint64_t idx, uint64_t n4, uint32_t tail, uint64_t n_words,
                                          bool have, const f32x4* v, const f32x4& b, const tall_param_t& p, ties_counts_t& n) {
  const int lane = threadIdx.x & 63;
  const uint64_t word = tall_word_of(idx);
  const uint32_t shift = tall_shift_of(idx);   // == 4 (lane & 7): a chunk starts at a multiple of 8 float4s
  const bool leader = (lane & 7) == 0 && word < n_words;
  uint32_t nib[NSRC];                          // CONSENSUS: bit c of nib[m] = keep_m of element c of this float4
#pragma unroll
  for (int m = 0; m < NSRC; ++m) nib[m] = 0;
  if (KIND == TALL_RESTORE) {
    // the leader reads the word once for the 32 elements of its eight lanes -- and only a word the mask has
    uint32_t w = 0;
    if (leader) w = __builtin_nontemporal_load(&reinterpret_cast<const uint32_t*>(j.mask[0])[word]);
    w = __shfl(w, lane & ~7, 64);
    nib[0] = (w >> shift) & 15u;
  }
  const bool at_tail = !have && tail != 0 && idx == n4;
  if (have) {
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (KIND == TALL_RESTORE) {
        o[c] = tall_pick((nib[0] >> c) & 1u, v[0][c], b[c], n);
      } else {
        float w[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) w[m] = v[m][c];
        uint32_t keep;
        o[c] = tall_elem<NSRC>(b[c], w, p, n, keep);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((keep >> m) & 1u) << c;
      }
    }
    __builtin_nontemporal_store(o, &reinterpret_cast<f32x4*>(j.dst)[idx]);
  } else if (at_tail) {
    for (uint32_t t = 0; t < tail; ++t) {
      const uint64_t i = (n4 << 2) + t;  // < n_elem
      float w[NSRC];
#pragma unroll
      for (int m = 0; m < NSRC; ++m) w[m] = reinterpret_cast<const float*>(j.src[m])[i];
      const float bt = reinterpret_cast<const float*>(j.base)[i];
      float o;
      if (KIND == TALL_RESTORE) {
        o = tall_pick((nib[0] >> t) & 1u, w[0], bt, n);
      } else {
        uint32_t keep;
        o = tall_elem<NSRC>(bt, w, p, n, keep);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((keep >> m) & 1u) << t;
      }
      reinterpret_cast<float*>(j.dst)[i] = o;
    }
  }
  if (KIND == TALL_MASKS) {
    // step 6, the whole wave active: eight nibbles -> one word in every lane of the eight; the leader stores it.  A plain store,
    // not a non-temporal one: a wave's eight words are 32 B and the four waves of a workgroup fill one 128-B line between them,
    // which L2 puts together when the words may stay there; streamed past it they cost 9 % of the pass instead of 2 %
    // (docs/experiments.md, "Consensus merge").
#pragma unroll
    for (int m = 0; m < NSRC; ++m) {
      uint32_t w = nib[m] << shift;
      w |= __shfl_xor(w, 1, 64);
      w |= __shfl_xor(w, 2, 64);
      w |= __shfl_xor(w, 4, 64);
      if (leader) reinterpret_cast<uint32_t*>(j.mask[m])[word] = w;
    }
  }
}

// The chunk at start4 of job j: chunk_stream's loads (4 float4 per thread, strided by the block, all issued before the first
// use), then the slots.  No __restrict__: dst may be the base or a source exactly; every load of a float4 precedes its store.
template <int NSRC, int KIND>
__device__ __forceinline__ void tall_chunk(const vlm_tall_job_t& j, uint64_t start4, const tall_param_t& p, ties_counts_t& n) {
  const uint64_t n4 = j.n_elem >> 2, n_words = tall_mask_words(j.n_elem);
  const uint32_t tail = (uint32_t)(j.n_elem & 3);
  const f32x4* base = reinterpret_cast<const f32x4*>(j.base);
  const f32x4* s[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) s[m] = reinterpret_cast<const f32x4*>(j.src[m]);
  f32x4 v[4][NSRC];
  f32x4 b[4];
  uint64_t idx[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    idx[u] = start4 + threadIdx.x + u * CHUNK_THREADS;
    if (idx[u] < n4) {
#pragma unroll
      for (int m = 0; m < NSRC; ++m) v[u][m] = __builtin_nontemporal_load(&s[m][idx[u]]);
      b[u] = __builtin_nontemporal_load(&base[idx[u]]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) tall_slot<NSRC, KIND>(j, idx[u], n4, tail, n_words, idx[u] < n4, v[u], b[u], p, n);
  if (tall_has_tail_slot(start4, j.n_elem))  // workgroup-uniform
    tall_slot<NSRC, KIND>(j, start4 + CHUNK_FLOATS / 4 + threadIdx.x, n4, tail, n_words, false, v[0], b[0], p, n);
}

__global__ __launch_bounds__(TALL_THREADS) void vlm_tall_clear_kernel(unsigned char* __restrict__ ws) {
  const tall_view_t w = counts_view<vlm_tall_header_t, vlm_tall_job_t>(ws);
  chunk_clear_counts(w.counters, w.hdr->n_jobs * VLM_TALL_COUNTERS);
}

__global__ __launch_bounds__(TALL_THREADS) void vlm_tall_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ u64_t red[(TALL_THREADS / 64) * VLM_TALL_COUNTERS];
  const tall_view_t w = counts_view<vlm_tall_header_t, vlm_tall_job_t>(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_TALL_COUNTERS; ++k) n.c[k] = 0;
  tall_param_t p = {0, 0.0f, 0.0f};
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_tall_job_t& jn = w.jobs[cur];
        p.k = jn.k;
        p.tall_lambda = jn.tall_lambda;
        p.lam = jn.lam;
      },
      [&](const vlm_tall_job_t& j, uint64_t start4) {
        if (j.op == VLM_TALL_RESTORE) {
          tall_chunk<1, TALL_RESTORE>(j, start4, p, n);
        } else {
          with_nsrc(j.n_src, [&](auto S) {
            if (j.mask[0]) tall_chunk<S(), TALL_MASKS>(j, start4, p, n);
            else tall_chunk<S(), TALL_PLAIN>(j, start4, p, n);
          });
        }
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, red, w.counters + (uint64_t)cur * VLM_TALL_COUNTERS); });
}

extern "C" size_t vlm_tall_plan_bytes(int n_jobs, uint64_t total_elems) {
  return counts_plan_bytes<vlm_tall_header_t, vlm_tall_job_t>(n_jobs, total_elems, VLM_TALL_COUNTERS);
}

extern "C" int vlm_tall_plan_upload(const vlm_tall_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return counts_plan_upload<vlm_tall_header_t, VLM_TALL_COUNTERS>(jobs, n_jobs, workspace, workspace_bytes, stream, [](const vlm_tall_job_t& j) {
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);
    return rc == VLM_OK ? tall_job_check(j) : rc;
  });
}

extern "C" int vlm_tall_run(void* workspace, void* stream) {
  return counts_run(workspace, stream, vlm_tall_clear_kernel, vlm_tall_apply_kernel, chunk_grid(TALL_APPLY_BLOCKS_PER_CU));
}
