// EMR-Merging (Huang et al., NeurIPS 2024: elect, mask and rescale) over every output tensor of an all_moe -> ufo merge, and the
// way back: one expert rebuilt from the unified tensor, the central tensor, a packed mask and one scalar.
// No reference site: the reference repository has neither.  The rule, INCLUDING the order of every floating-point sum, is written
// down in include/vlm_hip.h and restated in numpy by tests/emr_restatement.py; the kernels are held to that restatement bit for
// bit, mask words, padding bits, sums and rescalers included.
//
// The pass is the consensus merge's traffic with masks on, 4 (S + 1) B read, 4 B written and S / 8 B of mask per element
// (RESTORE: 8 B + 1 / 8 B read, 4 B written), plus one 112-B record per 16-KiB chunk.
//   vlm_emr_pass_kernel   one launch over the plan's chunk table through chunk_reduce_run (chunk_records.h).  The chunk body has
//                         tall.hip's shape -- every thread of the workgroup enters every float4 slot, 16-B non-temporal loads and
//                         stores, the eight nibbles of a mask word folded with three __shfl_xor steps and stored by the group
//                         leader with a plain 4-B store, the ragged tail handled by the ONE lane that stands at the partial float4
//                         -- and it also gathers, per thread, the f64 addends of step 6 and the counts; their wave sums go to
//                         chunk_record, which leaves one record at the chunk's index.  Both ops, one kernel.
//   vlm_emr_fold_kernel   one workgroup per job at a time, one thread per slot: the job's records added in chunk order
//                         (CHUNK_FOLD_RECORDS); then one thread does step 7 and writes the job's whole vlm_emr_result_t.
// Two launches, ordered by the stream alone.  No atomics; every record and every result is overwritten by each run, so nothing is
// cleared.  -ffp-contract=off and the __f*_rn / __d*_rn forms: one rounding per operation, no FMA.
// A record is 14 doubles: a[4], b[4], then the counts kept[4], zero, conflict AS DOUBLES -- a chunk counts at most 4099 per slot and
// sums of integers stay exact below 2^53, far above the family's length limit of 2^34 elements, so the shared record writer and
// fold (which add doubles) serve the counts unchanged.
// Registers and LDS (the compiler's resource-usage remarks for gfx950, vlm_emr_pass_kernel, which holds every instantiation up to
// S = 4 with masks on): see the figures behind EMR_BLOCKS_PER_CU below; no scratch.  LDS: the two record buffers of
// chunk_reduce_run, 2 x 4 waves x 14 doubles = 896 B.
// The run loop, the record writer and the fold are chunk_records.h's, the walker chunk_walk.h's, the record plan (layout, upload)
// and the host checks chunk_plan.h's, the place of a bit and the checks on a job's masks tall_mask.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "chunk_records.h"
#include "tall_mask.h"

#define EMR_THREADS CHUNK_THREADS
#define EMR_FOLD_THREADS 64   // lanes 0 .. 13 add one slot each; lane 0 then does step 7
// tall.hip's value, INHERITED: not A/B-measured against other values for this kernel (docs/experiments.md, "EMR merge").
// vlm_emr_pass_kernel: 156 VGPRs, 0 AGPRs, 104 SGPRs (6 spilled to VGPR lanes), 0 bytes of scratch, 896 B of LDS: occupancy 3
// waves per SIMD, as vlm_tall_apply_kernel (136 VGPRs).  vlm_emr_fold_kernel: 43 VGPRs, 112 B of LDS, no scratch.
#define EMR_BLOCKS_PER_CU 12

// the slots of a record
#define EMR_A 0                              // a[m]: sum f64(|x_m|)
#define EMR_B VLM_MERGE_MAX_SRC              // b[m]: sum (agree_m ? f64(e) : +0.0)
#define EMR_KEPT (2 * VLM_MERGE_MAX_SRC)     // kept[m]
#define EMR_ZERO (3 * VLM_MERGE_MAX_SRC)
#define EMR_CONFLICT (EMR_ZERO + 1)
#define EMR_SUMS VLM_EMR_SUMS

static_assert(EMR_SUMS == EMR_CONFLICT + 1 && EMR_SUMS == 14, "a record is a[4], b[4], kept[4], zero, conflict");
static_assert(sizeof(vlm_emr_result_t) == 128 && offsetof(vlm_emr_result_t, uni_sum) == EMR_B * 8 &&
                  offsetof(vlm_emr_result_t, kept) == EMR_KEPT * 8 && offsetof(vlm_emr_result_t, rescale) == EMR_SUMS * 8,
              "a result begins as a record does, then the four rescalers");

// what a chunk does, a compile-time constant of its body
#define EMR_PLAIN 0     // MERGE without masks
#define EMR_MASKS 1     // MERGE, one mask per source written
#define EMR_RESTORE 2   // RESTORE: one mask read

typedef records_view_t<vlm_emr_header_t, vlm_emr_job_t, double, vlm_emr_result_t> emr_view_t;
__device__ __forceinline__ emr_view_t emr_view(unsigned char* ws) {
  return records_view<vlm_emr_header_t, vlm_emr_job_t, double, vlm_emr_result_t>(ws);
}

// a thread's sums and counts over one chunk (RESTORE uses kept[0] alone)
template <int NSRC>
struct emr_acc_t {
  double a[NSRC], b[NSRC];
  uint32_t kept[NSRC], zero, conflict;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < NSRC; ++m) {
      a[m] = b[m] = 0.0;
      kept[m] = 0;
    }
    zero = conflict = 0;
  }
};

// Steps 1-4 and the addends of step 6 for one element; bit m of `agree` = agree_m.
template <int NSRC>
__device__ __forceinline__ float emr_elem(float c, const float* wv, float lam, emr_acc_t<NSRC>& n, uint32_t& agree) {
  float x[NSRC];
  float s = 0.0f;
  bool has_pos = false, has_neg = false;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {
    x[m] = __fsub_rn(wv[m], c);                                          // step 1
    s = __fadd_rn(s, x[m]);                                              // step 2
    has_pos |= x[m] > 0.0f;
    has_neg |= x[m] < 0.0f;
  }
  const bool sp = s > 0.0f, sn = s < 0.0f;
  float e = 0.0f;
  agree = 0;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {                                       // step 3
    const bool ag = (sp && x[m] > 0.0f) || (sn && x[m] < 0.0f);
    const float ax = fabsf(x[m]);
    e = (ag && ax > e) ? ax : e;
    agree |= (ag ? 1u : 0u) << m;
  }
  const double ed = (double)e;
#pragma unroll
  for (int m = 0; m < NSRC; ++m) {                                       // step 6: this element's addends
    const bool ag = (agree >> m) & 1u;
    n.a[m] = __dadd_rn(n.a[m], (double)fabsf(x[m]));
    n.b[m] = __dadd_rn(n.b[m], ag ? ed : 0.0);
    n.kept[m] += ag ? 1u : 0u;
  }
  n.zero += (sp || sn) ? 0u : 1u;
  n.conflict += (has_pos && has_neg) ? 1u : 0u;
  const float u = sp ? e : (sn ? -e : 0.0f);
  return __fadd_rn(c, __fmul_rn(lam, u));                                // step 4
}

// the restore rule for one element: three roundings
__device__ __forceinline__ float emr_pick(bool bit, float uni, float c, float rescale, uint32_t& kept) {
  kept += bit ? 1u : 0u;
  const float t = __fsub_rn(uni, c);
  return __fadd_rn(c, __fmul_rn(rescale, bit ? t : 0.0f));
}

// One float4 slot of a chunk, entered by EVERY thread of the workgroup (tall.hip's tall_slot).  `have`: float4 idx lies inside the
// tensor and v (one float4 per source) and b (the base) hold it.  The lane with idx == n4 of a tensor with a ragged tail handles
// the tail's elements 4 n4 + t, t < tail, as the partial float4 it is -- their addends enter THIS lane's sums, behind its float4s
// (every later slot of the lane lies past the end), in element order.  Every other lane past the end does nothing but take part
// in the cross-lane steps, with zero bits.  `scale`: lam (MERGE) or rescale (RESTORE).
template <int NSRC, int KIND>
__device__ __forceinline__ void emr_slot(const vlm_emr_job_t& j, uint64_t idx, uint64_t n4, uint32_t tail, uint64_t n_words,
                                         bool have, const f32x4* v, const f32x4& b, float scale, emr_acc_t<NSRC>& n) {
  const int lane = threadIdx.x & 63;
  const uint64_t word = tall_word_of(idx);
  const uint32_t shift = tall_shift_of(idx);   // == 4 (lane & 7): a chunk starts at a multiple of 8 float4s
  const bool leader = (lane & 7) == 0 && word < n_words;
  uint32_t nib[NSRC];                          // MERGE: bit c of nib[m] = agree_m of element c of this float4
#pragma unroll
  for (int m = 0; m < NSRC; ++m) nib[m] = 0;
  if (KIND == EMR_RESTORE) {
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
      if (KIND == EMR_RESTORE) {
        o[c] = emr_pick((nib[0] >> c) & 1u, v[0][c], b[c], scale, n.kept[0]);
      } else {
        float w[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) w[m] = v[m][c];
        uint32_t agree;
        o[c] = emr_elem<NSRC>(b[c], w, scale, n, agree);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((agree >> m) & 1u) << c;
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
      if (KIND == EMR_RESTORE) {
        o = emr_pick((nib[0] >> t) & 1u, w[0], bt, scale, n.kept[0]);
      } else {
        uint32_t agree;
        o = emr_elem<NSRC>(bt, w, scale, n, agree);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((agree >> m) & 1u) << t;
      }
      reinterpret_cast<float*>(j.dst)[i] = o;
    }
  }
  if (KIND == EMR_MASKS) {
    // step 5, the whole wave active: eight nibbles -> one word in every lane of the eight; the leader stores it, with a plain
    // store (docs/experiments.md, "Consensus merge": streamed past L2 the words cost 9 % of the pass instead of 2 %)
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
// use), the slots, then the wave sums of what the threads gathered into red[wave][slot] (lane 0 writes; only the slots the job has:
// emr_slot_used).  No __restrict__: dst may be the base or a source exactly; every load of a float4 precedes its store.
template <int NSRC, int KIND>
__device__ __forceinline__ void emr_chunk(const vlm_emr_job_t& j, uint64_t start4, double* red) {
  const uint64_t n4 = j.n_elem >> 2, n_words = tall_mask_words(j.n_elem);
  const uint32_t tail = (uint32_t)(j.n_elem & 3);
  const float scale = KIND == EMR_RESTORE ? j.rescale : j.lam;
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
  emr_acc_t<NSRC> n;
  n.clear();
#pragma unroll
  for (int u = 0; u < 4; ++u) emr_slot<NSRC, KIND>(j, idx[u], n4, tail, n_words, idx[u] < n4, v[u], b[u], scale, n);
  if (tall_has_tail_slot(start4, j.n_elem))  // workgroup-uniform
    emr_slot<NSRC, KIND>(j, start4 + CHUNK_FLOATS / 4 + threadIdx.x, n4, tail, n_words, false, v[0], b[0], scale, n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* r = red + wave * EMR_SUMS;
  auto put_n = [&](int slot, uint32_t c) {
    c = chunk_wave_sum(c);
    if (lane == 0) r[slot] = (double)c;
  };
  if (KIND == EMR_RESTORE) {
    put_n(EMR_KEPT, n.kept[0]);
  } else {
#pragma unroll
    for (int m = 0; m < NSRC; ++m) {
      const double a = chunk_wave_sum(n.a[m]), bb = chunk_wave_sum(n.b[m]);
      if (lane == 0) {
        r[EMR_A + m] = a;
        r[EMR_B + m] = bb;
      }
      put_n(EMR_KEPT + m, n.kept[m]);
    }
    put_n(EMR_ZERO, n.zero);
    put_n(EMR_CONFLICT, n.conflict);
  }
}

// does a job have the slot `k` of a record?  RESTORE: kept[0] alone.
__device__ __forceinline__ bool emr_slot_used(int k, int op, int S) {
  if (op == VLM_EMR_RESTORE) return k == EMR_KEPT;
  return k >= EMR_ZERO || (k & (VLM_MERGE_MAX_SRC - 1)) < S;
}
static_assert(VLM_MERGE_MAX_SRC == 4, "emr_slot_used takes a slot's source as k & 3");

__global__ __launch_bounds__(EMR_THREADS) void vlm_emr_pass_kernel(unsigned char* __restrict__ ws) {
  const emr_view_t w = emr_view(ws);
  chunk_reduce_run<EMR_SUMS>(
      w.chunks, w.jobs, w.hdr->n_chunks, w.first, w.records, [](uint32_t) {},
      [](const vlm_emr_job_t& j, uint64_t start4, double* r) {
        if (j.op == VLM_EMR_RESTORE) {
          emr_chunk<1, EMR_RESTORE>(j, start4, r);
        } else {
          with_nsrc(j.n_src, [&](auto S) {
            if (j.mask[0]) emr_chunk<S(), EMR_MASKS>(j, start4, r);
            else emr_chunk<S(), EMR_PLAIN>(j, start4, r);
          });
        }
      },
      [](const vlm_emr_job_t& j, int k) { return emr_slot_used(k, j.op, j.n_src); });
}

// Step 7 for a job whose folded record is s[0 .. EMR_SUMS) (LDS): the whole result, written field by field (the loops have
// compile-time bounds, so nothing is indexed at run time and nothing lives in scratch).  A slot the job does not have is +0.0 in
// every record, so its sums, counts and rescaler come out zero.
__device__ __forceinline__ void emr_result(const double* s, vlm_emr_result_t* out) {
#pragma unroll
  for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) {
    const double a = s[EMR_A + m], b = s[EMR_B + m];
    out->abs_sum[m] = a;
    out->uni_sum[m] = b;
    out->kept[m] = (uint64_t)s[EMR_KEPT + m];
    out->rescale[m] = b > 0.0 ? __double2float_rn(__ddiv_rn(a, b)) : 0.0f;
  }
  out->zero = (uint64_t)s[EMR_ZERO];
  out->conflict = (uint64_t)s[EMR_CONFLICT];
}

__global__ __launch_bounds__(EMR_FOLD_THREADS) void vlm_emr_fold_kernel(unsigned char* __restrict__ ws) {
  __shared__ double sums[EMR_SUMS];
  const emr_view_t w = emr_view(ws);
  const int k = threadIdx.x;
  // a workgroup per job; the grid is fixed (the job count lives in the header, on the device), so it strides over the jobs
  for (uint64_t job = blockIdx.x; job < w.hdr->n_jobs; job += gridDim.x) {
    if (k < EMR_SUMS) {
      const double* rec = w.records + k;
      const uint64_t c0 = w.first[job], c1 = w.first[job + 1];
      double sum = 0.0;
      CHUNK_FOLD_RECORDS(sum, rec, EMR_SUMS, c0, c1);
      sums[k] = sum;
    }
    __syncthreads();
    if (k == 0) emr_result(sums, &w.results[job]);
    __syncthreads();  // the next job's sums overwrite these
  }
}

extern "C" size_t vlm_emr_plan_bytes(int n_jobs, uint64_t total_elems) {
  return records_plan_bytes<vlm_emr_header_t, vlm_emr_job_t>(n_jobs, total_elems, EMR_SUMS * sizeof(double), sizeof(vlm_emr_result_t));
}

extern "C" int vlm_emr_plan_upload(const vlm_emr_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream) {
  return records_plan_upload<vlm_emr_header_t>(
      jobs, n_jobs, workspace, workspace_bytes, stream, EMR_SUMS * sizeof(double), sizeof(vlm_emr_result_t), [](const vlm_emr_job_t& j) {
        const int rc = chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);  // one elementwise pass: dst may be an input exactly
        return rc == VLM_OK ? emr_job_check(j) : rc;
      });
}

extern "C" int vlm_emr_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // two launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL(vlm_emr_pass_kernel, chunk_grid(EMR_BLOCKS_PER_CU), dim3(EMR_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_emr_fold_kernel, chunk_grid(1), dim3(EMR_FOLD_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
