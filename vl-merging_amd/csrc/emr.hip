// EMR-Merging (Huang et al., NeurIPS 2024: elect, mask and rescale) over every output tensor of an all_moe -> ufo merge, and the
// way back: one expert rebuilt from the unified tensor, the central tensor, a packed mask and one scalar.
// No reference site: the reference repository has neither.  The rule, INCLUDING the order of every floating-point sum, is written
// down in include/vlm_hip.h and restated in numpy by tests/emr_restatement.py; the kernels are held to that restatement bit for
// bit, mask words, padding bits, sums and rescalers included.
//
// The pass is the consensus merge's traffic with masks on, 4 (S + 1) B read, 4 B written and S / 8 B of mask per element
// (RESTORE: 8 B + 1 / 8 B read, 4 B written), plus one 112-B record per 16-KiB chunk.
//   vlm_emr_pass_kernel   one launch over the plan's chunk table through chunk_reduce_run (chunk_records.h).  The chunk body is
//                         mask_chunk (mask_chunk.h, shared with tall.hip: the slot every thread enters, the one lane that owns the
//                         ragged tail, the plain word store); this file's rule also gathers, per thread, the f64 addends of step 6
//                         and the counts; their wave sums go to chunk_record, which leaves one record at the chunk's index.  Both
//                         ops, one kernel.
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
// and the host checks chunk_plan.h's, the chunk body mask_chunk.h's, the place of a bit and the checks on a job's masks tall_mask.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "chunk_records.h"
#include "mask_chunk.h"
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

// what mask_chunk asks of a method: `scale`, lam (MERGE) or rescale (RESTORE), and the thread's sums and counts, by reference
template <int NSRC>
struct emr_rule_t {
  float scale;
  emr_acc_t<NSRC>& n;
  __device__ __forceinline__ float elem(float c, const float* w, uint32_t& bits) { return emr_elem<NSRC>(c, w, scale, n, bits); }
  __device__ __forceinline__ float pick(bool bit, float u, float c) { return emr_pick(bit, u, c, scale, n.kept[0]); }
};

// The chunk at start4 of job j: mask_chunk (mask_chunk.h) with this file's rule, then the wave sums of what the threads gathered
// into red[wave][slot] (lane 0 writes; only the slots the job has: emr_slot_used).
template <int NSRC, int KIND>
__device__ __forceinline__ void emr_chunk(const vlm_emr_job_t& j, uint64_t start4, double* red) {
  emr_acc_t<NSRC> n;
  n.clear();
  emr_rule_t<NSRC> rule = {KIND == MASK_RESTORE ? j.rescale : j.lam, n};
  mask_chunk<NSRC, KIND>(j, start4, rule);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* r = red + wave * EMR_SUMS;
  auto put_n = [&](int slot, uint32_t c) {
    c = chunk_wave_sum(c);
    if (lane == 0) r[slot] = (double)c;
  };
  if (KIND == MASK_RESTORE) {
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
          emr_chunk<1, MASK_RESTORE>(j, start4, r);
        } else {
          with_nsrc(j.n_src, [&](auto S) {
            if (j.mask[0]) emr_chunk<S(), MASK_WRITE>(j, start4, r);
            else emr_chunk<S(), MASK_PLAIN>(j, start4, r);
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
