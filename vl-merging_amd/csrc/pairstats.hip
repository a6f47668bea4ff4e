// Expert-pair statistics over every tensor of a checkpoint: squared norms, dot products, squared distances, the soft sign
// dissimilarity and its truncated form, sign conflicts -- what "how far apart are the experts?" is answered from.
// No reference site: the reference repository ships no such measure.  The rule, INCLUDING the order of every floating-point
// sum, is written down in include/vlm_hip.h and restated in numpy by tests/pairstats_restatement.py; the kernels are held to
// that restatement bit for bit.
//
// The pass reads what the task-vector merge reads, 4 (S + 1) B per element, and writes one 448-B record per 16-KiB chunk.
//   vlm_pairstats_stream_kernel  one launch over the plan's chunk table (chunk_plan.h), dealt as vlm_dare_apply_kernel's: a
//                                workgroup owns a CONTIGUOUS run of chunks.  Per chunk: the per-thread sums from +0.0 through
//                                chunk_stream<S, BASE, false> (chunk_walk.h), the wave fold by halves, the four waves added in
//                                order, one record written at the chunk's index -- so the dealing cannot show in the result.
//   vlm_pairstats_fold_kernel    one workgroup per job at a time, one thread per statistic: the job's records added in chunk order.
// No atomics; every record and every result is overwritten by each run, so nothing is cleared.  -ffp-contract=off and the
// __f*_rn / __d*_rn forms: one rounding per operation, no FMA.
// This file holds the rule (pairstats_rule) and the two reductions; the walker and the run loop are chunk_walk.h's, the wave fold
// and the workspace's view chunk_records.h's, the record plan (layout, upload) and the host checks chunk_plan.h's.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "chunk_records.h"  // the view and the wave fold (the record writer and the fold are this file's own: see below)

#define PS_THREADS CHUNK_THREADS
#define PS_PAIRS VLM_PAIRSTATS_PAIRS
#define PS_HALF (VLM_MERGE_MAX_SRC + 4 * PS_PAIRS)  // 28 doubles, then 28 counts: vlm_pairstats_result_t as 56 8-byte slots
#define PS_SLOTS (2 * PS_HALF)
#define PS_FOLD_THREADS 128           // wave 0: the doubles, wave 1: the counts
// Just under 256 registers: two workgroups per CU are resident (tests/test_pairstats_cpu.py watches the occupancy); six rounds of
// them keep the runs short enough to even out their ends.  Measured against 2, 4, 8 and 16: docs/experiments.md, "Pair statistics".
#define PS_BLOCKS_PER_CU 12

static_assert(sizeof(vlm_pairstats_result_t) == PS_SLOTS * 8, "a result is 56 8-byte slots");
static_assert(PS_PAIRS == VLM_MERGE_MAX_SRC * (VLM_MERGE_MAX_SRC - 1) / 2, "one slot per pair");

// records: [n_chunks][PS_SLOTS], results: [n_jobs][PS_SLOTS], doubles as their bits
typedef records_view_t<vlm_pairstats_header_t, vlm_pairstats_job_t, u64_t, u64_t> ps_view_t;
__device__ __forceinline__ ps_view_t ps_view(unsigned char* ws) {
  return records_view<vlm_pairstats_header_t, vlm_pairstats_job_t, u64_t, u64_t>(ws);
}

// A thread's sums over one chunk, for a job of S sources: NP = S (S - 1) / 2 pairs, pair (a, b) at b (b - 1) / 2 + a < NP.
template <int S>
struct ps_acc_t {
  static constexpr int NP = S * (S - 1) / 2;
  static constexpr int NPA = NP > 0 ? NP : 1;
  double sq[S], dot[NPA], dist2[NPA], ssd[NPA], tssd[NPA];
  uint32_t nnz[S], live[NPA], conflict[NPA], tlive[NPA], tconflict[NPA];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < S; ++m) {
      sq[m] = 0.0;
      nnz[m] = 0;
    }
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      dot[p] = dist2[p] = ssd[p] = tssd[p] = 0.0;
      live[p] = conflict[p] = tlive[p] = tconflict[p] = 0;
    }
  }
};

// Steps 1-3 as chunk_stream's rule: elem() adds one element to the thread's sums and returns nothing worth storing.
template <int S, bool BASE>
struct pairstats_rule {
  const uint32_t* tkey;  // workgroup-uniform
  ps_acc_t<S>& n;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    float x[S];
    double xd[S];
    bool in[S];
#pragma unroll
    for (int m = 0; m < S; ++m) {
      x[m] = BASE ? __fsub_rn(wv[m], c) : wv[m];                                   // step 1
      in[m] = (__float_as_uint(x[m]) & 0x7fffffffu) >= tkey[m];
      xd[m] = (double)x[m];
      n.sq[m] = __dadd_rn(n.sq[m], __dmul_rn(xd[m], xd[m]));                       // step 2
      n.nnz[m] += x[m] != 0.0f ? 1u : 0u;
    }
#pragma unroll
    for (int b = 1; b < S; ++b) {                                                  // step 3
#pragma unroll
      for (int a = 0; a < b; ++a) {
        const int p = b * (b - 1) / 2 + a;
        const float den = __fadd_rn(fabsf(x[a]), fabsf(x[b]));
        const bool live = den > 0.0f;
        const float r = live ? __fdiv_rn(fabsf(__fadd_rn(x[a], x[b])), den) : 0.0f;
        const bool conf = (x[a] > 0.0f && x[b] < 0.0f) || (x[a] < 0.0f && x[b] > 0.0f);
        const bool t = live && (in[a] || in[b]);
        const double d = __dsub_rn(xd[a], xd[b]);
        const double rd = (double)r;
        n.dot[p] = __dadd_rn(n.dot[p], __dmul_rn(xd[a], xd[b]));
        n.dist2[p] = __dadd_rn(n.dist2[p], __dmul_rn(d, d));
        n.ssd[p] = __dadd_rn(n.ssd[p], rd);
        n.tssd[p] = __dadd_rn(n.tssd[p], t ? rd : 0.0);
        n.live[p] += live ? 1u : 0u;
        n.conflict[p] += conf ? 1u : 0u;
        n.tlive[p] += t ? 1u : 0u;
        n.tconflict[p] += (t && conf) ? 1u : 0u;
      }
    }
    return 0.0f;
  }
};

// Wave sums of the thread's statistics into red[wave][slot] (lane 0 writes; the slots are vlm_pairstats_result_t's order).
template <int S>
__device__ __forceinline__ void ps_wave_fold(const ps_acc_t<S>& n, u64_t* red) {
  constexpr int NP = ps_acc_t<S>::NP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64_t* r = red + wave * PS_SLOTS;
  auto put_d = [&](int slot, double v) {
    v = chunk_wave_sum(v);
    if (lane == 0) r[slot] = (u64_t)__double_as_longlong(v);
  };
  auto put_n = [&](int slot, uint32_t v) {
    v = chunk_wave_sum(v);
    if (lane == 0) r[PS_HALF + slot] = v;
  };
#pragma unroll
  for (int m = 0; m < S; ++m) {
    put_d(m, n.sq[m]);
    put_n(m, n.nnz[m]);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    put_d(VLM_MERGE_MAX_SRC + p, n.dot[p]);
    put_d(VLM_MERGE_MAX_SRC + PS_PAIRS + p, n.dist2[p]);
    put_d(VLM_MERGE_MAX_SRC + 2 * PS_PAIRS + p, n.ssd[p]);
    put_d(VLM_MERGE_MAX_SRC + 3 * PS_PAIRS + p, n.tssd[p]);
    put_n(VLM_MERGE_MAX_SRC + p, n.live[p]);
    put_n(VLM_MERGE_MAX_SRC + PS_PAIRS + p, n.conflict[p]);
    put_n(VLM_MERGE_MAX_SRC + 2 * PS_PAIRS + p, n.tlive[p]);
    put_n(VLM_MERGE_MAX_SRC + 3 * PS_PAIRS + p, n.tconflict[p]);
  }
}

// does a job of S sources have the statistic at `slot` (0 .. PS_SLOTS)?
__device__ __forceinline__ bool ps_slot_used(int slot, int S) {
  const int g = slot < PS_HALF ? slot : slot - PS_HALF;
  return g < VLM_MERGE_MAX_SRC ? g < S : (g - VLM_MERGE_MAX_SRC) % PS_PAIRS < S * (S - 1) / 2;
}

template <int S, bool BASE>
__device__ __forceinline__ void ps_chunk(const vlm_pairstats_job_t& j, uint64_t start4, const uint32_t* tkey, u64_t* red) {
  ps_acc_t<S> n;
  n.clear();
  pairstats_rule<S, BASE> rule{tkey, n};
  chunk_stream<S, BASE, false>(j, start4, rule);
  ps_wave_fold<S>(n, red);
}

__global__ __launch_bounds__(PS_THREADS) void vlm_pairstats_stream_kernel(unsigned char* __restrict__ ws) {
  // two buffers, used in turn: a chunk's wave sums are read behind ONE barrier while the next chunk's are written to the other
  __shared__ u64_t red[2][RECORD_WAVES * PS_SLOTS];
  const ps_view_t w = ps_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  uint32_t tkey[VLM_MERGE_MAX_SRC] = {0, 0, 0, 0};
  uint64_t first = 0;
  int turn = 0;
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_pairstats_job_t& jn = w.jobs[cur];
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) tkey[m] = jn.tkey[m];
        first = w.first[cur];
      },
      [&](const vlm_pairstats_job_t& j, uint64_t start4) {
        u64_t* r = red[turn];
        with_nsrc(j.n_src, [&](auto S) {
          if (j.base) ps_chunk<S(), true>(j, start4, tkey, r);
          else ps_chunk<S(), false>(j, start4, tkey, r);
        });
        __syncthreads();
        // This record writer (and the run around it) stays this file's own beside chunk_records.h's chunk_record and
        // chunk_reduce_run: a record here mixes doubles (as their bits) and counts in 8-byte slots, and the shared writer adds doubles.
        if (threadIdx.x < PS_SLOTS) {  // ((w0 + w1) + w2) + w3; the statistics the job does not have are zero
          const int k = threadIdx.x;
          u64_t out = 0;
          if (ps_slot_used(k, j.n_src)) {
            if (k < PS_HALF) {
              double t = __longlong_as_double((long long)r[k]);
#pragma unroll
              for (int wv = 1; wv < RECORD_WAVES; ++wv) t = __dadd_rn(t, __longlong_as_double((long long)r[wv * PS_SLOTS + k]));
              out = (u64_t)__double_as_longlong(t);
            } else {
#pragma unroll
              for (int wv = 0; wv < RECORD_WAVES; ++wv) out += r[wv * PS_SLOTS + k];
            }
          }
          w.records[(first + (start4 / (CHUNK_FLOATS / 4))) * PS_SLOTS + k] = out;  // the record index is the chunk index
        }
        turn ^= 1;
      },
      [&](uint32_t) {});
}

__global__ __launch_bounds__(PS_FOLD_THREADS) void vlm_pairstats_fold_kernel(unsigned char* __restrict__ ws) {
  const ps_view_t w = ps_view(ws);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane >= PS_HALF) return;
  const int k = wave * PS_HALF + lane;
  const u64_t* rec = w.records + k;
  // a workgroup per job; the grid is fixed (the job count lives in the header, on the device), so it strides over the jobs
  for (uint64_t job = blockIdx.x; job < w.hdr->n_jobs; job += gridDim.x) {
    const uint64_t c0 = w.first[job], c1 = w.first[job + 1];
    double sum = 0.0;
    u64_t cnt = 0;
    for (uint64_t c = c0; c < c1; c += RECORD_FOLD_BATCH) {
      u64_t v[RECORD_FOLD_BATCH];
#pragma unroll
      for (int i = 0; i < RECORD_FOLD_BATCH; ++i) v[i] = c + i < c1 ? rec[(c + i) * PS_SLOTS] : 0;  // +0.0 or 0: changes no sum
#pragma unroll
      for (int i = 0; i < RECORD_FOLD_BATCH; ++i) {
        if (wave == 0) sum = __dadd_rn(sum, __longlong_as_double((long long)v[i]));
        else cnt += v[i];
      }
    }
    w.results[job * PS_SLOTS + k] = wave == 0 ? (u64_t)__double_as_longlong(sum) : cnt;
  }
}

extern "C" size_t vlm_pairstats_plan_bytes(int n_jobs, uint64_t total_elems) {
  return records_plan_bytes<vlm_pairstats_header_t, vlm_pairstats_job_t>(n_jobs, total_elems, sizeof(vlm_pairstats_result_t),
                                                                         sizeof(vlm_pairstats_result_t));
}

extern "C" int vlm_pairstats_plan_upload(const vlm_pairstats_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  return records_plan_upload<vlm_pairstats_header_t>(
      jobs, n_jobs, workspace, workspace_bytes, stream, sizeof(vlm_pairstats_result_t), sizeof(vlm_pairstats_result_t),
      [](const vlm_pairstats_job_t& j) { return chunk_job_check<false>(j, CHUNK_OVERLAP_UNCHECKED, false); });  // no dst: nothing for an input to overlap
}

extern "C" int vlm_pairstats_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // two launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header
  hipLaunchKernelGGL(vlm_pairstats_stream_kernel, chunk_grid(PS_BLOCKS_PER_CU), dim3(PS_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_pairstats_fold_kernel, chunk_grid(1), dim3(PS_FOLD_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
