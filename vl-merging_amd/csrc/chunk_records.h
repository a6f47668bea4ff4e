// The record reducer of the merge family (pairstats.hip, stock.hip and sphere.hip through gram_reduce.h, sce.hip, emr.hip), stated once:
// a pass over the chunk table that leaves ONE record of f64 sums per chunk, at the chunk's index, so that how the chunks were
// dealt to workgroups cannot show in a result.  The pinned order of every sum (include/vlm_hip.h): thread, wave by halves,
// ((w0 + w1) + w2) + w3, the records of a job added in chunk order, every sum from +0.0.
//   records_view       a record plan's workspace
//   chunk_wave_sum     the wave fold by halves
//   chunk_record       the four waves' sums into the chunk's record
//   chunk_reduce_run   a workgroup's run of chunks around a method's own chunk body
//   CHUNK_FOLD_RECORDS a job's records added in chunk order (the fold kernels)
// The host side -- first[], the record plan's layout and upload -- is chunk_plan.h's.
// Device code only.  -ffp-contract=off and the __d*_rn forms: one rounding per operation, no FMA.
#pragma once
#include "vlm_common.h"
#include "chunk_walk.h"

#define RECORD_WAVES (CHUNK_THREADS / 64)
#define RECORD_FOLD_BATCH 16  // records whose loads are in flight together in a fold (the additions stay in order)

// A record plan's workspace (chunk_plan.h: records_layout) as the kernels of pairstats.hip and stock.hip see it: Record is what the
// records are addressed as ([n_chunks][slots]), Result what the results are ([n_jobs]).
template <class Hdr, class Job, class Record, class Result>
struct records_view_t {
  const Hdr* hdr;
  const Job* jobs;
  const chunk_t* chunks;
  const uint64_t* first;
  Record* records;
  Result* results;
};

template <class Hdr, class Job, class Record, class Result>
__device__ __forceinline__ records_view_t<Hdr, Job, Record, Result> records_view(unsigned char* ws) {
  records_view_t<Hdr, Job, Record, Result> v;
  v.hdr = reinterpret_cast<const Hdr*>(ws);
  v.jobs = reinterpret_cast<const Job*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.first = reinterpret_cast<const uint64_t*>(ws + v.hdr->first_off);
  v.records = reinterpret_cast<Record*>(ws + v.hdr->records_off);
  v.results = reinterpret_cast<Result*>(ws + v.hdr->results_off);
  return v;
}

// the wave fold by halves: lane 0 ends with the pinned tree's value (a + b is commutative, so the butterfly's lane 0 is the tree's
// -- and every other lane's: all 64 end with the same bytes)
__device__ __forceinline__ double chunk_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ uint32_t chunk_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The record of the chunk at start4 of a job whose first record is `first`, from the wave sums r[wave][slot] (behind a barrier):
// threads 0 .. SUMS - 1 add ((w0 + w1) + w2) + w3; a sum the job does not have (`used(slot)` is false) is zero.  The record index
// is the chunk index.
template <int SUMS, class Used>
__device__ __forceinline__ void chunk_record(const double* r, Used&& used, double* records, uint64_t first, uint64_t start4) {
  if (threadIdx.x < SUMS) {
    const int k = threadIdx.x;
    double t = 0.0;
    if (used(k)) {
      t = r[k];
#pragma unroll
      for (int wv = 1; wv < RECORD_WAVES; ++wv) t = __dadd_rn(t, r[wv * SUMS + k]);
    }
    records[(first + (start4 / (CHUNK_FLOATS / 4))) * SUMS + k] = t;
  }
}

// The run of chunks this workgroup owns, for a plan with the tables `chunks`, `jobs` and `first_of` (chunk_first_fill).  Entering a
// job: its first record, then `enter(job index)` for the method's own scalars.  Per chunk: `chunk(job, start4, r)` leaves the wave
// sums of the chunk in r[wave][slot]; behind ONE barrier they become the chunk's record (`used(job, slot)`) -- two buffers, used in
// turn, so the next chunk's wave sums are written to the other while these are read.
template <int SUMS, class Job, class Enter, class Chunk, class Used>
__device__ __forceinline__ void chunk_reduce_run(const chunk_t* chunks, const Job* jobs, uint64_t n_chunks, const uint64_t* first_of,
                                                 double* records, Enter&& enter, Chunk&& chunk, Used&& used) {
  __shared__ double red[2][RECORD_WAVES * SUMS];
  uint64_t c0, c1;
  if (!chunk_my_run(n_chunks, &c0, &c1)) return;
  uint64_t first = 0;
  int turn = 0;
  chunk_run(
      chunks, jobs, c0, c1,
      [&](uint32_t cur) {
        first = first_of[cur];
        enter(cur);
      },
      [&](const Job& j, uint64_t start4) {
        double* r = red[turn];
        chunk(j, start4, r);
        __syncthreads();
        chunk_record<SUMS>(r, [&](int k) { return used(j, k); }, records, first, start4);
        turn ^= 1;
      },
      [&](uint32_t) {});
}

// A job's sum at one slot: `sum` (a double at +0.0) receives the records c0 .. c1 added in chunk order; a missing record adds +0.0
// and changes no sum.  `rec`: the slot's place in record 0, `stride`: doubles per record.  A macro, not a function: as an inlined
// function the loop is rotated otherwise, and the fold kernels keep the instructions they had when the loop stood in them.
#define CHUNK_FOLD_RECORDS(sum, rec, stride, c0, c1)                                                                           \
  for (uint64_t c = (c0); c < (c1); c += RECORD_FOLD_BATCH) {                                                                  \
    double v[RECORD_FOLD_BATCH];                                                                                               \
    _Pragma("unroll") for (int i = 0; i < RECORD_FOLD_BATCH; ++i) v[i] = c + i < (c1) ? (rec)[(c + i) * (stride)] : 0.0;       \
    _Pragma("unroll") for (int i = 0; i < RECORD_FOLD_BATCH; ++i) sum = __dadd_rn(sum, v[i]);                                  \
  }
