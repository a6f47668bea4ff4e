// The chunk plan of the merge family (merge.hip, ties.hip): every job (one output tensor) is cut into 16-KiB chunks listed in a
// device-resident table, so that ONE grid covers all tensors of a plan.  A chunk is what one 256-thread workgroup moves as
// 4 float4 per thread; a job's ragged end (n_elem % 4 floats) rides with exactly one of its chunks.
// Everything but the upload compiles without HIP (tests/helpers/chunk_plan_check.cpp does so).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define CHUNK_FLOATS 4096u  // floats per chunk: 256 threads x 4 float4
#define CHUNK_THREADS 256

struct chunk_t {
  uint32_t job;
  uint32_t start4;  // chunk start / 4 (float4 units)
};

static inline size_t chunk_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static inline uint64_t chunks_of(uint64_t n_elem) {
  uint64_t n4 = n_elem >> 2;
  uint64_t c = (n4 + CHUNK_FLOATS / 4 - 1) / (CHUNK_FLOATS / 4);
  return c == 0 ? 1 : c;  // a job shorter than 4 floats still needs its tail chunk
}

// what *_plan_bytes reserves before the jobs are known: every job may add one partial chunk
static inline uint64_t chunks_bound(int n_jobs, uint64_t total_elems) {
  return total_elems / CHUNK_FLOATS + 2ull * (uint64_t)n_jobs + 1;
}

// The checks every job of the family passes.  A pointer that fails is VLM_ERR_ARG; a length or a chunk count that fails is
// VLM_ERR_UNSUPPORTED (start4 and n_chunks are 32-bit).
static inline bool chunk_ptr_ok(const void* p) { return p && !((uintptr_t)p & 15); }
static inline bool chunk_len_ok(uint64_t n_elem) { return (n_elem >> 2) < (1ull << 32); }
static inline bool chunk_count_ok(uint64_t n_chunks) { return n_chunks < (1ull << 32); }

// `ck` receives sum_i chunks_of(jobs[i].n_elem) records.  Plain job order: a workgroup's stream of chunks stays contiguous.
template <class Job>
static inline uint64_t chunk_table_fill(chunk_t* ck, const Job* jobs, int n_jobs) {
  uint64_t c = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const uint64_t nc = chunks_of(jobs[i].n_elem);
    for (uint64_t k = 0; k < nc; ++k) {
      ck[c].job = (uint32_t)i;
      ck[c].start4 = (uint32_t)(k * (CHUNK_FLOATS / 4));
      ++c;
    }
  }
  return c;
}

#ifdef __HIPCC__
#define CHUNK_HD __host__ __device__ __forceinline__
#else
#define CHUNK_HD static inline
#endif

// The ragged tail (n_elem % 4 floats) belongs to the chunk that holds the last float4, or to chunk 0 of a job shorter than
// one.  Host and device: the kernels ask, the host test checks that exactly one chunk of a job answers yes.
CHUNK_HD bool chunk_owns_tail(uint64_t start4, uint64_t n_elem) { return start4 + (CHUNK_FLOATS / 4) >= (n_elem >> 2); }
// how many tail floats the chunk at start4 owns: thread t < that count handles element (n_elem & ~3) + t
CHUNK_HD uint32_t chunk_tail_len(uint64_t start4, uint64_t n_elem) {
  return chunk_owns_tail(start4, n_elem) ? (uint32_t)(n_elem & 3) : 0u;
}

#ifdef __HIPCC__
// Host image -> device.  `img` is a pageable temporary, so the copy is waited for before the caller lets it die: the upload
// entry points synchronise the stream (include/vlm_hip.h says so).
static inline int chunk_upload(void* dst, const void* img, size_t bytes, hipStream_t s) {
  if (hipMemcpyAsync(dst, img, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return VLM_ERR_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return VLM_ERR_LAUNCH;
  return VLM_OK;
}
#endif
