// The chunk plan of the merge family (merge.hip, ties.hip, dare.hip, pairstats.hip, band.hip, stock.hip, sce.hip, sphere.hip,
// tall.hip; della.hip takes its checks, layout cursor, upload and run and lists tiles of rows instead): every job (one tensor) is
// cut into 16-KiB chunks listed in a device-resident table, so that ONE grid covers all tensors of a plan.  A chunk is what one
// 256-thread workgroup moves as 4 float4 per thread; a job's ragged end (n_elem % 4 floats) rides with exactly one of its chunks.
// This is the family's host side, stated once: the chunk table, the checks every job passes (chunk_job_check, chunk_jobs_check),
// the host image "header, jobs, chunk table" (chunk_layout_t, chunk_image), its upload and the grid rule -- and the two plans
// that several methods share whole: the COUNTER plan (header, jobs, chunks, counters per job: dare.hip, tall.hip) and the RECORD
// plan (header, jobs, chunks, first[], one record per chunk, one result per job: pairstats.hip, stock.hip, emr.hip; sphere.hip puts its
// tiles between).  The device side -- the chunk walker, a workgroup's run loop, the source-count dispatch, the counter plan's
// view -- is chunk_walk.h; the record plan's reducer is chunk_records.h.
// Everything but the uploads, the grid and the runs compiles without HIP (tests/helpers/chunk_plan_check.cpp does so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/vlm_hip.h"

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

// dst against an input of the same job (overlap ACROSS jobs is the caller's to avoid)
enum chunk_overlap_t {
  CHUNK_OVERLAP_UNCHECKED,  // plain merge: the caller's to avoid
  CHUNK_OVERLAP_NONE,       // TIES: dst may not meet an input (the selection passes re-read the inputs)
  CHUNK_OVERLAP_EXACT       // DARE: dst may be an input exactly (the pass is elementwise), any other meeting is refused
};

// do the byte ranges [a, a + 4 n) and [b, b + 4 n) meet?
static inline bool chunk_ranges_meet(const void* a, const void* b, uint64_t n_elem) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  const uint64_t bytes = n_elem * 4;
  return x < y ? (y - x) < bytes : (x - y) < bytes;
}

static inline bool chunk_input_ok(chunk_overlap_t overlap, const void* dst, const void* in, uint64_t n_elem) {
  if (!chunk_ptr_ok(in)) return false;
  if (overlap == CHUNK_OVERLAP_UNCHECKED || (overlap == CHUNK_OVERLAP_EXACT && dst == in)) return true;
  return !chunk_ranges_meet(dst, in, n_elem);
}

// The checks on a job's fields dst, base, src, n_src and n_elem, in the family's order of precedence.  `need_base`: a NULL base
// is VLM_ERR_ARG (otherwise it is skipped).  Where byte ranges are compared, the length is checked before they are formed.
// HAS_DST = false: a job type without a `dst` field (pair statistics write no tensor) -- nothing is asked of an output and no
// byte ranges are compared, whatever `overlap` says; the inputs' pointers, the source count and the length are checked as ever.
template <bool HAS_DST = true, class Job>
static inline int chunk_job_check(const Job& j, chunk_overlap_t overlap, bool need_base) {
  const void* dst = nullptr;
  if constexpr (HAS_DST) dst = j.dst;
  else overlap = CHUNK_OVERLAP_UNCHECKED;
  if (j.n_src < 1 || j.n_src > VLM_MERGE_MAX_SRC || (HAS_DST && !dst) || (need_base && !j.base)) return VLM_ERR_ARG;
  if (overlap != CHUNK_OVERLAP_UNCHECKED && !chunk_len_ok(j.n_elem)) return VLM_ERR_UNSUPPORTED;
  if ((HAS_DST && !chunk_ptr_ok(dst)) || (j.base && !chunk_input_ok(overlap, dst, j.base, j.n_elem))) return VLM_ERR_ARG;
  for (int m = 0; m < j.n_src; ++m)
    if (!chunk_input_ok(overlap, dst, j.src[m], j.n_elem)) return VLM_ERR_ARG;
  return chunk_len_ok(j.n_elem) ? VLM_OK : VLM_ERR_UNSUPPORTED;
}

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

// first[i] = the chunks before job i, first[n_jobs] = the plan's chunks, which is returned: a reducer writes one record per chunk
// at the chunk's index, and a job's records are first[i] .. first[i + 1].  `chunks(job)`: a job's chunk count (sphere_plan.h: a
// row job has none).
template <class Job, class Chunks>
static inline uint64_t chunk_first_fill(const Job* jobs, int n_jobs, uint64_t* first, Chunks&& chunks) {
  uint64_t c = 0;
  for (int i = 0; i < n_jobs; ++i) {
    first[i] = c;
    c += chunks(jobs[i]);
  }
  first[n_jobs] = c;
  return c;
}
template <class Job>
static inline uint64_t chunk_first_fill(const Job* jobs, int n_jobs, uint64_t* first) {
  return chunk_first_fill(jobs, n_jobs, first, [](const Job& j) { return chunks_of(j.n_elem); });
}

// The head of an upload: the arguments, then per job, in job order, "n_elem > 0" and the method's own `check(job)` (VLM_OK or
// the code to return).  The first job that fails decides.
template <class Job, class Check>
static inline int chunk_jobs_check(const Job* jobs, int n_jobs, const void* workspace, Check&& check) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  for (int i = 0; i < n_jobs; ++i) {
    if (jobs[i].n_elem == 0) return VLM_ERR_ARG;
    const int rc = check(jobs[i]);
    if (rc != VLM_OK) return rc;
  }
  return VLM_OK;
}

// A workspace is laid out as 256-byte aligned parts, the header first: take() gives the next part's offset.
struct chunk_layout_t {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += chunk_align_up(bytes, 256);
    return at;
  }
};

// The parts every chunk plan begins with: the header, the jobs, the chunk table.  Returns the cursor behind them.
template <class Hdr, class Job>
static inline chunk_layout_t chunk_layout_head(Hdr* h, uint64_t n_jobs, uint64_t n_chunks) {
  chunk_layout_t at;
  at.take(sizeof(Hdr));
  h->n_jobs = n_jobs;
  h->n_chunks = n_chunks;
  h->jobs_off = at.take(n_jobs * sizeof(Job));
  h->chunks_off = at.take(n_chunks * sizeof(chunk_t));
  return at;
}

// The counter plan: `counters` 64-bit counters per job behind the chunk table (device-made: every run zeroes them first).
// Fills every offset of `h`; returns the total size.
template <class Hdr, class Job>
static inline size_t counts_layout(Hdr* h, uint64_t n_jobs, uint64_t n_chunks, int counters) {
  chunk_layout_t at = chunk_layout_head<Hdr, Job>(h, n_jobs, n_chunks);
  h->counters_off = at.take(n_jobs * counters * sizeof(uint64_t));
  return at.off;
}

template <class Hdr, class Job>
static inline size_t counts_plan_bytes(int n_jobs, uint64_t total_elems, int counters) {
  if (n_jobs < 0) return 0;
  Hdr h;
  return counts_layout<Hdr, Job>(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems), counters);
}

// The record plan's own parts, appended at `at` to a header whose n_jobs and n_chunks are set: first[n_jobs + 1] (host-made),
// then one record per chunk and one result per job (device-made: every run overwrites all of them).
template <class Hdr>
static inline void records_parts(chunk_layout_t& at, Hdr* h, size_t record_bytes, size_t result_bytes) {
  h->first_off = at.take((h->n_jobs + 1) * sizeof(uint64_t));
  h->records_off = at.take(h->n_chunks * record_bytes);
  h->results_off = at.take(h->n_jobs * result_bytes);
}

// The record plan.  Fills every offset of `h`; returns the total size.
template <class Hdr, class Job>
static inline size_t records_layout(Hdr* h, uint64_t n_jobs, uint64_t n_chunks, size_t record_bytes, size_t result_bytes) {
  chunk_layout_t at = chunk_layout_head<Hdr, Job>(h, n_jobs, n_chunks);
  records_parts(at, h, record_bytes, result_bytes);
  return at.off;
}

template <class Hdr, class Job>
static inline size_t records_plan_bytes(int n_jobs, uint64_t total_elems, size_t record_bytes, size_t result_bytes) {
  if (n_jobs < 0) return 0;
  Hdr h;
  return records_layout<Hdr, Job>(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems), record_bytes, result_bytes);
}

// The host image of a plan: `hdr` at 0, the jobs at hdr.jobs_off, their chunk table at hdr.chunks_off, zeros up to img_bytes
// (where a method appends tables of its own).  What lies behind img_bytes in the workspace is device-made.
template <class Hdr, class Job>
static inline std::vector<unsigned char> chunk_image(const Hdr& hdr, const Job* jobs, int n_jobs, size_t img_bytes) {
  std::vector<unsigned char> img(img_bytes, 0);
  memcpy(img.data(), &hdr, sizeof(hdr));
  memcpy(img.data() + hdr.jobs_off, jobs, (size_t)n_jobs * sizeof(Job));
  chunk_table_fill(reinterpret_cast<chunk_t*>(img.data() + hdr.chunks_off), jobs, n_jobs);
  return img;
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
// Host image -> device, after `zero_bytes` behind it are zeroed (TIES: its histograms start at zero).  `img` is a pageable
// temporary, so the copy is waited for before the caller lets it die: the upload entry points synchronise the stream
// (include/vlm_hip.h says so).
static inline int chunk_upload(void* dst, const std::vector<unsigned char>& img, size_t zero_bytes, hipStream_t s) {
  if (zero_bytes && hipMemsetAsync((unsigned char*)dst + img.size(), 0, zero_bytes, s) != hipSuccess) return VLM_ERR_LAUNCH;
  if (hipMemcpyAsync(dst, img.data(), img.size(), hipMemcpyHostToDevice, s) != hipSuccess) return VLM_ERR_LAUNCH;
  if (hipStreamSynchronize(s) != hipSuccess) return VLM_ERR_LAUNCH;
  return VLM_OK;
}

// `per_cu` workgroups per CU (256 CUs when the device does not say)
static inline dim3 chunk_grid(int per_cu) {
  const int cus = vlm_device_cus();
  return dim3((cus <= 0 ? 256 : cus) * per_cu);
}

// The counter plan's upload: chunk_jobs_check with the method's `check`, the chunk count, the workspace size, the image.
template <class Hdr, int COUNTERS, class Job, class Check>
static inline int counts_plan_upload(const Job* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream,
                                     Check&& check) {
  const int rc = chunk_jobs_check(jobs, n_jobs, workspace, check);
  if (rc != VLM_OK) return rc;
  uint64_t n_chunks = 0;
  for (int i = 0; i < n_jobs; ++i) n_chunks += chunks_of(jobs[i].n_elem);
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  Hdr hdr;
  if (counts_layout<Hdr, Job>(&hdr, (uint64_t)n_jobs, n_chunks, COUNTERS) > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the counters begin
  return chunk_upload(workspace, chunk_image(hdr, jobs, n_jobs, hdr.counters_off), 0, (hipStream_t)stream);
}

// The counter plan's run (della.hip's too): the clear and the apply pass, two launches, stream-ordered, no host
// synchronisation -- the sizes of the plan live in the workspace header.
static inline int counts_run(void* workspace, void* stream, void (*clear_kernel)(unsigned char*),
                             void (*apply_kernel)(unsigned char*), dim3 apply_grid) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clear_kernel, dim3(64), dim3(CHUNK_THREADS), 0, s, ws);
  hipLaunchKernelGGL(apply_kernel, apply_grid, dim3(CHUNK_THREADS), 0, s, ws);
  if (hipGetLastError() != hipSuccess) return VLM_ERR_LAUNCH;
  return VLM_OK;
}

// The record plan's upload: as the counter plan's, with first[] in the image, which ends where the records begin.
template <class Hdr, class Job, class Check>
static inline int records_plan_upload(const Job* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream,
                                      size_t record_bytes, size_t result_bytes, Check&& check) {
  const int rc = chunk_jobs_check(jobs, n_jobs, workspace, check);
  if (rc != VLM_OK) return rc;
  std::vector<uint64_t> first((size_t)n_jobs + 1);
  const uint64_t n_chunks = chunk_first_fill(jobs, n_jobs, first.data());
  if (!chunk_count_ok(n_chunks)) return VLM_ERR_UNSUPPORTED;
  Hdr hdr;
  if (records_layout<Hdr, Job>(&hdr, (uint64_t)n_jobs, n_chunks, record_bytes, result_bytes) > workspace_bytes) return VLM_ERR_WORKSPACE;
  std::vector<unsigned char> img = chunk_image(hdr, jobs, n_jobs, hdr.records_off);
  memcpy(img.data() + hdr.first_off, first.data(), first.size() * sizeof(uint64_t));
  return chunk_upload(workspace, img, 0, (hipStream_t)stream);
}
#endif
