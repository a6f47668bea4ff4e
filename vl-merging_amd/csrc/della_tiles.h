// The tile table of the DELLA merge (della.hip): the rank of step 2 (include/vlm_hip.h) is a property of a ROW, so a job is cut
// into tiles of whole rows, not into chunk_plan.h's 16-KiB chunks.  A tile is as many whole rows of one job as fit in
// DELLA_TILE_FLOATS elements, at least one; the last tile of a job may hold fewer rows.  The record has chunk_t's shape, so that
// a workgroup's run over the table is chunk_walk.h's chunk_run as it is: `start4` holds the tile's FIRST ROW.
// Compiles without HIP (tests/helpers/della_tiles_check.cpp does so).
#pragma once
#include "chunk_plan.h"

#define DELLA_TILE_FLOATS 4096u  // = VLM_DELLA_MAX_ROW: one row always fits

typedef chunk_t della_tile_t;  // {job, first row}

#ifdef __HIPCC__
#define DELLA_HD __host__ __device__ __forceinline__
#else
#define DELLA_HD static inline
#endif

// rows of a full tile, for 1 <= row_len <= DELLA_TILE_FLOATS
DELLA_HD uint32_t della_tile_rows(uint32_t row_len) { return DELLA_TILE_FLOATS / row_len; }

static inline uint64_t della_tiles_of(uint64_t n_elem, uint32_t row_len) {
  const uint64_t rows = n_elem / row_len, per = della_tile_rows(row_len);
  return (rows + per - 1) / per;
}

// what vlm_della_plan_bytes reserves before the jobs are known.  A full tile holds MORE than DELLA_TILE_FLOATS / 2 elements
// (row_len <= 2048: rows x row_len > 4096 - row_len; longer rows: one row), and every job may add one partial tile.
static inline uint64_t della_tiles_bound(int n_jobs, uint64_t total_elems) {
  return total_elems / (DELLA_TILE_FLOATS / 2) + (uint64_t)n_jobs + 1;
}

// a job's rows must fit the record's 32 bits
static inline bool della_rows_ok(uint64_t n_elem, uint32_t row_len) { return n_elem / row_len < (1ull << 32); }

// `tl` receives sum_i della_tiles_of(jobs[i]) records, in job order and row order
template <class Job>
static inline uint64_t della_tile_fill(della_tile_t* tl, const Job* jobs, int n_jobs) {
  uint64_t c = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const uint64_t nt = della_tiles_of(jobs[i].n_elem, jobs[i].row_len), per = della_tile_rows(jobs[i].row_len);
    for (uint64_t k = 0; k < nt; ++k) {
      tl[c].job = (uint32_t)i;
      tl[c].start4 = (uint32_t)(k * per);
      ++c;
    }
  }
  return c;
}
