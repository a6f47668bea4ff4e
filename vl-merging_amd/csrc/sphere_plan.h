// The host side of a spherical plan (sphere.hip) that needs no HIP: the checks a job passes beyond the family's
// (chunk_job_check), and the two tables of a plan that may mix tensor jobs (row_len == 0: chunk_plan.h's 16-KiB chunks) and row
// jobs (della_tiles.h's tiles of whole rows) -- each table lists the jobs of its kind alone, under their index in the plan.
// Compiles without HIP (tests/helpers/sphere_plan_check.cpp does so).
#pragma once
#include "chunk_plan.h"
#include "della_tiles.h"

// do the byte ranges [a, a + la) and [b, b + lb) meet?
static inline bool sphere_ranges_meet(const void* a, uint64_t la, const void* b, uint64_t lb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? (y - x) < la : (x - y) < lb;
}

// groups of a job: its rows, or one
static inline uint64_t sphere_groups(const vlm_sphere_job_t& j) { return j.row_len ? j.n_elem / j.row_len : 1; }

// Every check of vlm_sphere_plan_upload on one job, in its order of precedence: VLM_OK, VLM_ERR_ARG or VLM_ERR_UNSUPPORTED.
static inline int sphere_job_check(const vlm_sphere_job_t& j) {
  if (j.n_elem == 0) return VLM_ERR_ARG;
  const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, false);  // the inputs are read twice (tensor) or kept (rows): dst meets none
  if (rc != VLM_OK) return rc;
  double sum = 0.0;
  for (int m = 0; m < j.n_src; ++m) {
    if (!(j.w[m] >= 0.0) || !(j.w[m] <= 1.7976931348623157e308)) return VLM_ERR_ARG;  // negative, NaN or infinite
    sum += j.w[m];
  }
  if (!(sum > 0.0)) return VLM_ERR_ARG;
  if (!j.base && j.lam != 1.0f) return VLM_ERR_ARG;
  if (j.row_len != 0 && (j.row_len > VLM_DELLA_MAX_ROW || j.n_elem % j.row_len != 0)) return VLM_ERR_ARG;
  if (j.row_len != 0 && !della_rows_ok(j.n_elem, j.row_len)) return VLM_ERR_UNSUPPORTED;
  if (j.coef_out) {
    const uint64_t cb = sphere_groups(j) * VLM_MERGE_MAX_SRC * sizeof(float), nb = j.n_elem * 4;
    if (!chunk_ptr_ok(j.coef_out) || sphere_ranges_meet(j.coef_out, cb, j.dst, nb) ||
        (j.base && sphere_ranges_meet(j.coef_out, cb, j.base, nb)))
      return VLM_ERR_ARG;
    for (int m = 0; m < j.n_src; ++m)
      if (sphere_ranges_meet(j.coef_out, cb, j.src[m], nb)) return VLM_ERR_ARG;
  }
  return VLM_OK;
}

// first[i] = the first chunk of job i (a row job has none: first[i] == first[i + 1]), first[n_jobs] = *n_chunks; *n_tiles = the
// row jobs' tiles.  The jobs have passed sphere_job_check.
static inline void sphere_count(const vlm_sphere_job_t* jobs, int n_jobs, uint64_t* first, uint64_t* n_chunks, uint64_t* n_tiles) {
  *n_chunks = chunk_first_fill(jobs, n_jobs, first,
                               [](const vlm_sphere_job_t& j) { return j.row_len == 0 ? chunks_of(j.n_elem) : (uint64_t)0; });
  *n_tiles = 0;
  for (int i = 0; i < n_jobs; ++i)
    if (jobs[i].row_len != 0) *n_tiles += della_tiles_of(jobs[i].n_elem, jobs[i].row_len);
}

// chunk_table_fill's records for the tensor jobs into `ck`, della_tile_fill's for the row jobs into `tl`, each in job order
static inline void sphere_tables_fill(chunk_t* ck, della_tile_t* tl, const vlm_sphere_job_t* jobs, int n_jobs) {
  uint64_t c = 0, t = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_sphere_job_t& j = jobs[i];
    if (j.row_len == 0) {
      for (uint64_t k = 0, nc = chunks_of(j.n_elem); k < nc; ++k, ++c) ck[c] = {(uint32_t)i, (uint32_t)(k * (CHUNK_FLOATS / 4))};
    } else {
      const uint64_t per = della_tile_rows(j.row_len);
      for (uint64_t k = 0, nt = della_tiles_of(j.n_elem, j.row_len); k < nt; ++k, ++t) tl[t] = {(uint32_t)i, (uint32_t)(k * per)};
    }
  }
}
