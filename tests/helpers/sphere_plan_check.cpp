// Host-only check of csrc/sphere_plan.h (no HIP, no GPU): the job checks of vlm_sphere_plan_upload and the two tables of a plan
// that mixes tensor jobs and row jobs.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_sphere_cpu.py; exit status 0 = every check held.  Every pointer of a job is fake: nothing here reads through one.
#include "sphere_plan.h"

#include <math.h>
#include <stdio.h>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
    }                               \
  } while (0)

static vlm_sphere_job_t job(uint64_t n_elem, uint32_t row_len, int n_src = 2) {
  vlm_sphere_job_t j = {};
  j.dst = (void*)0x10000000;
  j.base = (const void*)0x20000000;
  for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) {
    j.src[m] = (const void*)(uintptr_t)(0x30000000 + 0x10000000 * (uintptr_t)m);
    j.w[m] = 1.0 + m;
  }
  j.n_elem = n_elem;
  j.row_len = row_len;
  j.n_src = n_src;
  j.lam = 1.0f;
  return j;
}

// the tables of a plan: every tensor job's chunks cover its float4s once, every row job's tiles its rows once, in job order,
// each table exactly as long as sphere_count says (the vectors are exactly that long: the sanitizer sees a fill that runs past)
static void check_plan(const char* what, const std::vector<vlm_sphere_job_t>& jobs) {
  const int n = (int)jobs.size();
  uint64_t total = 0;
  for (const vlm_sphere_job_t& j : jobs) {
    CHECK(sphere_job_check(j) == VLM_OK, "%s: a job of %llu / %u fails its checks", what, (unsigned long long)j.n_elem, j.row_len);
    total += j.n_elem;
  }
  std::vector<uint64_t> first((size_t)n + 1, ~0ull);
  uint64_t n_chunks = ~0ull, n_tiles = ~0ull;
  sphere_count(jobs.data(), n, first.data(), &n_chunks, &n_tiles);
  CHECK(first[n] == n_chunks, "%s: first[n_jobs] is not the chunk count", what);
  CHECK(n_chunks <= chunks_bound(n, total) && n_tiles <= della_tiles_bound(n, total), "%s: a table outgrows what plan_bytes reserves", what);
  std::vector<chunk_t> ck(n_chunks);
  std::vector<della_tile_t> tl(n_tiles);
  sphere_tables_fill(ck.data(), tl.data(), jobs.data(), n);
  uint64_t c = 0, t = 0;
  for (int i = 0; i < n; ++i) {
    const vlm_sphere_job_t& j = jobs[i];
    CHECK(first[i] == c, "%s: job %d: first chunk %llu, expected %llu", what, i, (unsigned long long)first[i], (unsigned long long)c);
    if (j.row_len == 0) {
      uint64_t at = 0;
      int tails = 0;
      for (; c < n_chunks && ck[c].job == (uint32_t)i; ++c) {
        CHECK(ck[c].start4 == at, "%s: job %d: gap or overlap at float4 %llu", what, i, (unsigned long long)at);
        tails += chunk_owns_tail(ck[c].start4, j.n_elem) ? 1 : 0;
        at += CHUNK_FLOATS / 4;
      }
      CHECK(at == chunks_of(j.n_elem) * (CHUNK_FLOATS / 4) && at >= (j.n_elem >> 2), "%s: job %d: chunks up to float4 %llu of %llu", what,
            i, (unsigned long long)at, (unsigned long long)(j.n_elem >> 2));
      CHECK(tails == 1, "%s: job %d: %d chunks own the ragged tail", what, i, tails);
    } else {
      const uint64_t rows = j.n_elem / j.row_len, per = della_tile_rows(j.row_len);
      uint64_t covered = 0;
      for (; t < n_tiles && tl[t].job == (uint32_t)i; ++t) {
        CHECK(tl[t].start4 == covered, "%s: job %d: gap or overlap at row %llu", what, i, (unsigned long long)covered);
        const uint64_t r = rows - covered < per ? rows - covered : per;
        CHECK(r >= 1 && r * j.row_len <= DELLA_TILE_FLOATS, "%s: job %d: a tile of %llu rows", what, i, (unsigned long long)r);
        covered += r;
      }
      CHECK(covered == rows, "%s: job %d: %llu of %llu rows covered", what, i, (unsigned long long)covered, (unsigned long long)rows);
    }
  }
  CHECK(c == n_chunks && t == n_tiles, "%s: records left over", what);
}

static void expect(const char* what, const vlm_sphere_job_t& j, int want) {
  const int got = sphere_job_check(j);
  CHECK(got == want, "%s: sphere_job_check gives %d, expected %d", what, got, want);
}

int main() {
  // the shapes of tests/test_sphere_gpu.py, each alone, then all in one plan, tensor and row jobs in turn
  const uint64_t sizes[] = {1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 70001};
  const uint32_t lens[] = {1, 3, 4, 64, 65, 768, 4096};
  std::vector<vlm_sphere_job_t> all;
  for (uint64_t n : sizes) {
    check_plan("a tensor job", {job(n, 0)});
    all.push_back(job(n, 0, 1 + (int)(n % 4)));
  }
  for (uint32_t L : lens) {
    const uint64_t per = 4096 / L;
    for (uint64_t rows : {(uint64_t)1, (uint64_t)2, per, per + 1, 2 * per + 3}) {
      check_plan("a row job", {job(rows * L, L)});
      all.push_back(job(rows * L, L, 1 + (int)(rows % 4)));
      all.push_back(job(rows * L + 1, 0));
    }
  }
  check_plan("all shapes in one plan", all);
  check_plan("row jobs first", {job(768 * 5, 768), job(3, 3), job(4097, 0), job(65 * 64, 65)});
  // the block tensors of a base-size merge, twelve layers, by tensor and by row
  for (int by_row = 0; by_row < 2; ++by_row) {
    std::vector<vlm_sphere_job_t> base;
    for (int layer = 0; layer < 12; ++layer) {
      const uint64_t shapes[][2] = {{2304ull * 768, 768}, {768ull * 768, 768}, {768, 768}, {768, 768}, {768, 768}, {3072ull * 768, 768},
                                    {3072, 3072}, {768ull * 3072, 3072}, {768, 768}, {768, 768}, {768, 768}, {768, 768}, {768, 768}};
      for (const auto& s : shapes) base.push_back(job(s[0], by_row ? (uint32_t)s[1] : 0, layer < 10 ? 2 : 3));
    }
    check_plan(by_row ? "base size by row" : "base size by tensor", base);
  }
  check_plan("tiny jobs", std::vector<vlm_sphere_job_t>(3000, job(5, 5)));

  // the checks of a job
  vlm_sphere_job_t j = job(64, 0);
  expect("a good job", j, VLM_OK);
  j = job(64, 0); j.base = nullptr;                       expect("no base", j, VLM_OK);
  j = job(64, 0); j.base = nullptr; j.lam = 0.5f;         expect("lam without a base", j, VLM_ERR_ARG);
  j = job(64, 0); j.lam = 0.5f;                           expect("lam with a base", j, VLM_OK);
  j = job(64, 0); j.w[0] = -1.0;                          expect("a negative weight", j, VLM_ERR_ARG);
  j = job(64, 0); j.w[1] = NAN;                           expect("a NaN weight", j, VLM_ERR_ARG);
  j = job(64, 0); j.w[1] = INFINITY;                      expect("an infinite weight", j, VLM_ERR_ARG);
  j = job(64, 0); j.w[0] = j.w[1] = 0.0;                  expect("weights all zero", j, VLM_ERR_ARG);
  j = job(64, 0); j.w[0] = 0.0;                           expect("one zero weight", j, VLM_OK);
  j = job(64, 0); j.w[3] = -1.0;                          expect("the weight of a source the job lacks", j, VLM_OK);
  j = job(64, 5);                                         expect("a row length that does not divide", j, VLM_ERR_ARG);
  j = job(8194, 4097);                                    expect("a row longer than a tile", j, VLM_ERR_ARG);
  j = job(64, 64);                                        expect("one row", j, VLM_OK);
  j = job(0, 0);                                          expect("no elements", j, VLM_ERR_ARG);
  j = job(64, 0); j.n_src = 5;                            expect("five sources", j, VLM_ERR_ARG);
  j = job(64, 0); j.dst = (void*)0x20000080;              expect("dst inside the base", j, VLM_ERR_ARG);
  j = job(1ull << 34, 0);                                 expect("too long", j, VLM_ERR_UNSUPPORTED);
  j = job((1ull << 32) * 1, 1); j.dst = (void*)(1ull << 60);  expect("too many rows", j, VLM_ERR_UNSUPPORTED);
  j = job(64, 0); j.coef_out = (void*)0x50000000;         expect("coef_out apart", j, VLM_OK);
  j = job(64, 0); j.coef_out = (void*)0x50000004;         expect("coef_out misaligned", j, VLM_ERR_ARG);
  j = job(64, 0); j.coef_out = (void*)0x100000f0;         expect("coef_out inside dst", j, VLM_ERR_ARG);
  j = job(64, 0); j.coef_out = (void*)0x0ffffff0;         expect("coef_out ends where dst begins", j, VLM_OK);
  j = job(64, 16); j.coef_out = (void*)0x0fffffc0;        expect("four rows of coefficients end where dst begins", j, VLM_OK);
  j = job(64, 16); j.coef_out = (void*)0x0fffffd0;        expect("four rows of coefficients reach into dst", j, VLM_ERR_ARG);
  j = job(64, 16); j.coef_out = (void*)0x400000f0;        expect("coef_out inside the second source", j, VLM_ERR_ARG);
  j = job(64, 16, 1); j.coef_out = (void*)0x400000f0;     expect("coef_out inside a source the job lacks", j, VLM_OK);
  CHECK(sphere_ranges_meet((void*)0x100, 16, (void*)0x110, 16) == false && sphere_ranges_meet((void*)0x100, 17, (void*)0x110, 16) &&
            sphere_ranges_meet((void*)0x110, 16, (void*)0x100, 17) && !sphere_ranges_meet((void*)0x110, 16, (void*)0x100, 16),
        "sphere_ranges_meet");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("sphere_plan_check: ok\n");
  return 0;
}
