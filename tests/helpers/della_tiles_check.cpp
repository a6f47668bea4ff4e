// Host-only check of csrc/della_tiles.h (no HIP, no GPU): the tile table of the DELLA merge for the row shapes of
// tests/test_della_gpu.py, for plans that mix them and for the tensor shapes of a base-size merge.  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_della_cpu.py; exit status 0 = every check held.
#include "della_tiles.h"

#include <stdio.h>
#include <vector>

struct job_t {  // the fields the table reads
  uint64_t n_elem;
  uint32_t row_len;
};

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
    }                               \
  } while (0)

static void check_table(const char* what, const std::vector<job_t>& jobs) {
  uint64_t want = 0, total = 0;
  for (const job_t& j : jobs) {
    const uint64_t rows = j.n_elem / j.row_len;
    uint64_t per = 1;  // stated independently of della_tile_rows: the most whole rows within 4096 elements, at least one
    while ((per + 1) * j.row_len <= 4096) ++per;
    want += (rows + per - 1) / per;
    total += j.n_elem;
    CHECK(della_tile_rows(j.row_len) == per, "%s: %u-long rows: %u per tile, expected %llu", what, j.row_len,
          della_tile_rows(j.row_len), (unsigned long long)per);
    CHECK(della_rows_ok(j.n_elem, j.row_len), "%s: rows do not fit", what);
  }
  uint64_t counted = 0;
  for (const job_t& j : jobs) counted += della_tiles_of(j.n_elem, j.row_len);
  CHECK(counted == want, "%s: della_tiles_of sums to %llu, expected %llu", what, (unsigned long long)counted, (unsigned long long)want);
  CHECK(want <= della_tiles_bound((int)jobs.size(), total), "%s: della_tiles_bound %llu is below the count %llu", what,
        (unsigned long long)della_tiles_bound((int)jobs.size(), total), (unsigned long long)want);
  std::vector<della_tile_t> tl(want);  // exactly the count: the sanitizer sees a fill that runs past it
  const uint64_t filled = della_tile_fill(tl.data(), jobs.data(), (int)jobs.size());
  CHECK(filled == want, "%s: the fill wrote %llu records, expected %llu", what, (unsigned long long)filled, (unsigned long long)want);
  uint64_t c = 0;
  for (size_t i = 0; i < jobs.size(); ++i) {
    const uint64_t L = jobs[i].row_len, rows = jobs[i].n_elem / L, per = della_tile_rows(jobs[i].row_len);
    uint64_t covered = 0;  // the tiles of a job, in order, cover rows [0, rows) exactly once
    for (; c < want && tl[c].job == i; ++c) {
      CHECK(tl[c].start4 == covered, "%s: job %zu: gap or overlap at row %llu", what, i, (unsigned long long)covered);
      const uint64_t n = rows - covered < per ? rows - covered : per;
      CHECK(n >= 1, "%s: job %zu: an empty tile", what, i);
      CHECK(n * L <= DELLA_TILE_FLOATS || n == 1, "%s: job %zu: a tile of %llu elements", what, i, (unsigned long long)(n * L));
      CHECK(n * L <= DELLA_TILE_FLOATS, "%s: job %zu: a row longer than a tile", what, i);
      covered += n;
    }
    CHECK(covered == rows, "%s: job %zu: %llu of %llu rows covered", what, i, (unsigned long long)covered, (unsigned long long)rows);
  }
  CHECK(c == want, "%s: records left over", what);
}

int main() {
  const job_t shapes[] = {{1, 1}, {3, 3}, {15, 5}, {28, 4}, {126, 63}, {192, 64}, {130, 65}, {1275, 255}, {771, 257}, {4608, 768},
                          {6144, 3072}, {12288, 4096}, {4098, 3}, {4097, 17}, {2, 1}, {1536, 768}, {8192, 2048}, {6147, 2049},
                          {4096, 1}, {4097, 1}, {8192, 2}, {1ull << 24, 1}, {3 * 1365 * 7, 3}, {4096ull * 4096, 4096}};
  for (const job_t& j : shapes) {
    char what[64];
    snprintf(what, sizeof(what), "%llu / %u", (unsigned long long)j.n_elem, j.row_len);
    check_table(what, {j});
  }
  check_table("all shapes in one plan", std::vector<job_t>(shapes, shapes + sizeof(shapes) / sizeof(shapes[0])));
  // the block tensors of a base-size merge (width 768, hidden 3072), twelve layers: matrices by their last dimension, vectors whole
  std::vector<job_t> base;
  for (int layer = 0; layer < 12; ++layer) {
    const job_t per_layer[] = {{2304ull * 768, 768}, {768ull * 768, 768}, {768, 768}, {768, 768}, {768, 768}, {3072ull * 768, 768},
                               {3072, 3072}, {768ull * 3072, 3072}, {768, 768}, {768, 768}, {768, 768}, {768, 768}, {768, 768}};
    base.insert(base.end(), per_layer, per_layer + 13);
  }
  check_table("base size", base);
  // many one-row jobs: the bound's per-job term
  check_table("tiny jobs", std::vector<job_t>(5000, job_t{5, 5}));
  CHECK(!della_rows_ok(1ull << 32, 1) && della_rows_ok((1ull << 32) - 1, 1) && della_rows_ok(1ull << 33, 4), "della_rows_ok");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("della tiles ok\n");
  return 0;
}
