// Host-only check of csrc/chunk_plan.h (no HIP, no GPU): the chunk table of the merge family for the ragged sizes of
// tests/test_merge_gpu.py and for the 156 tensor lengths of a base-size all_moe -> ufo merge.  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_chunk_plan_cpu.py; exit status 0 = every check held.
#include "chunk_plan.h"

#include <stdio.h>
#include <vector>

struct job_t {
  uint64_t n_elem;
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
  const uint64_t per = CHUNK_FLOATS / 4;  // float4 per chunk
  uint64_t want = 0, total = 0;
  for (const job_t& j : jobs) {
    const uint64_t n4 = j.n_elem / 4;
    want += n4 == 0 ? 1 : (n4 + per - 1) / per;  // stated independently of chunks_of
    total += j.n_elem;
  }
  uint64_t counted = 0;
  for (const job_t& j : jobs) counted += chunks_of(j.n_elem);
  CHECK(counted == want, "%s: chunks_of sums to %llu, expected %llu", what, (unsigned long long)counted, (unsigned long long)want);
  CHECK(want <= chunks_bound((int)jobs.size(), total), "%s: chunks_bound is below the count", what);
  std::vector<chunk_t> ck(want);  // exactly the count: the sanitizer sees a fill that runs past it
  const uint64_t filled = chunk_table_fill(ck.data(), jobs.data(), (int)jobs.size());
  CHECK(filled == want, "%s: the fill wrote %llu records, expected %llu", what, (unsigned long long)filled, (unsigned long long)want);
  uint64_t c = 0;
  for (size_t i = 0; i < jobs.size(); ++i) {
    const uint64_t n = jobs[i].n_elem, n4 = n / 4;
    uint64_t covered = 0;  // the chunks of a job, in order, cover [0, n4) exactly once
    int owners = 0;
    uint32_t tail = 0;
    for (uint64_t k = 0; c < want && ck[c].job == i; ++k, ++c) {
      CHECK(ck[c].start4 == k * per, "%s: job %zu chunk %llu starts at %u", what, i, (unsigned long long)k, ck[c].start4);
      CHECK(ck[c].start4 == covered, "%s: job %zu: gap or overlap at float4 %llu", what, i, (unsigned long long)covered);
      const uint64_t end = ck[c].start4 + per < n4 ? ck[c].start4 + per : n4;
      covered = end;
      if (chunk_owns_tail(ck[c].start4, n)) ++owners;
      tail += chunk_tail_len(ck[c].start4, n);
    }
    CHECK(covered == n4, "%s: job %zu (n = %llu): %llu of %llu float4 covered", what, i, (unsigned long long)n,
          (unsigned long long)covered, (unsigned long long)n4);
    CHECK(owners == 1, "%s: job %zu (n = %llu): %d chunks own the tail", what, i, (unsigned long long)n, owners);
    CHECK(tail == n % 4, "%s: job %zu (n = %llu): %u tail floats handled", what, i, (unsigned long long)n, tail);
  }
  CHECK(c == want, "%s: %llu records belong to no job", what, (unsigned long long)(want - c));
}

int main() {
  std::vector<job_t> ragged;
  for (uint64_t n : {1, 3, 5, 4095, 4096, 4097, 8195, 12289}) ragged.push_back({n});
  check_table("ragged", ragged);

  // base size (hidden 768, MLP 3072): the 13 output tensors of a block, 12 blocks
  const uint64_t D = 768, F = 3072;
  std::vector<job_t> base;
  for (int layer = 0; layer < 12; ++layer)
    for (uint64_t n : {3 * D * D, D * D, D, D, D, F * D, F, D * F, D, D, D, D, D}) base.push_back({n});
  CHECK(base.size() == 156, "base table has %zu jobs", base.size());
  check_table("base", base);

  // the common checks
  alignas(16) static char buf[32];
  CHECK(chunk_ptr_ok(buf) && !chunk_ptr_ok(buf + 4) && !chunk_ptr_ok(nullptr), "chunk_ptr_ok");
  CHECK(chunk_len_ok((1ull << 34) - 1) && !chunk_len_ok(1ull << 34), "chunk_len_ok");
  CHECK(chunk_count_ok((1ull << 32) - 1) && !chunk_count_ok(1ull << 32), "chunk_count_ok");
  CHECK(chunk_align_up(1, 256) == 256 && chunk_align_up(256, 256) == 256 && chunk_align_up(0, 256) == 0, "chunk_align_up");
  if (failures) fprintf(stderr, "%d checks failed\n", failures);
  else printf("chunk plan ok\n");
  return failures ? 1 : 0;
}
