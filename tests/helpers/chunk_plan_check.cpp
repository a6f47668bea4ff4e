// Host-only check of csrc/chunk_plan.h (no HIP, no GPU): the chunk table of the merge family for the ragged sizes of
// tests/test_merge_gpu.py and for the 156 tensor lengths of a base-size all_moe -> ufo merge, the host image built around it,
// the per-job checks under each overlap policy, and what the methods share whole: chunk_first_fill, chunk_jobs_check and the
// layouts of the counter plan (dare.hip, tall.hip) and the record plan (pairstats.hip, stock.hip; sphere.hip's parts).  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_chunk_plan_cpu.py; exit status 0 = every check held.
#include "chunk_plan.h"

#include <stdio.h>
#include <string.h>
#include <vector>

struct job_t {  // the fields the family's job types share
  uint64_t n_elem;
  void* dst = nullptr;
  const void* base = nullptr;
  const void* src[VLM_MERGE_MAX_SRC] = {};
  int n_src = 0;
  job_t(uint64_t n) : n_elem(n) {}
};

struct header_t {  // a header as the methods' are: the offsets chunk_image reads, then a part of the method's own
  uint64_t n_jobs, n_chunks, jobs_off, chunks_off, own_off;
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

  // the host image around that table: 256-byte aligned parts in the order taken, nothing written outside them
  header_t h;
  chunk_layout_t at;
  CHECK(at.take(sizeof(h)) == 0, "%s: the header is not at 0", what);
  h.n_jobs = jobs.size();
  h.n_chunks = want;
  h.jobs_off = at.take(jobs.size() * sizeof(job_t));
  h.chunks_off = at.take(want * sizeof(chunk_t));
  h.own_off = at.take(100);  // what a method appends (TIES: unit0, units): left zero by the builder
  CHECK(h.jobs_off == 256 && h.chunks_off == h.jobs_off + chunk_align_up(jobs.size() * sizeof(job_t), 256) &&
            h.own_off == h.chunks_off + chunk_align_up(want * sizeof(chunk_t), 256) && at.off == h.own_off + 256,
        "%s: layout offsets", what);
  const std::vector<unsigned char> img = chunk_image(h, jobs.data(), (int)jobs.size(), at.off);
  CHECK(img.size() == at.off, "%s: image of %zu bytes, expected %zu", what, img.size(), at.off);
  CHECK(!memcmp(img.data(), &h, sizeof(h)), "%s: header bytes", what);
  CHECK(!memcmp(img.data() + h.jobs_off, jobs.data(), jobs.size() * sizeof(job_t)), "%s: job bytes", what);
  CHECK(!memcmp(img.data() + h.chunks_off, ck.data(), want * sizeof(chunk_t)), "%s: chunk table bytes", what);
  size_t stray = 0;
  for (size_t i = sizeof(h); i < h.jobs_off; ++i) stray += img[i] != 0;
  for (size_t i = h.jobs_off + jobs.size() * sizeof(job_t); i < h.chunks_off; ++i) stray += img[i] != 0;
  for (size_t i = h.chunks_off + want * sizeof(chunk_t); i < img.size(); ++i) stray += img[i] != 0;
  CHECK(stray == 0, "%s: %zu non-zero bytes between the parts", what, stray);
}

// chunk_job_check under the three overlap policies (plain merge: unchecked, TIES: no meeting, DARE: exact alias allowed)
static void check_job_checks() {
  alignas(16) static float buf[64];  // dst at buf, inputs of n = 8 floats relative to it
  const chunk_overlap_t policies[] = {CHUNK_OVERLAP_UNCHECKED, CHUNK_OVERLAP_NONE, CHUNK_OVERLAP_EXACT};
  for (chunk_overlap_t pol : policies) {
    const bool checked = pol != CHUNK_OVERLAP_UNCHECKED;
    auto job = [&](const void* base, const void* s0, const void* s1) {
      job_t j(8);
      j.dst = buf;
      j.base = base;
      j.src[0] = s0;
      j.src[1] = s1;
      j.n_src = 2;
      return j;
    };
    auto rc = [&](const job_t& j, bool need_base = true) { return chunk_job_check(j, pol, need_base); };
    CHECK(rc(job(buf + 8, buf + 16, buf + 24)) == VLM_OK, "policy %d: disjoint ranges", (int)pol);
    // equal ranges: only where exact alias is allowed (or nothing is compared)
    CHECK(rc(job(buf, buf + 16, buf + 24)) == (pol == CHUNK_OVERLAP_NONE ? VLM_ERR_ARG : VLM_OK), "policy %d: dst == base", (int)pol);
    CHECK(rc(job(buf + 8, buf + 16, buf)) == (pol == CHUNK_OVERLAP_NONE ? VLM_ERR_ARG : VLM_OK), "policy %d: dst == src[1]", (int)pol);
    // offset by 16 B either way: refused under both policies that compare
    CHECK(rc(job(buf + 4, buf + 16, buf + 24)) == (checked ? VLM_ERR_ARG : VLM_OK), "policy %d: base 16 B above dst", (int)pol);
    CHECK(rc(job(buf + 8, buf + 4, buf + 24)) == (checked ? VLM_ERR_ARG : VLM_OK), "policy %d: src[0] 16 B above dst", (int)pol);
    job_t below = job(buf + 16, buf + 24, buf);
    below.dst = buf + 4;
    CHECK(rc(below) == (checked ? VLM_ERR_ARG : VLM_OK), "policy %d: src[1] 16 B below dst", (int)pol);
    job_t touch = job(buf + 8, buf + 16, buf + 24);  // ranges that end where the next begins do not meet
    CHECK(rc(touch) == VLM_OK, "policy %d: adjacent ranges", (int)pol);
    // misaligned and null pointers
    CHECK(rc(job(buf + 9, buf + 16, buf + 24)) == VLM_ERR_ARG, "policy %d: misaligned base", (int)pol);
    CHECK(rc(job(buf + 8, buf + 17, buf + 24)) == VLM_ERR_ARG, "policy %d: misaligned src[0]", (int)pol);
    CHECK(rc(job(buf + 8, buf + 16, nullptr)) == VLM_ERR_ARG, "policy %d: null src[1]", (int)pol);
    CHECK(rc(job(nullptr, buf + 16, buf + 24)) == VLM_ERR_ARG, "policy %d: null base where one is needed", (int)pol);
    CHECK(rc(job(nullptr, buf + 16, buf + 24), false) == VLM_OK, "policy %d: null base where none is needed", (int)pol);
    job_t bad = job(buf + 8, buf + 16, buf + 24);
    bad.dst = nullptr;
    CHECK(rc(bad) == VLM_ERR_ARG, "policy %d: null dst", (int)pol);
    bad = job(buf + 8, buf + 16, buf + 24);
    bad.dst = buf + 1;
    CHECK(rc(bad) == VLM_ERR_ARG, "policy %d: misaligned dst", (int)pol);
    for (int n_src : {0, VLM_MERGE_MAX_SRC + 1}) {
      bad = job(buf + 8, buf + 16, buf + 24);
      bad.n_src = n_src;
      CHECK(rc(bad) == VLM_ERR_ARG, "policy %d: n_src = %d", (int)pol, n_src);
    }
    // the length limit; with a misaligned pointer as well, the policies that form byte ranges answer for the length first
    job_t far = job(buf + 32, buf + 40, buf + 48);  // far apart: no byte range below is formed from these lengths
    far.n_elem = (1ull << 34) - 1;
    CHECK(rc(far) == (checked ? VLM_ERR_ARG : VLM_OK), "policy %d: the longest length (its ranges meet)", (int)pol);
    far.n_elem = 1ull << 34;
    CHECK(rc(far) == VLM_ERR_UNSUPPORTED, "policy %d: one past the longest length", (int)pol);
    far.src[0] = buf + 41;
    CHECK(rc(far) == (checked ? VLM_ERR_UNSUPPORTED : VLM_ERR_ARG), "policy %d: too long and misaligned", (int)pol);
  }
}

struct counts_header_t {  // vlm_dare_header_t's and vlm_tall_header_t's fields
  uint64_t n_jobs, n_chunks, jobs_off, chunks_off, counters_off;
};
struct records_header_t {  // vlm_stock_header_t's and vlm_pairstats_header_t's fields
  uint64_t n_jobs, n_chunks, jobs_off, chunks_off, first_off, records_off, results_off;
};

// offs: every part's offset in the order taken, then the total.  256-aligned, the header at 0, and part i ends (its bytes[i],
// rounded up) exactly where part i + 1 begins: disjoint, no gap beyond the rounding.
static void check_parts(const char* what, const std::vector<size_t>& offs, const std::vector<size_t>& bytes) {
  CHECK(offs[0] == 0, "%s: the header is not at 0", what);
  for (size_t i = 0; i + 1 < offs.size(); ++i) {
    CHECK(offs[i] % 256 == 0, "%s: part %zu at %zu is not 256-aligned", what, i, offs[i]);
    CHECK(offs[i] + bytes[i] <= offs[i + 1], "%s: part %zu runs into part %zu", what, i, i + 1);
    CHECK(offs[i + 1] == offs[i] + (bytes[i] + 255) / 256 * 256, "%s: part %zu begins at %zu", what, i + 1, offs[i + 1]);
  }
}

// chunk_first_fill and the two shared layouts against the formulas each method's own *_layout had
static void check_shared_plans(const char* what, const std::vector<job_t>& jobs) {
  const int n = (int)jobs.size();
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  std::vector<uint64_t> first(jobs.size() + 1);  // exactly n + 1: the sanitizer sees a fill that runs past it
  const uint64_t c = chunk_first_fill(jobs.data(), n, first.data());
  uint64_t before = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(first[i] == before, "%s: first[%d] = %llu, expected %llu", what, i, (unsigned long long)first[i], (unsigned long long)before);
    before += chunks_of(jobs[i].n_elem);
  }
  CHECK(first[n] == before && c == before, "%s: first[n] = %llu, returned %llu, expected %llu", what, (unsigned long long)first[n],
        (unsigned long long)c, (unsigned long long)before);
  std::vector<chunk_t> ck(c);
  chunk_table_fill(ck.data(), jobs.data(), n);
  for (int i = 0; i < n; ++i)  // a job's records are its chunks: the chunk at first[i] + k is chunk k of job i
    for (uint64_t k = first[i]; k < first[i + 1]; ++k)
      CHECK(ck[k].job == (uint32_t)i && ck[k].start4 == (k - first[i]) * (CHUNK_FLOATS / 4), "%s: record %llu is not job %d's", what,
            (unsigned long long)k, i);
  // a plan whose odd jobs have no chunks (sphere_plan.h: row jobs)
  const uint64_t ce = chunk_first_fill(jobs.data(), n, first.data(),
                                       [&](const job_t& j) { return (&j - jobs.data()) % 2 ? (uint64_t)0 : chunks_of(j.n_elem); });
  before = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(first[i] == before, "%s: first[%d] with empty odd jobs", what, i);
    before += i % 2 ? 0 : chunks_of(jobs[i].n_elem);
  }
  CHECK(first[n] == before && ce == before, "%s: first[n] with empty odd jobs", what);

  const size_t head = 256 + up(n * sizeof(job_t)) + up(c * sizeof(chunk_t));  // header, jobs, chunk table
  for (int counters : {6, 10}) {  // VLM_DARE_COUNTERS == VLM_TALL_COUNTERS, and a wider set
    counts_header_t h;
    const size_t total = counts_layout<counts_header_t, job_t>(&h, n, c, counters);
    CHECK(h.n_jobs == (uint64_t)n && h.n_chunks == c, "%s: counter plan counts", what);
    check_parts(what, {0, h.jobs_off, h.chunks_off, h.counters_off, total},
                {sizeof(h), n * sizeof(job_t), c * sizeof(chunk_t), (size_t)n * counters * 8});
    CHECK(total == head + up((size_t)n * counters * 8), "%s: counter plan of %zu bytes", what, total);  // dare_layout, tall_layout
  }
  const size_t shapes[][2] = {{80, 152}, {448, 448}};  // (record, result) bytes of stock.hip and pairstats.hip
  for (const auto& rr : shapes) {
    records_header_t h;
    const size_t total = records_layout<records_header_t, job_t>(&h, n, c, rr[0], rr[1]);
    CHECK(h.n_jobs == (uint64_t)n && h.n_chunks == c, "%s: record plan counts", what);
    check_parts(what, {0, h.jobs_off, h.chunks_off, h.first_off, h.records_off, h.results_off, total},
                {sizeof(h), n * sizeof(job_t), c * sizeof(chunk_t), (size_t)(n + 1) * 8, c * rr[0], n * rr[1]});
    CHECK(total == head + up((size_t)(n + 1) * 8) + up(c * rr[0]) + up(n * rr[1]), "%s: record plan of %zu bytes", what, total);  // stock_layout, ps_layout
    // sphere.hip: the same three parts behind a tile table of its own
    records_header_t g;
    chunk_layout_t at = chunk_layout_head<records_header_t, job_t>(&g, n, c);
    const size_t tiles_off = at.take(40 * sizeof(chunk_t));
    records_parts(at, &g, rr[0], rr[1]);
    CHECK(tiles_off == h.first_off && g.first_off == h.first_off + 512 && g.records_off - g.first_off == h.records_off - h.first_off &&
              g.results_off - g.first_off == h.results_off - h.first_off && at.off == total + 512, "%s: record parts behind tiles", what);
    uint64_t elems = 0;
    for (const job_t& j : jobs) elems += j.n_elem;
    CHECK((records_plan_bytes<records_header_t, job_t>(n, elems, rr[0], rr[1]) >= total), "%s: records_plan_bytes is below the plan", what);
    CHECK((records_plan_bytes<records_header_t, job_t>(-1, elems, rr[0], rr[1]) == 0), "%s: records_plan_bytes of no plan", what);
  }
  uint64_t elems = 0;
  for (const job_t& j : jobs) elems += j.n_elem;
  counts_header_t h;
  CHECK((counts_plan_bytes<counts_header_t, job_t>(n, elems, 6) >= counts_layout<counts_header_t, job_t>(&h, n, c, 6)),
        "%s: counts_plan_bytes is below the plan", what);
  CHECK((counts_plan_bytes<counts_header_t, job_t>(-1, elems, 6) == 0), "%s: counts_plan_bytes of no plan", what);
}

// chunk_jobs_check: the arguments first, then per job "n_elem > 0" before the method's check; the first failing job decides
static void check_jobs_check() {
  alignas(16) static char ws[32];
  std::vector<job_t> jobs = {{8}, {8}, {8}};
  int asked = 0;
  auto ok = [&](const job_t&) { return ++asked, (int)VLM_OK; };
  CHECK(chunk_jobs_check(jobs.data(), 3, ws, ok) == VLM_OK && asked == 3, "jobs check: three good jobs");
  CHECK(chunk_jobs_check((const job_t*)nullptr, 3, ws, ok) == VLM_ERR_ARG, "jobs check: no jobs");
  CHECK(chunk_jobs_check(jobs.data(), 0, ws, ok) == VLM_ERR_ARG, "jobs check: n_jobs = 0");
  CHECK(chunk_jobs_check(jobs.data(), 3, ws + 4, ok) == VLM_ERR_ARG && chunk_jobs_check(jobs.data(), 3, nullptr, ok) == VLM_ERR_ARG,
        "jobs check: workspace pointer");
  asked = 0;
  auto second_unsupported = [&](const job_t& j) { return ++asked, &j == &jobs[1] ? (int)VLM_ERR_UNSUPPORTED : (int)VLM_OK; };
  CHECK(chunk_jobs_check(jobs.data(), 3, ws, second_unsupported) == VLM_ERR_UNSUPPORTED && asked == 2, "jobs check: the first failing job decides");
  jobs[0].n_elem = 0;  // an empty job is refused before its own check is asked
  asked = 0;
  CHECK(chunk_jobs_check(jobs.data(), 3, ws, second_unsupported) == VLM_ERR_ARG && asked == 0, "jobs check: n_elem = 0");
}

int main() {
  std::vector<job_t> ragged;
  for (uint64_t n : {1, 3, 5, 4095, 4096, 4097, 8195, 12289}) ragged.push_back({n});
  check_table("ragged", ragged);
  check_shared_plans("ragged", ragged);

  // base size (hidden 768, MLP 3072): the 13 output tensors of a block, 12 blocks
  const uint64_t D = 768, F = 3072;
  std::vector<job_t> base;
  for (int layer = 0; layer < 12; ++layer)
    for (uint64_t n : {3 * D * D, D * D, D, D, D, F * D, F, D * F, D, D, D, D, D}) base.push_back({n});
  CHECK(base.size() == 156, "base table has %zu jobs", base.size());
  check_table("base", base);
  check_shared_plans("base", base);

  check_job_checks();
  check_jobs_check();

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
