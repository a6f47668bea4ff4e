// Host-side checks of what csrc/emr.hip takes from csrc/tall_mask.h and csrc/chunk_plan.h, compiled WITHOUT HIP as a stand-alone
// program (tests/test_emr_cpu.py builds it with -fsanitize=address,undefined).
//   emr_plan_check tail N...   walks the slots of every chunk of a job of N elements as mask_chunk does and prints, per N,
//                              "tail N chunk thread slot": which chunk, thread and slot stand at the partial float4 n4 = N >> 2.
//                              Exactly one place does when N & 3 != 0 (else the line says "tail N none"); it must be the job's last
//                              chunk and thread n4 & 255 -- the rule's step 6 -- and every slot of that thread behind it lies past
//                              the end, so the tail's addends come after the thread's float4s.
//   emr_plan_check check       the verdicts of the upload's per-job check (chunk_job_check, then emr_job_check) on a fixed list.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "tall_mask.h"

static int tail(uint64_t n) {
  const uint64_t n4 = n >> 2, nc = chunks_of(n);
  const uint32_t tl = (uint32_t)(n & 3);
  int found = 0;
  uint64_t at_chunk = 0;
  uint32_t at_thread = 0;
  int at_slot = 0;
  for (uint64_t c = 0; c < nc; ++c) {
    const uint64_t start4 = c * (CHUNK_FLOATS / 4);
    const int slots = tall_has_tail_slot(start4, n) ? 5 : 4;
    for (int u = 0; u < slots; ++u)
      for (uint32_t t = 0; t < CHUNK_THREADS; ++t) {
        const uint64_t idx = start4 + t + (uint64_t)u * CHUNK_THREADS;
        const bool have = u < 4 && idx < n4;
        if (!have && tl != 0 && idx == n4) {  // mask_slot's at_tail
          ++found;
          at_chunk = c;
          at_thread = t;
          at_slot = u;
          if (!chunk_owns_tail(start4, n)) return fprintf(stderr, "%llu: the tail stands in a chunk that does not own it\n", (unsigned long long)n), 1;
          for (int v = u + 1; v < 4; ++v)
            if (start4 + t + (uint64_t)v * CHUNK_THREADS < n4) return fprintf(stderr, "%llu: a float4 behind the tail\n", (unsigned long long)n), 1;
          if (tall_word_of(idx) != tall_mask_words(n) - 1) return fprintf(stderr, "%llu: the tail is not in the last word\n", (unsigned long long)n), 1;
        }
      }
  }
  if (found != (tl ? 1 : 0)) return fprintf(stderr, "%llu: %d places stand at the tail\n", (unsigned long long)n, found), 1;
  if (!tl) return printf("tail %llu none\n", (unsigned long long)n), 0;
  if (at_chunk != nc - 1 || at_thread != (uint32_t)(n4 & (CHUNK_THREADS - 1)))
    return fprintf(stderr, "%llu: chunk %llu thread %u\n", (unsigned long long)n, (unsigned long long)at_chunk, at_thread), 1;
  printf("tail %llu %llu %u %d\n", (unsigned long long)n, (unsigned long long)at_chunk, at_thread, at_slot);
  return 0;
}

static vlm_emr_job_t good() {
  vlm_emr_job_t j;
  memset(&j, 0, sizeof(j));
  j.dst = (void*)0x10000;
  j.base = (const void*)0x20000;
  j.src[0] = (const void*)0x30000;
  j.src[1] = (const void*)0x40000;
  j.mask[0] = (void*)0x50000;
  j.mask[1] = (void*)0x50010;  // 100 elements: 4 words = 16 bytes per mask, so these two touch but do not meet
  j.n_elem = 100;
  j.n_src = 2;
  j.op = VLM_EMR_MERGE;
  j.lam = 1.0f;
  return j;
}

static vlm_emr_job_t good_restore() {
  vlm_emr_job_t j = good();
  j.op = VLM_EMR_RESTORE;
  j.n_src = 1;
  j.rescale = 1.7f;
  return j;
}

static void show(const char* name, const vlm_emr_job_t& j) {
  const int rc = chunk_job_check(j, CHUNK_OVERLAP_EXACT, true);
  printf("check %s %d\n", name, rc == VLM_OK ? emr_job_check(j) : rc);
}

static int check() {
  vlm_emr_job_t j = good();
  show("good", j);
  j = good(); j.mask[0] = j.mask[1] = nullptr; show("no_masks", j);
  j = good(); j.mask[1] = nullptr; show("partial_masks", j);
  j = good(); j.mask[1] = (void*)0x50008; show("misaligned_mask", j);
  j = good(); j.mask[1] = (void*)0x50000; show("mask_is_mask", j);
  j = good(); j.n_elem = 129; show("masks_meet_at_five_words", j);
  j = good(); j.mask[0] = (void*)0x10000; show("mask_is_dst", j);
  j = good(); j.mask[1] = (void*)0x10190; show("mask_behind_dst", j);
  j = good(); j.mask[0] = (void*)0x30100; show("mask_in_src0", j);
  j = good(); j.mask[1] = (void*)0x40000; show("mask_is_src1", j);
  j = good(); j.dst = (void*)0x20000; show("dst_is_base", j);
  j = good(); j.dst = (void*)0x40000; show("dst_is_src1", j);
  j = good(); j.dst = (void*)0x20010; show("dst_inside_base", j);
  j = good(); j.base = nullptr; show("no_base", j);
  j = good(); j.op = 2; show("bad_op", j);
  j = good(); j.rescale = strtof("nan", nullptr); show("merge_ignores_rescale", j);
  j = good(); j.op = VLM_EMR_RESTORE; show("restore_two_sources", j);
  j = good_restore(); show("restore", j);
  j = good_restore(); j.rescale = 0.0f; show("restore_zero", j);
  j = good_restore(); j.mask[0] = nullptr; show("restore_no_mask", j);
  j = good_restore(); j.rescale = strtof("nan", nullptr); show("restore_nan", j);
  j = good_restore(); j.rescale = -0.5f; show("restore_negative", j);
  j = good_restore(); j.rescale = INFINITY; show("restore_infinite", j);
  j = good_restore(); j.dst = (void*)0x30000; show("restore_in_place", j);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "check")) return check();
  if (argc >= 3 && !strcmp(argv[1], "tail")) {
    for (int a = 2; a < argc; ++a) {
      char* end = nullptr;
      const unsigned long long n = strtoull(argv[a], &end, 10);
      if (end == argv[a] || *end != '\0' || n == 0 || n > (1ull << 28)) return fprintf(stderr, "bad length %s\n", argv[a]), 2;
      if (tail(n)) return 1;
    }
    return 0;
  }
  fprintf(stderr, "usage: emr_plan_check tail N... | emr_plan_check check\n");
  return 2;
}
