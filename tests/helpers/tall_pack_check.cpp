// Host-only use of csrc/tall_mask.h (no HIP, no GPU), built and run as a child process by tests/test_tall_cpu.py under
// AddressSanitizer + UBSan.
//   tall_pack_check pack N...   for every length N: walks the job's chunks as mask_chunk does -- 256 threads, four float4 slots per
//                               chunk and the fifth where tall_has_tail_slot says so, eight neighbouring lanes folding their nibbles
//                               into the word tall_word_of names at the shift tall_shift_of names, the ragged tail taken by the one
//                               lane that stands at n4 -- with bit i of the mask = pattern(i), into a buffer of EXACTLY
//                               ceil(N / 32) words (so a write past the end is the sanitizer's to report).  Checks that every word
//                               is written exactly once and equals the definition (element i = bit i & 31 of word i >> 5, padding
//                               zero), that every element is visited exactly once, and prints "pack N words popcount".
//   tall_pack_check check       runs tall_job_check over a fixed list of jobs and prints "check <name> <rc>" for each.
#include "tall_mask.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static bool pattern(uint64_t i) { return ((i * 2654435761ull) >> 7 & 3) != 0 || i % 97 == 0; }

static int pack(uint64_t n) {
  const uint64_t n4 = n >> 2, n_words = tall_mask_words(n);
  const uint32_t tail = (uint32_t)(n & 3);
  std::vector<uint32_t> words(n_words, 0xdeadbeefu);
  std::vector<unsigned char> written(n_words, 0), seen(n, 0);
  const uint64_t n_chunks = chunks_of(n);
  int tail_owners = 0;
  for (uint64_t ck = 0; ck < n_chunks; ++ck) {
    const uint64_t start4 = ck * (CHUNK_FLOATS / 4);
    const int slots = 4 + (tall_has_tail_slot(start4, n) ? 1 : 0);
    for (int u = 0; u < slots; ++u) {
      for (int group = 0; group < CHUNK_THREADS / 8; ++group) {
        uint32_t folded = 0;
        uint64_t word = 0;
        for (int l = 0; l < 8; ++l) {
          const uint64_t idx = start4 + (uint64_t)(group * 8 + l) + (uint64_t)u * CHUNK_THREADS;
          uint32_t nib = 0;
          if (u < 4 && idx < n4) {
            for (int c = 0; c < 4; ++c) {
              nib |= (pattern(4 * idx + c) ? 1u : 0u) << c;
              ++seen[4 * idx + c];
            }
          } else if (tail != 0 && idx == n4) {
            ++tail_owners;
            for (uint32_t t = 0; t < tail; ++t) {
              nib |= (pattern(4 * n4 + t) ? 1u : 0u) << t;
              ++seen[4 * n4 + t];
            }
          }
          if (tall_shift_of(idx) != 4u * (uint32_t)l) return fprintf(stderr, "shift of %llu\n", (unsigned long long)idx), 1;
          if (l == 0) word = tall_word_of(idx);
          else if (tall_word_of(idx) != word) return fprintf(stderr, "lanes of one group disagree on the word\n"), 1;
          folded |= nib << tall_shift_of(idx);
        }
        if (word < n_words) {
          if (written[word]++) return fprintf(stderr, "word %llu written twice\n", (unsigned long long)word), 1;
          words[word] = folded;
        } else if (folded) {
          return fprintf(stderr, "bits past the last word\n"), 1;
        }
      }
    }
  }
  if (tail_owners != (tail ? 1 : 0)) return fprintf(stderr, "n %llu: %d lanes own the tail\n", (unsigned long long)n, tail_owners), 1;
  unsigned long long pop = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (seen[i] != 1) return fprintf(stderr, "element %llu visited %d times\n", (unsigned long long)i, seen[i]), 1;
  for (uint64_t w = 0; w < n_words; ++w) {
    if (written[w] != 1) return fprintf(stderr, "word %llu never written\n", (unsigned long long)w), 1;
    uint32_t want = 0;
    for (int b = 0; b < 32; ++b)
      if (32 * w + b < n && pattern(32 * w + b)) want |= 1u << b;
    if (words[w] != want) return fprintf(stderr, "word %llu is %08x, not %08x\n", (unsigned long long)w, words[w], want), 1;
    pop += (unsigned)__builtin_popcount(want);
  }
  printf("pack %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)n_words, pop);
  return 0;
}

static vlm_tall_job_t good() {
  vlm_tall_job_t j;
  memset(&j, 0, sizeof(j));
  j.dst = (void*)0x10000;
  j.base = (const void*)0x20000;
  j.src[0] = (const void*)0x30000;
  j.src[1] = (const void*)0x40000;
  j.mask[0] = (void*)0x50000;
  j.mask[1] = (void*)0x50010;  // 100 elements: 4 words = 16 bytes per mask, so these two touch but do not meet
  j.n_elem = 100;
  j.n_src = 2;
  j.op = VLM_TALL_CONSENSUS;
  j.k = 2;
  j.tall_lambda = 0.4f;
  j.lam = 1.0f;
  return j;
}

static void show(const char* name, const vlm_tall_job_t& j) { printf("check %s %d\n", name, tall_job_check(j)); }

static int check() {
  vlm_tall_job_t j = good();
  show("good", j);
  j = good(); j.mask[0] = j.mask[1] = nullptr; show("no_masks", j);
  j = good(); j.mask[1] = nullptr; show("partial_masks", j);
  j = good(); j.mask[1] = (void*)0x50008; show("misaligned_mask", j);
  j = good(); j.mask[1] = (void*)0x50000; show("mask_is_mask", j);
  j = good(); j.n_elem = 129; show("masks_meet_at_five_words", j);   // 5 words = 20 bytes: 0x50000 .. 0x50014 meets 0x50010
  j = good(); j.mask[1] = (void*)0x10180; show("mask_in_dst", j);    // dst is 0x10000 .. 0x10190
  j = good(); j.mask[1] = (void*)0x10190; show("mask_behind_dst", j);
  j = good(); j.mask[0] = (void*)0x1fff0; show("mask_before_base", j);  // 16 bytes end exactly where the base begins
  j = good(); j.n_elem = 129; j.mask[0] = (void*)0x1fff0; show("mask_runs_into_base", j);
  j = good(); j.mask[0] = (void*)0x30100; show("mask_in_src0", j);
  j = good(); j.mask[1] = (void*)0x40000; show("mask_is_src1", j);
  j = good(); j.k = 3; show("k_above_s", j);
  j = good(); j.k = -1; show("k_negative", j);
  j = good(); j.k = 0; show("k_zero", j);
  j = good(); j.tall_lambda = -0.5f; show("lambda_negative", j);
  j = good(); j.tall_lambda = 0.0f; show("lambda_zero", j);
  j = good(); j.tall_lambda = strtof("nan", nullptr); show("lambda_nan", j);
  j = good(); j.op = 2; show("bad_op", j);
  j = good(); j.op = VLM_TALL_RESTORE; show("restore_two_sources", j);
  j = good(); j.op = VLM_TALL_RESTORE; j.n_src = 1; j.k = 0; show("restore", j);
  j = good(); j.op = VLM_TALL_RESTORE; j.n_src = 1; j.k = 0; j.mask[0] = nullptr; show("restore_no_mask", j);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "check")) return check();
  if (argc >= 3 && !strcmp(argv[1], "pack")) {
    for (int a = 2; a < argc; ++a) {
      char* end = nullptr;
      const unsigned long long n = strtoull(argv[a], &end, 10);
      if (end == argv[a] || *end != '\0' || n == 0 || n > (1ull << 26)) return fprintf(stderr, "bad length %s\n", argv[a]), 2;
      if (pack(n)) return 1;
    }
    return 0;
  }
  fprintf(stderr, "usage: tall_pack_check pack N... | tall_pack_check check\n");
  return 2;
}
