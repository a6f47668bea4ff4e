// The packed masks of the consensus merge (tall.hip) and of EMR-Merging (emr.hip): where an element's bit lives, and the checks
// vlm_tall_plan_upload and vlm_emr_plan_upload make on a job's op, scalars and mask pointers.  A mask of n elements is ceil(n / 32) 32-bit words; element i is bit (i & 31) of word
// i >> 5, bit 0 the least significant; the bits at positions >= n of the last word are zero.
// The streaming pass moves float4s, so it sees a mask as nibbles: float4 idx4 (elements 4 idx4 .. 4 idx4 + 3) is nibble idx4 & 7 of
// word idx4 >> 3.  A 16-KiB chunk starts at a multiple of 1024 float4s and thread t takes float4 start4 + t + 256 u, so the eight
// lanes t & ~7 .. t | 7 of a wave hold the eight nibbles of ONE word, in order.  The ragged tail (n & 3 elements) is the partial
// float4 n4 = n >> 2: nibble n4 & 7 of word n4 >> 3, which is the tensor's last word.
// Compiles without HIP (tests/helpers/tall_pack_check.cpp does so); the device body that walks a chunk by these rules is
// mask_chunk.h's.
#pragma once
#include "chunk_plan.h"

CHUNK_HD uint64_t tall_mask_words(uint64_t n_elem) { return (n_elem + 31) >> 5; }
CHUNK_HD uint64_t tall_word_of(uint64_t idx4) { return idx4 >> 3; }
CHUNK_HD uint32_t tall_shift_of(uint64_t idx4) { return 4u * (uint32_t)(idx4 & 7); }

// The float4 slots a chunk walks: u = 0 .. 3 are its own (chunk_walk.h); slot 4 exists only in the chunk that owns a ragged tail
// whose partial float4 n4 lies just behind the chunk's last float4 (n4 a positive multiple of 1024): there thread 0 stands at n4.
CHUNK_HD bool tall_has_tail_slot(uint64_t start4, uint64_t n_elem) {
  return chunk_tail_len(start4, n_elem) != 0 && (n_elem >> 2) == start4 + CHUNK_FLOATS / 4;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet?
static inline bool tall_bytes_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? (y - x) < na : (x - y) < nb;
}

// What a job with packed masks (fields dst, base, src, mask, n_src, n_elem: tall.hip's and emr.hip's) is asked about them.
// `restore`: the job reads ONE mask -- one source and its mask; otherwise it writes them -- no mask or one per source.  Every mask
// 16-byte aligned and its 4 ceil(n / 32) bytes clear of dst, the base, every source and every other mask of the job.  Call it
// after chunk_job_check: the length is known to be in range.
template <class Job>
static inline int tall_masks_check(const Job& j, bool restore) {
  int n_mask = 0;
  for (int m = 0; m < j.n_src; ++m) n_mask += j.mask[m] ? 1 : 0;
  if (restore ? (j.n_src != 1 || n_mask != 1) : (n_mask != 0 && n_mask != j.n_src)) return VLM_ERR_ARG;
  const uint64_t mb = 4 * tall_mask_words(j.n_elem), tb = 4 * j.n_elem;
  for (int m = 0; m < j.n_src && n_mask; ++m) {
    const void* p = j.mask[m];
    if (!chunk_ptr_ok(p)) return VLM_ERR_ARG;
    if (tall_bytes_meet(p, mb, j.dst, tb) || (j.base && tall_bytes_meet(p, mb, j.base, tb))) return VLM_ERR_ARG;
    for (int s = 0; s < j.n_src; ++s)
      if (tall_bytes_meet(p, mb, j.src[s], tb)) return VLM_ERR_ARG;
    for (int o = 0; o < m; ++o)
      if (tall_bytes_meet(p, mb, j.mask[o], mb)) return VLM_ERR_ARG;
  }
  return VLM_OK;
}

// What vlm_tall_plan_upload asks of a job beyond chunk_job_check: a valid op, k in [0, n_src], tall_lambda >= 0 (a NaN fails the
// comparison), then tall_masks_check.
template <class Job>
static inline int tall_job_check(const Job& j) {
  if (j.op != VLM_TALL_CONSENSUS && j.op != VLM_TALL_RESTORE) return VLM_ERR_ARG;
  if (j.k < 0 || j.k > j.n_src || !(j.tall_lambda >= 0.0f)) return VLM_ERR_ARG;
  return tall_masks_check(j, j.op == VLM_TALL_RESTORE);
}

// What vlm_emr_plan_upload asks of a job beyond chunk_job_check: a valid op; RESTORE: a rescale that is finite and >= 0 (a NaN
// fails both comparisons); then tall_masks_check.
template <class Job>
static inline int emr_job_check(const Job& j) {
  if (j.op != VLM_EMR_MERGE && j.op != VLM_EMR_RESTORE) return VLM_ERR_ARG;
  if (j.op == VLM_EMR_RESTORE && !(j.rescale >= 0.0f && j.rescale <= 3.402823466e+38f)) return VLM_ERR_ARG;
  return tall_masks_check(j, j.op == VLM_EMR_RESTORE);
}
