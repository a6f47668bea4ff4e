// The chunk body of the methods whose streaming pass has a bit-packed side (tall.hip, emr.hip), stated once: a method's file
// holds its rule per element and what it gathers.  Device code only; where an element's bit lives and the checks on a job's masks
// are tall_mask.h's, which compiles without HIP.
// The body is not chunk_stream (chunk_walk.h): the mask words need the lanes of a wave to talk to each other, and chunk_stream
// computes under `if (idx < n4)`.  Here a float4 SLOT is walked by the whole workgroup: a lane whose float4 lies past the end
// computes nothing and contributes a zero nibble, and the eight lanes that hold one word's nibbles (tall_mask.h) fold them with
// three __shfl_xor steps that every lane of the wave executes.  The ragged tail is not a separate path of threads 0 .. 2: it is
// the partial float4 n4, handled by the ONE lane that stands at n4, so its bits enter the same fold as its neighbours' and the
// tensor's last word -- float4 lanes, tail bits, zero padding -- is written once, by one lane; what the rule gathers for the
// tail's elements enters THAT lane's state, behind its float4s (every later slot of the lane lies past the end), in element
// order.  Where n4 lies just behind the tail chunk's last float4 the chunk walks a fifth slot for it (tall_has_tail_slot).
// A mask word is stored with a plain store, not a non-temporal one: a wave's eight words are 32 B and the four waves of a
// workgroup fill one 128-B line between them, which L2 puts together when the words may stay there; streamed past it they cost
// 9 % of the pass instead of 2 % (docs/experiments.md, "Consensus merge").
#pragma once
#include "chunk_walk.h"  // chunk_stream, whose loads these are
#include "tall_mask.h"

// what a chunk does, a compile-time constant of its body
#define MASK_PLAIN 0     // the merge without masks
#define MASK_WRITE 1     // the merge, one mask per source written
#define MASK_RESTORE 2   // the restore: one source, one mask read

// A method hands the body a Rule that carries its state (a job's scalars, the thread's counters and sums) by reference:
//   float elem(float c, const float* w, uint32_t& bits)   the merge of one element with base c and sources w[0 .. NSRC); bit m of
//                                                         `bits` = what source m's mask says of the element
//   float pick(bool bit, float u, float c)                the restore of one element from its mask bit, the unified value u and c

// A kernel picks the kind from the job: RESTORE by its op, with NSRC = 1; otherwise WRITE iff the job has mask[0].

// One float4 slot of a chunk, entered by EVERY thread of the workgroup.  `have`: float4 idx lies inside the tensor and v (one
// float4 per source) and b (the base) hold it.  The lane with idx == n4 of a tensor with a ragged tail handles the tail's
// elements 4 n4 + t, t < tail, as the partial float4 it is.  Every other lane past the end does nothing but take part in the
// cross-lane steps, with zero bits.
template <int NSRC, int KIND, class Job, class Rule>
__device__ __forceinline__ void mask_slot(const Job& j, uint64_t idx, uint64_t n4, uint32_t tail, uint64_t n_words, bool have,
                                          const f32x4* v, const f32x4& b, Rule& rule) {
  const int lane = threadIdx.x & 63;
  const uint64_t word = tall_word_of(idx);
  const uint32_t shift = tall_shift_of(idx);   // == 4 (lane & 7): a chunk starts at a multiple of 8 float4s
  const bool leader = (lane & 7) == 0 && word < n_words;
  uint32_t nib[NSRC];                          // the merge: bit c of nib[m] = source m's bit of element c of this float4
#pragma unroll
  for (int m = 0; m < NSRC; ++m) nib[m] = 0;
  if (KIND == MASK_RESTORE) {
    // the leader reads the word once for the 32 elements of its eight lanes -- and only a word the mask has
    uint32_t w = 0;
    if (leader) w = __builtin_nontemporal_load(&reinterpret_cast<const uint32_t*>(j.mask[0])[word]);
    w = __shfl(w, lane & ~7, 64);
    nib[0] = (w >> shift) & 15u;
  }
  const bool at_tail = !have && tail != 0 && idx == n4;
  if (have) {
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (KIND == MASK_RESTORE) {
        o[c] = rule.pick((nib[0] >> c) & 1u, v[0][c], b[c]);
      } else {
        float w[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) w[m] = v[m][c];
        uint32_t bits;
        o[c] = rule.elem(b[c], w, bits);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((bits >> m) & 1u) << c;
      }
    }
    __builtin_nontemporal_store(o, &reinterpret_cast<f32x4*>(j.dst)[idx]);
  } else if (at_tail) {
    for (uint32_t t = 0; t < tail; ++t) {
      const uint64_t i = (n4 << 2) + t;  // < n_elem
      float w[NSRC];
#pragma unroll
      for (int m = 0; m < NSRC; ++m) w[m] = reinterpret_cast<const float*>(j.src[m])[i];
      const float bt = reinterpret_cast<const float*>(j.base)[i];
      float o;
      if (KIND == MASK_RESTORE) {
        o = rule.pick((nib[0] >> t) & 1u, w[0], bt);
      } else {
        uint32_t bits;
        o = rule.elem(bt, w, bits);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) nib[m] |= ((bits >> m) & 1u) << t;
      }
      reinterpret_cast<float*>(j.dst)[i] = o;
    }
  }
  if (KIND == MASK_WRITE) {
    // the whole wave active: eight nibbles -> one word in every lane of the eight; the leader stores it, with a plain store
#pragma unroll
    for (int m = 0; m < NSRC; ++m) {
      uint32_t w = nib[m] << shift;
      w |= __shfl_xor(w, 1, 64);
      w |= __shfl_xor(w, 2, 64);
      w |= __shfl_xor(w, 4, 64);
      if (leader) reinterpret_cast<uint32_t*>(j.mask[m])[word] = w;
    }
  }
}

// The chunk at start4 of job j (fields dst, base, src, mask, n_elem): chunk_stream's loads (4 float4 per thread, strided by the
// block, all issued before the first use), then the slots.  No __restrict__: dst may be the base or a source exactly; every load
// of a float4 precedes its store.
template <int NSRC, int KIND, class Job, class Rule>
__device__ __forceinline__ void mask_chunk(const Job& j, uint64_t start4, Rule& rule) {
  const uint64_t n4 = j.n_elem >> 2, n_words = tall_mask_words(j.n_elem);
  const uint32_t tail = (uint32_t)(j.n_elem & 3);
  const f32x4* base = reinterpret_cast<const f32x4*>(j.base);
  const f32x4* s[NSRC];
#pragma unroll
  for (int m = 0; m < NSRC; ++m) s[m] = reinterpret_cast<const f32x4*>(j.src[m]);
  f32x4 v[4][NSRC];
  f32x4 b[4];
  uint64_t idx[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    idx[u] = start4 + threadIdx.x + u * CHUNK_THREADS;
    if (idx[u] < n4) {
#pragma unroll
      for (int m = 0; m < NSRC; ++m) v[u][m] = __builtin_nontemporal_load(&s[m][idx[u]]);
      b[u] = __builtin_nontemporal_load(&base[idx[u]]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) mask_slot<NSRC, KIND>(j, idx[u], n4, tail, n_words, idx[u] < n4, v[u], b[u], rule);
  if (tall_has_tail_slot(start4, j.n_elem))  // workgroup-uniform
    mask_slot<NSRC, KIND>(j, start4 + CHUNK_FLOATS / 4 + threadIdx.x, n4, tail, n_words, false, v[0], b[0], rule);
}
