// Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"): a counter-based generator, so a draw is a
// pure function of (counter, key) and costs no memory.  dare.hip and della.hip key it by (seed, stream, source, element):
// include/vlm_hip.h, the DARE block, step 2.  Plain C++ integer arithmetic (a 64-bit product per multiplier gives both halves);
// compiles without HIP as chunk_plan.h does (tests/helpers/philox_check.cpp does so).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PHILOX_HD __host__ __device__ __forceinline__
#else
#define PHILOX_HD static inline
#endif

#define PHILOX_M0 0xD2511F53u  // times counter word 0
#define PHILOX_M1 0xCD9E8D57u  // times counter word 2
#define PHILOX_W0 0x9E3779B9u  // key increments
#define PHILOX_W1 0xBB67AE85u

struct philox4_t {
  uint32_t w[4];
};

PHILOX_HD philox4_t philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0;
    const uint64_t p1 = (uint64_t)PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += PHILOX_W0;  // bumped after each round
    k1 += PHILOX_W1;
  }
  philox4_t o;
  o.w[0] = c0;
  o.w[1] = c1;
  o.w[2] = c2;
  o.w[3] = c3;
  return o;
}

// word c (0 .. 3) of a block, for a c that is not a compile-time constant: selects, not an indexed (scratch) access
PHILOX_HD uint32_t philox_word(const philox4_t& r, uint32_t c) {
  return c == 0 ? r.w[0] : (c == 1 ? r.w[1] : (c == 2 ? r.w[2] : r.w[3]));
}

// The four draws of DARE for the float4 `i4` (= element index >> 2) of source m: word (i & 3) belongs to element i.
PHILOX_HD philox4_t dare_draw4(uint64_t seed, uint32_t stream, uint32_t m, uint32_t i4) {
  return philox4x32_10(i4, 0u, m, stream, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}
