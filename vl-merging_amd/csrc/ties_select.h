// What the radix selects of ties.hip (one rank per source) and band.hip (two ranks per source) share, moved here from ties.hip
// as it stood: the block and grid constants, the (job, source) unit, the key, the bins and shift of a pass, and the flush of a
// workgroup's LDS histograms into a unit's global ones.  Device code only.
#pragma once
#include "vlm_common.h"
#include "chunk_walk.h"

#define TIES_THREADS CHUNK_THREADS  // the chunk walkers need the chunk's 256; the scan kernel uses the same block
#define TIES_BINS 2048u           // bins per source in LDS and in global memory (pass 0 uses all, passes 1 and 2 use 1024)
#define TIES_HIST_BLOCKS_PER_CU 4  // under 128 VGPRs: four workgroups (one wave per SIMD each) are resident per CU; 32 KiB LDS each
#define TIES_APPLY_BLOCKS_PER_CU 12  // three resident per CU (145 VGPRs): four even rounds
#define TIES_SCAN_BLOCKS 1024
// The three grid sizes above follow from the kernels' resident-workgroup counts (register and LDS use recorded by the build); none of
// them has been A/B-measured against other values (docs/experiments.md, "TIES merge").

struct ties_unit_t {  // one (job, source) pair
  uint32_t job;
  uint32_t m;
};

template <int PASS>
__device__ __forceinline__ constexpr uint32_t ties_bins() { return PASS == 0 ? 2048u : 1024u; }
template <int PASS>
__device__ __forceinline__ constexpr int ties_shift() { return PASS == 0 ? 20 : (PASS == 1 ? 10 : 0); }

__device__ __forceinline__ uint32_t ties_key(float w, float c) { return __float_as_uint(__fsub_rn(w, c)) & 0x7fffffffu; }

template <int PASS>
__device__ __forceinline__ void ties_flush(uint32_t* lds, u64_t* hist, int n_src) {
  __syncthreads();  // every LDS atomic of the run has landed
  for (int m = 0; m < n_src; ++m)
    for (uint32_t i = threadIdx.x; i < ties_bins<PASS>(); i += TIES_THREADS) {
      const uint32_t cnt = lds[m * TIES_BINS + i];
      if (cnt) {
        __hip_atomic_fetch_add(&hist[(uint64_t)m * TIES_BINS + i], (u64_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lds[m * TIES_BINS + i] = 0;
      }
    }
  __syncthreads();
}
