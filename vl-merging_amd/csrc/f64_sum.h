// The fixed-order float64 sum of the per-matrix merge kernels (csrc/isoc.hip, csrc/wudi.hip), stated once: a thread adds its elements
// in index order, a workgroup's 256 sums meet in a shuffle tree (f64_block_sum) and leave one partial, the partials of a matrix
// (f64_elem_parts of them for an elementwise pass, a function of the element count alone) are added by one wave in the same way
// (f64_wave_fold, f64_fold_kernel).  No atomics: the same bits every run.
#pragma once
#include "vlm_common.h"
#include "f64_tab.h"

#define F64_SUM_MAX_PARTS 256
#define F64_SUM_PER_BLOCK 2048  // elements per partial: a pass over N elements runs min(F64_SUM_MAX_PARTS, ceil(N / 2048)) workgroups,
                                // each striding over the matrix and leaving one partial sum

static int f64_elem_parts(size_t N) {
  const size_t p = (N + F64_SUM_PER_BLOCK - 1) / F64_SUM_PER_BLOCK;
  return p > F64_SUM_MAX_PARTS ? F64_SUM_MAX_PARTS : (int)(p ? p : 1);
}

// The workgroup's (256 threads) sum of `v` in a fixed order, valid in thread 0.
__device__ __forceinline__ double f64_block_sum(double v) {
  __shared__ double wsum[4];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = __dadd_rn(v, __shfl_down(v, d));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return __dadd_rn(__dadd_rn(wsum[0], wsum[1]), __dadd_rn(wsum[2], wsum[3]));
}

// One wave's sum of p[0 .. parts) in a fixed order, valid in lane 0.
__device__ __forceinline__ double f64_wave_fold(const double* __restrict__ p, int parts) {
  double v = 0.0;
  for (int i = threadIdx.x; i < parts; i += 64) v = __dadd_rn(v, p[i]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = __dadd_rn(v, __shfl_down(v, d));
  return v;
}

// W[b][slot] = the sum of matrix b's `parts` partials, `stride` doubles apart from the next matrix's: one wave per matrix.  (static:
// every translation unit that includes this has its own.)
static __global__ __launch_bounds__(64) void f64_fold_kernel(const double* __restrict__ partials, int stride, int parts, const f64_tab_t W,
                                                             int slot) {
  const double v = f64_wave_fold(partials + (size_t)blockIdx.x * stride, parts);
  if (threadIdx.x == 0) W.p[blockIdx.x][slot] = v;
}

static int f64_fold(const double* partials, int stride, int parts, const f64_tab_t& W, int slot, int count, hipStream_t s) {
  hipLaunchKernelGGL(f64_fold_kernel, dim3(count), dim3(64), 0, s, partials, stride, parts, W, slot);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
