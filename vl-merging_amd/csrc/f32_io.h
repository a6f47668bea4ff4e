// The fp32 side of the per-matrix float64 merge kernels (csrc/isoc.hip, csrc/wudi.hip, csrc/tsvm.hip), stated once: the
// kernel-argument tables of their fp32 tensors (beside f64_tab.h's table of working sets), the checks their entry points make of
// a pointer list and of a count, four-at-a-time loads and stores with a ragged tail, and the index of an element in the transpose.
#pragma once
#include "vlm_common.h"
#include "f64_tab.h"

struct f32_in_tab_t {
  const float* c[VLM_F64_MAX_BATCH];  // the central tensors
  const float* s[VLM_F64_MAX_BATCH];  // ONE source each, or unused
};
struct f32_out_tab_t {
  float* p[VLM_F64_MAX_BATCH];
};
struct f32_io_tab_t {
  const float* c[VLM_F64_MAX_BATCH];
  float* dst[VLM_F64_MAX_BATCH];  // dst[b] may be c[b]
};

static inline int f64_count(int count) { return count >= 1 && count <= VLM_F64_MAX_BATCH ? VLM_OK : VLM_ERR_ARG; }

// `count` fp32 tensors, each non-null and 16-byte aligned (the float4 accesses below), into a table's column.
template <class T>
static inline int f32_ptrs(T* const* list, int count, T** out) {
  if (!list) return VLM_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    if (!list[i] || ((uintptr_t)list[i] & 15)) return VLM_ERR_ARG;
    out[i] = list[i];
  }
  return VLM_OK;
}

// v = t[e .. e + 4): one float4 load, or the `cnt` < 4 elements of a ragged tail one by one with zeros behind them.
__device__ __forceinline__ void f32_load4(const float* t, size_t e, int cnt, float (&v)[4]) {
  if (cnt == 4) {
    const float4 x = *reinterpret_cast<const float4*>(t + e);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? t[e + j] : 0.0f;
  }
}

// t[e .. e + cnt) = v: one float4 store, or a ragged tail one by one.
__device__ __forceinline__ void f32_store4(float* t, size_t e, int cnt, const float (&v)[4]) {
  if (cnt == 4) {
    *reinterpret_cast<float4*>(t + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) t[e + j] = v[j];
  }
}

// Where element f of a row-major [m][n] matrix lies in its row-major transpose [n][m].
__device__ __forceinline__ size_t f64_transposed(size_t f, int m, int n) { return (f % n) * m + f / n; }
