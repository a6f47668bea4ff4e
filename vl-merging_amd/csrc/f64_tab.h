// Kernel-argument tables of the float64 kernels (csrc/f64ops.hip, csrc/isoc.hip): `count` (<= VLM_F64_MAX_BATCH) matrices of ONE
// shape per launch, a block index picks the matrix.  A single matrix is a one-entry table.
#pragma once
#include "vlm_common.h"

#define VLM_F64_MAX_BATCH 64
struct f64_tab_t {
  double* p[VLM_F64_MAX_BATCH];
};
static inline int f64_tab(double* const* list, int count, f64_tab_t& t) {
  if (!list || count <= 0 || count > VLM_F64_MAX_BATCH) return VLM_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    if (!list[i]) return VLM_ERR_ARG;
    t.p[i] = list[i];
  }
  return VLM_OK;
}

// Iso-C's working set of one matrix (csrc/isoc.hip) is ONE allocation of VLM_ISO_HEAD + 3 * rows * cols doubles:
//   [0] = ||D||_F^2   [1] = <X, D>   [2 + k] = ||X_{k+1} - X_k||_F^2 of step k   then D, X and Y, each [rows][cols] row-major
#define ISO_FRO2 0
#define ISO_NUCLEAR 1
#define ISO_STEP0 2
