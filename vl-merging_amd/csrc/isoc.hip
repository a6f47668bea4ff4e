// Iso-C (isotropic merging; Marczak et al. 2025) without an SVD: the elementwise kernels around the fp64 polar iteration.  The rule
// and the order of its operations: include/vlm_hip.h.  Per step the products, the factorisation and the solve are csrc/f64ops.hip's
// (vlm_iso_gram: the SYRK body of the Gram cache; vlm_cholesky_f64_batched; vlm_solve_spd_right_f64_batched); what is here forms D
// and its norm, combines X and Y after a step, and writes the merged tensor.  Every kernel runs `count` matrices of one shape in
// lock step, blockIdx.y the matrix, pointers from kernel-argument tables (f64_tab.h, f32_io.h).
//
// Sums (||D||_F^2, the step norms, <X, D>) are made in the FIXED order of f64_sum.h, f64_elem_parts(rows * cols) partials per matrix:
// three runs give the same bits.  The fp32 tensors are read and written through f32_io.h.
#include "vlm_common.h"
#include "f64_tab.h"
#include "f64_sum.h"
#include "f32_io.h"

struct iso_in_tab_t {
  const float* c[VLM_F64_MAX_BATCH];
  const float* s[VLM_MERGE_MAX_SRC][VLM_F64_MAX_BATCH];
};

// D = ((0 + (W_0 - c)) + (W_1 - c)) + ... in fp64 from the fp32 tensors [m][n] (float4 loads; a ragged tail element by element),
// stored in working orientation -- transposed when m < n -- as D and as Y, the first solve's right-hand side.  The transposed store
// is strided (consecutive lanes are m doubles apart): it runs once per merge, the iteration's ~100 launches per step dwarf it.
__global__ __launch_bounds__(256) void iso_delta_kernel(const iso_in_tab_t in, const f64_tab_t W, int S, int m, int n, int transposed,
                                                        double* __restrict__ partials) {
  const int b = blockIdx.y;
  const size_t N = (size_t)m * n;
  const float* __restrict__ c = in.c[b];
  double* __restrict__ D = W.p[b] + VLM_ISO_HEAD;
  double* __restrict__ Y = D + 2 * N;
  double acc = 0.0;
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; e < N; e += (size_t)gridDim.x * 1024) {
    const int cnt = N - e < 4 ? (int)(N - e) : 4;
    float cv[4], sv[VLM_MERGE_MAX_SRC][4];
    f32_load4(c, e, cnt, cv);
#pragma unroll
    for (int k = 0; k < VLM_MERGE_MAX_SRC; ++k)
      if (k < S) f32_load4(in.s[k][b], e, cnt, sv[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < VLM_MERGE_MAX_SRC; ++k)
        if (k < S) d = __dadd_rn(d, __dsub_rn((double)sv[k][j], (double)cv[j]));
      const size_t f = e + j;
      const size_t w = transposed ? f64_transposed(f, m, n) : f;
      D[w] = d;
      Y[w] = d;
      acc = __dadd_rn(acc, __dmul_rn(d, d));
    }
  }
  acc = f64_block_sum(acc);
  if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// X <- p X + q Y (two products, one sum) and Y <- the new X, the next solve's right-hand side; the partial of ||X_new - X||_F^2.
// first: X is D / alpha and Y arrives unscaled (the Gram step folded 1 / alpha^2 into Z): both are divided by alpha = sqrt(||D||_F^2)
// here, zero where alpha is not positive.
__global__ __launch_bounds__(256) void iso_step_kernel(const f64_tab_t W, size_t N, int first, double p, double q,
                                                       double* __restrict__ partials) {
  const int b = blockIdx.y;
  double* __restrict__ head = W.p[b];
  const double* __restrict__ D = head + VLM_ISO_HEAD;
  double* __restrict__ X = head + VLM_ISO_HEAD + N;
  double* __restrict__ Y = X + N;
  const double alpha = first ? __dsqrt_rn(head[ISO_FRO2]) : 1.0;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) {
    double x = first ? D[e] : X[e], y = Y[e];
    if (first) {
      x = alpha > 0.0 ? __ddiv_rn(x, alpha) : 0.0;
      y = alpha > 0.0 ? __ddiv_rn(y, alpha) : 0.0;
    }
    const double xn = __dadd_rn(__dmul_rn(p, x), __dmul_rn(q, y));
    const double d = __dsub_rn(xn, x);
    acc = __dadd_rn(acc, __dmul_rn(d, d));
    X[e] = xn;
    Y[e] = xn;
  }
  acc = f64_block_sum(acc);
  if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// finish, phase 1: the partial of <X, D>
__global__ __launch_bounds__(256) void iso_dot_kernel(const f64_tab_t W, size_t N, double* __restrict__ partials) {
  const int b = blockIdx.y;
  const double* __restrict__ D = W.p[b] + VLM_ISO_HEAD;
  const double* __restrict__ X = D + N;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) acc = __dadd_rn(acc, __dmul_rn(X[e], D[e]));
  acc = f64_block_sum(acc);
  if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// finish, phase 2: dst = fl32(c + s X) with s = (lam * <X, D>) / r, X read back through the transpose when m < n (strided, once per
// merge); c itself where ||D||_F^2 = 0.  A thread reads its elements of c before it writes them: dst may be c, or a source (no
// source is read here).
__global__ __launch_bounds__(256) void iso_apply_kernel(const iso_in_tab_t in, const f32_out_tab_t dst, const f64_tab_t W, int m, int n,
                                                        int transposed, double lam, double r) {
  const int b = blockIdx.y;
  const size_t N = (size_t)m * n;
  const float* c = in.c[b];
  float* out = dst.p[b];
  const double* __restrict__ head = W.p[b];
  const double* __restrict__ X = head + VLM_ISO_HEAD + N;
  const bool zero = !(head[ISO_FRO2] > 0.0);
  const double s = __ddiv_rn(__dmul_rn(lam, head[ISO_NUCLEAR]), r);
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; e < N; e += (size_t)gridDim.x * 1024) {
    const int cnt = N - e < 4 ? (int)(N - e) : 4;
    float cv[4];
    f32_load4(c, e, cnt, cv);
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t f = e + j;
      const double x = j < cnt ? X[transposed ? f64_transposed(f, m, n) : f] : 0.0;
      o[j] = zero ? cv[j] : __double2float_rn(__dadd_rn((double)cv[j], __dmul_rn(s, x)));
    }
    f32_store4(out, e, cnt, o);
  }
}

static int iso_shape(int m, int n, int count) { return m > 0 && n > 0 ? f64_count(count) : VLM_ERR_ARG; }

extern "C" int vlm_iso_parts(int m, int n) { return m > 0 && n > 0 ? f64_elem_parts((size_t)m * n) : 0; }

extern "C" int vlm_iso_delta(const float* const* c_list, const float* const* src_list, int S, int m, int n, double* const* work_list,
                             double* partials, int count, void* stream) {
  if (iso_shape(m, n, count) || S < 1 || S > VLM_MERGE_MAX_SRC || !src_list || !partials) return VLM_ERR_ARG;
  iso_in_tab_t in;
  f64_tab_t W;
  int rc = f32_ptrs(c_list, count, in.c);
  for (int k = 0; k < S && !rc; ++k) rc = f32_ptrs(src_list + (size_t)k * count, count, in.s[k]);
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const int parts = f64_elem_parts((size_t)m * n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(iso_delta_kernel, dim3(parts, count), dim3(256), 0, s, in, W, S, m, n, m < n ? 1 : 0, partials);
  VLM_CHECK_LAUNCH();
  return f64_fold(partials, parts, parts, W, ISO_FRO2, count, s);
}

extern "C" int vlm_iso_step(double* const* work_list, int rows, int cols, int first, double p, double q, int k, double* partials,
                            int count, void* stream) {
  if (iso_shape(rows, cols, count) || k < 0 || k >= VLM_ISO_MAX_STEPS || !partials) return VLM_ERR_ARG;
  f64_tab_t W;
  int rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const size_t N = (size_t)rows * cols;
  const int parts = f64_elem_parts(N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(iso_step_kernel, dim3(parts, count), dim3(256), 0, s, W, N, first, p, q, partials);
  VLM_CHECK_LAUNCH();
  return f64_fold(partials, parts, parts, W, ISO_STEP0 + k, count, s);
}

extern "C" int vlm_iso_finish(double* const* work_list, const float* const* c_list, float* const* dst_list, int m, int n, double lam,
                              double* partials, int count, int phases, void* stream) {
  if (iso_shape(m, n, count) || !dst_list || !partials || phases < 1 || phases > (VLM_ISO_PHASE_NUCLEAR | VLM_ISO_PHASE_APPLY))
    return VLM_ERR_ARG;
  iso_in_tab_t in;
  f32_out_tab_t dst;
  f64_tab_t W;
  int rc = f32_ptrs(c_list, count, in.c);
  if (!rc) rc = f32_ptrs(dst_list, count, dst.p);
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const size_t N = (size_t)m * n;
  const int parts = f64_elem_parts(N);
  hipStream_t s = (hipStream_t)stream;
  if (phases & VLM_ISO_PHASE_NUCLEAR) {
    hipLaunchKernelGGL(iso_dot_kernel, dim3(parts, count), dim3(256), 0, s, W, N, partials);
    VLM_CHECK_LAUNCH();
    rc = f64_fold(partials, parts, parts, W, ISO_NUCLEAR, count, s);
    if (rc) return rc;
  }
  if (phases & VLM_ISO_PHASE_APPLY) {
    hipLaunchKernelGGL(iso_apply_kernel, dim3(parts, count), dim3(256), 0, s, in, dst, W, m, n, m < n ? 1 : 0, lam,
                       (double)(m < n ? m : n));
    VLM_CHECK_LAUNCH();
  }
  return VLM_OK;
}
