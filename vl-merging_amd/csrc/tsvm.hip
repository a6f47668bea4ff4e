// TSV-M (task singular vectors; Gargiulo et al., CVPR 2025) around the batched Jacobi SVD of csrc/jacobi.hip: the task vectors into
// SVD working sets, the gather of every expert's leading triplets into Ucat^T and Vcat^T, and the recombination
// Uo diag(scat) Vo^T on the MFMA-f64 tiles of f64_tile.h with the output in its epilogue.  The rule: include/vlm_hip.h.  Every
// kernel runs `count` matrices of one shape in lock step, blockIdx.y (the product: .z) the matrix, pointers from kernel-argument
// tables (f64_tab.h, f32_io.h).  No atomics and no sums outside the product: the same bits every run.
#include "vlm_common.h"
#include "f64_tab.h"
#include "f32_io.h"
#include "f64_tile.h"

struct tsv_src_tab_t {
  const double* w[VLM_MERGE_MAX_SRC][VLM_F64_MAX_BATCH];
};

// A = W - c in fp64 from the fp32 tensors [m][n], stored as [p <= q] rows: transposed when m > n (a strided store, once per merge).
__global__ __launch_bounds__(256) void tsv_delta_kernel(const f32_in_tab_t in, const f64_tab_t W, int m, int n, int transposed) {
  const int b = blockIdx.y;
  const size_t N = (size_t)m * n;
  const float* __restrict__ c = in.c[b];
  const float* __restrict__ s = in.s[b];
  double* __restrict__ A = W.p[b] + VLM_SVD_HEAD;
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; e < N; e += (size_t)gridDim.x * 1024) {
    const int cnt = N - e < 4 ? (int)(N - e) : 4;
    float cv[4], sv[4];
    f32_load4(c, e, cnt, cv);
    f32_load4(s, e, cnt, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      const size_t f = e + j;
      A[transposed ? f64_transposed(f, m, n) : f] = (double)sv[j] - (double)cv[j];
    }
  }
}

// Row i k + r of the destination's A is expert i's triplet of rank r < k: row order_i[r] of its R (side 0: u^T, length p) or of its
// unit rows (side 1: v^T, length q); a zero row where that singular value is exactly zero.  scat[i k + r] = that singular value.
__global__ __launch_bounds__(256) void tsv_gather_kernel(const tsv_src_tab_t src, const f64_tab_t dst, const f64_tab_t scat, int p, int q, int k,
                                                         int side) {
  const int b = blockIdx.y, row = blockIdx.x, i = row / k, r = row % k;
  const double* __restrict__ head = src.w[i][b];
  const double* __restrict__ A = head + VLM_SVD_HEAD;
  const double* __restrict__ R = A + (size_t)p * q;
  const double* __restrict__ s = R + (size_t)p * p;
  const int* __restrict__ order = reinterpret_cast<const int*>(s + p) + p;
  const int j = order[r];
  const double sj = s[j];
  const int len = side ? q : p;
  const double* __restrict__ from = side ? A + (size_t)j * q : R + (size_t)j * p;
  double* __restrict__ to = dst.p[b] + VLM_SVD_HEAD + (size_t)row * len;
  for (int e = threadIdx.x; e < len; e += 256) to[e] = sj > 0.0 ? from[e] : 0.0;
  if (side && threadIdx.x == 0) scat.p[b][row] = sj;
}

// T [p][q] = PU^T diag(scat) PV with PU [kS][p] and PV [kS][q] (the transposed polar factors), one 64 x 64 tile per workgroup, and
// dst = fl32(c + lam * T) in the tensor's own orientation (element (i, j) of T is element (j, i) of a tall tensor).  A lane reads
// its elements of c before it writes them: dst may be c.  kS = 0: T = 0 and dst = c bit for bit.
__global__ __launch_bounds__(256) void tsv_apply_kernel(const f64_tab_t PU, const f64_tab_t PV, const f64_tab_t scat, const f32_io_tab_t io,
                                                        const f64_tab_t Tt, int p, int q, int kS, int n_orig, int transposed, double lam) {
  __shared__ double sa[F64_LDS_DOUBLES], sb[F64_LDS_DOUBLES];
  const int b = blockIdx.z;
  const double* __restrict__ pu = PU.p[b];
  const double* __restrict__ pv = PV.p[b];
  const double* __restrict__ sc = scat.p[b];
  const int i0 = blockIdx.y * F64_TILE, j0 = blockIdx.x * F64_TILE;
  f64_acc_t acc;
  auto a_at = [&](int k, int c) { return i0 + c < p ? pu[(size_t)k * p + i0 + c] * sc[k] : 0.0; };
  auto b_at = [&](int k, int c) { return j0 + c < q ? pv[(size_t)k * q + j0 + c] : 0.0; };
  f64_tile_mac<false, false>(acc.v, 0, kS, a_at, b_at, sa, sb);
  const float* c = io.c[b];
  float* out = io.dst[b];
  double* __restrict__ T = Tt.p[b];
  acc.for_each(i0, j0, p, q, [&](int i, int j, double v) {
    T[(size_t)i * q + j] = v;
    const size_t o = transposed ? (size_t)j * n_orig + i : (size_t)i * n_orig + j;
    const float cv = c[o];
    out[o] = kS > 0 ? __double2float_rn((double)cv + lam * v) : cv;
  });
}

extern "C" int vlm_tsv_delta(const float* const* c_list, const float* const* src_list, int m, int n, double* const* work_list, int count,
                             void* stream) {
  if (m < 1 || n < 1 || f64_count(count)) return VLM_ERR_ARG;
  if ((m > n ? m : n) > 8192) return VLM_ERR_UNSUPPORTED;
  f32_in_tab_t in;
  f64_tab_t W;
  int rc = f32_ptrs(c_list, count, in.c);
  if (!rc) rc = f32_ptrs(src_list, count, in.s);
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const size_t blocks = ((size_t)m * n + 1023) / 1024;
  hipLaunchKernelGGL(tsv_delta_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks), count), dim3(256), 0, (hipStream_t)stream, in, W, m, n,
                     m > n ? 1 : 0);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_tsv_gather(const double* const* src_work_list, int S, int p, int q, int k, int side, double* const* dst_work_list,
                              double* const* scat_list, int count, void* stream) {
  if (S < 1 || S > VLM_MERGE_MAX_SRC || p < 1 || q < p || k < 1 || (long)k * S > p || (side != 0 && side != 1) || f64_count(count) ||
      !src_work_list)
    return VLM_ERR_ARG;
  tsv_src_tab_t src;
  f64_tab_t dst, scat = {};
  int rc = f64_tab(dst_work_list, count, dst);
  if (!rc && side) rc = f64_tab(scat_list, count, scat);  // (side 0 writes no singular values: scat_list may be NULL)
  if (rc) return rc;
  for (int i = 0; i < S; ++i)
    for (int b = 0; b < count; ++b) {
      if (!src_work_list[(size_t)i * count + b]) return VLM_ERR_ARG;
      src.w[i][b] = src_work_list[(size_t)i * count + b];
    }
  hipLaunchKernelGGL(tsv_gather_kernel, dim3(k * S, count), dim3(256), 0, (hipStream_t)stream, src, dst, scat, p, q, k, side);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_tsv_apply(const double* const* pu_list, const double* const* pv_list, const double* const* scat_list,
                             const float* const* c_list, float* const* dst_list, double* const* t_list, int m, int n, int kS, double lam,
                             int count, void* stream) {
  const int p = m < n ? m : n, q = m < n ? n : m;
  if (m < 1 || n < 1 || kS < 0 || kS > p || f64_count(count)) return VLM_ERR_ARG;
  f64_tab_t PU, PV, scat, T;
  f32_io_tab_t io;
  int rc = f64_tab(const_cast<double* const*>(pu_list), count, PU);
  if (!rc) rc = f64_tab(const_cast<double* const*>(pv_list), count, PV);
  if (!rc) rc = f64_tab(const_cast<double* const*>(scat_list), count, scat);
  if (!rc) rc = f64_tab(t_list, count, T);
  if (!rc) rc = f32_ptrs(c_list, count, io.c);
  if (!rc) rc = f32_ptrs(dst_list, count, io.dst);
  if (rc) return rc;
  dim3 grid((q + F64_TILE - 1) / F64_TILE, (p + F64_TILE - 1) / F64_TILE, count);
  hipLaunchKernelGGL(tsv_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, PU, PV, scat, io, T, p, q, kS, n, m > n ? 1 : 0, lam);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
