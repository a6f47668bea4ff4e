// Batched float64 SVD by one-sided (Hestenes) Jacobi on contiguous rows.  The rule and the working set: include/vlm_hip.h.  A matrix
// is worked on as [p <= q] rows of length q; a sweep walks the round-robin tournament of csrc/jacobi_schedule.h, every step ONE
// launch over `count` matrices of one shape (blockIdx.y the matrix, pointers from a kernel-argument table, f64_tab.h), one
// workgroup per pair: both rows are loaded once into registers, the three sums are made in a fixed lane-then-wave order, and the
// rotated rows of A and of R go back with plain stores.  The pairs of a step are disjoint, so no two workgroups of a launch touch
// the same row.  The only atomics are one count and one maximum per workgroup into the head: both are independent of the order.
//
// Nothing here synchronises.  A matrix whose previous sweep rotated nothing is finished: its workgroups leave at once, so a caller
// may enqueue a generous number of sweeps and read the heads once.
//
// (The build passes -ffp-contract=off: every product and sum below is one rounded operation.)
#include "vlm_common.h"
#include "f64_tab.h"
#include "jacobi_schedule.h"

#define SVD_SMAX 0      // head[0]: the largest singular value (vlm_svd_finish)
#define SVD_DROPPED 1   // head[1]: the rows vlm_svd_finish zeroed (s_j <= floor * s_max, or s_j = 0)
#define SVD_ROT0 2      // head[2 + k]: rotations of sweep k
#define SVD_OFF0 32     // head[32 + k]: the largest |gamma| / sqrt(alpha beta) sweep k met
#define SVD_MAX_Q 8192  // 32 doubles per lane and row

static_assert(SVD_ROT0 + VLM_SVD_MAX_SWEEPS <= SVD_OFF0 && SVD_OFF0 + VLM_SVD_MAX_SWEEPS <= VLM_SVD_HEAD, "the head holds two slots per sweep");

__device__ __forceinline__ double* svd_A(double* head) { return head + VLM_SVD_HEAD; }
__device__ __forceinline__ double* svd_R(double* head, int p, int q) { return head + VLM_SVD_HEAD + (size_t)p * q; }
__device__ __forceinline__ double* svd_S(double* head, int p, int q) { return svd_R(head, p, q) + (size_t)p * p; }
__device__ __forceinline__ int* svd_rank(double* head, int p, int q) { return reinterpret_cast<int*>(svd_S(head, p, q) + p); }

// The sums of three values over the workgroup in a fixed order (a wave's shuffle tree, then the four waves), in every thread.
__device__ __forceinline__ void svd_block_sum3(double& a, double& b, double& c) {
  __shared__ double wsum[3][4];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a += __shfl_down(a, d);
    b += __shfl_down(b, d);
    c += __shfl_down(c, d);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[0][threadIdx.x >> 6] = a;
    wsum[1][threadIdx.x >> 6] = b;
    wsum[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  a = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
  b = (wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3]);
  c = (wsum[2][0] + wsum[2][1]) + (wsum[2][2] + wsum[2][3]);
}

// One pair of one matrix.  PER: doubles per lane and row, PER * 256 >= q; lane t holds elements t, t + 256, ...
template <int PER>
__global__ __launch_bounds__(256) void jacobi_step_kernel(const f64_tab_t W, int p, int q, int step, int sweep, double thr) {
  double* __restrict__ head = W.p[blockIdx.y];
  if (sweep > 0 && head[SVD_ROT0 + sweep - 1] == 0.0) return;  // the previous sweep rotated nothing: this matrix is done
  int i, j;
  jacobi_pair(p, step, blockIdx.x, &i, &j);
  double* __restrict__ ai = svd_A(head) + (size_t)i * q;
  double* __restrict__ aj = svd_A(head) + (size_t)j * q;
  const int tid = threadIdx.x;
  double x[PER], y[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = u * 256 + tid;
    x[u] = e < q ? ai[e] : 0.0;
    y[u] = e < q ? aj[e] : 0.0;
  }
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    alpha += x[u] * x[u];
    beta += y[u] * y[u];
    gamma += x[u] * y[u];
  }
  svd_block_sum3(alpha, beta, gamma);
  const double ab = sqrt(alpha * beta);
  const bool rotate = fabs(gamma) > thr * ab;
  if (tid == 0) {
    const double ratio = ab > 0.0 ? fabs(gamma) / ab : 0.0;
    if (ratio > 0.0)  // non-negative doubles order as their bit patterns do
      atomicMax(reinterpret_cast<unsigned long long*>(head + SVD_OFF0 + sweep), (unsigned long long)__double_as_longlong(ratio));
    if (rotate) atomicAdd(head + SVD_ROT0 + sweep, 1.0);  // a count: exact in any order
  }
  if (!rotate) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double s = c * t;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = u * 256 + tid;
    if (e < q) {
      ai[e] = c * x[u] - s * y[u];
      aj[e] = s * x[u] + c * y[u];
    }
  }
  double* __restrict__ ri = svd_R(head, p, q) + (size_t)i * p;
  double* __restrict__ rj = svd_R(head, p, q) + (size_t)j * p;
#pragma unroll
  for (int u = 0; u < PER; ++u) {  // (p <= q: the same PER covers a row of R)
    const int e = u * 256 + tid;
    if (e < p) {
      const double rx = ri[e], ry = rj[e];
      ri[e] = c * rx - s * ry;
      rj[e] = s * rx + c * ry;
    }
  }
}

// R = I and a zero head (the ranks and s are written by vlm_svd_finish before anything reads them).
__global__ __launch_bounds__(256) void svd_reset_kernel(const f64_tab_t W, int p, int q) {
  double* __restrict__ head = W.p[blockIdx.y];
  double* __restrict__ R = svd_R(head, p, q);
  const size_t N = (size_t)p * p;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) R[e] = e / p == e % p ? 1.0 : 0.0;
  if (blockIdx.x == 0 && threadIdx.x < VLM_SVD_HEAD) head[threadIdx.x] = 0.0;
}

// s_j = |a_j|: one workgroup per row, a lane adds its elements in index order.
__global__ __launch_bounds__(256) void svd_norm_kernel(const f64_tab_t W, int p, int q) {
  double* __restrict__ head = W.p[blockIdx.y];
  const double* __restrict__ a = svd_A(head) + (size_t)blockIdx.x * q;
  double acc = 0.0, z0 = 0.0, z1 = 0.0;
  for (int e = threadIdx.x; e < q; e += 256) acc += a[e] * a[e];
  svd_block_sum3(acc, z0, z1);
  if (threadIdx.x == 0) svd_S(head, p, q)[blockIdx.x] = sqrt(acc);
}

// rank[j] = the number of rows in front of row j by (s descending, index ascending); order[rank[j]] = j; head[0] = s_max and
// head[1] = the number of rows that svd_unit_kernel zeroes.  One workgroup per matrix, O(p^2).
__global__ __launch_bounds__(256) void svd_rank_kernel(const f64_tab_t W, int p, int q, double floor_rel) {
  double* __restrict__ head = W.p[blockIdx.x];
  const double* __restrict__ s = svd_S(head, p, q);
  int* __restrict__ rank = svd_rank(head, p, q);
  int* __restrict__ order = rank + p;
  __shared__ double smax;
  if (threadIdx.x == 0) smax = 0.0;
  __syncthreads();
  for (int j = threadIdx.x; j < p; j += 256) {
    const double sj = s[j];
    int r = 0;
    for (int i = 0; i < p; ++i) {
      const double si = s[i];
      r += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    rank[j] = r;
    order[r] = j;
    if (r == 0) smax = sj;
  }
  __syncthreads();
  double dropped = 0.0, z0 = 0.0, z1 = 0.0;
  for (int j = threadIdx.x; j < p; j += 256) dropped += (s[j] > floor_rel * smax && s[j] > 0.0) ? 0.0 : 1.0;
  svd_block_sum3(dropped, z0, z1);  // a count: exact
  if (threadIdx.x == 0) {
    head[SVD_SMAX] = smax;
    head[SVD_DROPPED] = dropped;
  }
}

// a_j <- a_j / s_j, or a zero row where s_j <= floor * s_max or s_j = 0.
__global__ __launch_bounds__(256) void svd_unit_kernel(const f64_tab_t W, int p, int q, double floor_rel) {
  double* __restrict__ head = W.p[blockIdx.y];
  double* __restrict__ a = svd_A(head) + (size_t)blockIdx.x * q;
  const double sj = svd_S(head, p, q)[blockIdx.x];
  const bool keep = sj > floor_rel * head[SVD_SMAX] && sj > 0.0;
  for (int e = threadIdx.x; e < q; e += 256) a[e] = keep ? a[e] / sj : 0.0;
}

static int svd_shape(int p, int q, int count) {
  if (p < 1 || q < p || count < 1 || count > VLM_F64_MAX_BATCH) return VLM_ERR_ARG;
  return q > SVD_MAX_Q ? VLM_ERR_UNSUPPORTED : VLM_OK;
}

extern "C" size_t vlm_svd_work_doubles(int p, int q) {
  return p < 1 || q < p ? 0 : (size_t)VLM_SVD_HEAD + (size_t)p * q + (size_t)p * p + 2 * (size_t)p;
}

extern "C" int vlm_svd_steps(int p) { return jacobi_steps(p); }

extern "C" int vlm_svd_reset(double* const* work_list, int p, int q, int count, void* stream) {
  f64_tab_t W;
  int rc = svd_shape(p, q, count);
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const size_t blocks = ((size_t)p * p + 255) / 256;
  hipLaunchKernelGGL(svd_reset_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), count), dim3(256), 0, (hipStream_t)stream, W, p, q);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

template <int PER>
static void jacobi_launch(const f64_tab_t& W, int p, int q, int step, int sweep, double thr, int count, hipStream_t s) {
  hipLaunchKernelGGL((jacobi_step_kernel<PER>), dim3(jacobi_pairs(p), count), dim3(256), 0, s, W, p, q, step, sweep, thr);
}

extern "C" int vlm_svd_sweep(double* const* work_list, int p, int q, int sweep, int count, void* stream) {
  f64_tab_t W;
  int rc = svd_shape(p, q, count);
  if (!rc && (sweep < 0 || sweep >= VLM_SVD_MAX_SWEEPS)) rc = VLM_ERR_ARG;
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const double thr = sqrt((double)q) * 0x1p-53;
  const int per = (q + 255) / 256, steps = jacobi_steps(p);
  for (int step = 0; step < steps; ++step) {
    if (per <= 1) jacobi_launch<1>(W, p, q, step, sweep, thr, count, s);
    else if (per <= 2) jacobi_launch<2>(W, p, q, step, sweep, thr, count, s);
    else if (per <= 4) jacobi_launch<4>(W, p, q, step, sweep, thr, count, s);
    else if (per <= 8) jacobi_launch<8>(W, p, q, step, sweep, thr, count, s);
    else if (per <= 12) jacobi_launch<12>(W, p, q, step, sweep, thr, count, s);
    else if (per <= 16) jacobi_launch<16>(W, p, q, step, sweep, thr, count, s);
    else jacobi_launch<32>(W, p, q, step, sweep, thr, count, s);
    VLM_CHECK_LAUNCH();
  }
  return VLM_OK;
}

extern "C" int vlm_svd_finish(double* const* work_list, int p, int q, double floor_rel, int count, void* stream) {
  f64_tab_t W;
  int rc = svd_shape(p, q, count);
  if (!rc && !(floor_rel >= 0.0 && floor_rel < 1.0)) rc = VLM_ERR_ARG;
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(svd_norm_kernel, dim3(p, count), dim3(256), 0, s, W, p, q);
  VLM_CHECK_LAUNCH();
  hipLaunchKernelGGL(svd_rank_kernel, dim3(count), dim3(256), 0, s, W, p, q, floor_rel);
  VLM_CHECK_LAUNCH();
  hipLaunchKernelGGL(svd_unit_kernel, dim3(p, count), dim3(256), 0, s, W, p, q, floor_rel);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
