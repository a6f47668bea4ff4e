// WUDI-Merging (Cheng et al., ICML 2025: data-free merging guided by the task vectors) on the fp64 MFMA leg.  The rule and the
// order of its operations: include/vlm_hip.h.  Per matrix [m][n] the loss L(X) = sum_i w_i ||(X - tau_i) tau_i^T||_F^2 has the
// gradient 2 (X G - B) with G = sum_i w_i tau_i^T tau_i and B = sum_i w_i tau_i (tau_i^T tau_i): the setup makes G, B and X_0 from
// products of csrc/f64ops.hip (vlm_gemm_f64_batched) and the small kernels here; the ITERATION is wudi_step_kernel, one launch per
// Adam step: the product X G on 64 x 64 tiles (f64_tile.h) with the whole Adam update in its epilogue.  Every kernel runs `count`
// matrices of one shape in lock step, pointers from kernel-argument tables (f64_tab.h).
//
// X is kept TWICE: a step reads X_{t-1} from buffer (t - 1) & 1 and writes X_t into buffer t & 1.  Every workgroup of a tile row
// reads that row's whole panel of X_{t-1} as its A operand while its neighbours are already in their epilogues: updated in place,
// late readers would multiply a mixture of two iterates.
//
// Sums (n_i, ||G_i||_F^2, the loss) are made in the FIXED order of f64_sum.h, without atomics: the same bits every run.  The fp32
// tensors are read and written through f32_io.h.
#include "vlm_common.h"
#include "f64_tab.h"
#include "f64_sum.h"
#include "f32_io.h"
#include "f64_tile.h"

// The working set of one matrix: ONE allocation of VLM_WUDI_HEAD + 2 n n + 5 m n doubles
//   head | G [n][n] | G_i [n][n] (setup scratch) | B | X (buffer 0) | X (buffer 1) | M | V      (the last five [m][n])
// M and V hold nothing before the first step: the setup keeps tau_i in V.
#define WUDI_SQ 0      // head[0 .. 3]: n_i = ||tau_i||_F^2
#define WUDI_GSQ 4     // head[4 .. 7]: ||w_i tau_i^T tau_i||_F^2
#define WUDI_K 8       // head[8]: K = sum_i n_i * head[4 + i]
#define WUDI_LOSS0 9   // head[9]: L(X_0);  head[10]: L(X_{T-1})

struct wudi_off_t {
  size_t G, Gi, B, X0, mn, M, V;
  __host__ __device__ wudi_off_t(int m, int n) {
    const size_t nn = (size_t)n * n;
    mn = (size_t)m * n;
    G = VLM_WUDI_HEAD, Gi = G + nn, B = Gi + nn, X0 = B + mn, M = X0 + 2 * mn, V = M + mn;
  }
  __host__ __device__ size_t X(int buf) const { return X0 + (buf ? mn : 0); }  // (no indexed member: that would live in scratch)
};

static int wudi_sum_parts(int m, int n) { return f64_elem_parts((size_t)n * (m > n ? m : n)); }  // the larger of [m][n] and [n][n]
static int wudi_tiles(int m, int n) { return ((m + F64_TILE - 1) / F64_TILE) * ((n + F64_TILE - 1) / F64_TILE); }
// per matrix: the partials of an elementwise sum, then two slots of per-tile loss shares (step 1; the latest later step)
static int wudi_parts(int m, int n) { return wudi_sum_parts(m, n) + 2 * wudi_tiles(m, n); }

// Source k: tau = W_k - c in fp64 into V; X_0 = 0 + tau (k = 0) or X_0 + tau; the partial of sum tau^2.
__global__ __launch_bounds__(256) void wudi_tau_kernel(const f32_in_tab_t in, const f64_tab_t W, int k, int m, int n,
                                                       double* __restrict__ partials, int stride) {
  const int b = blockIdx.y;
  const wudi_off_t off(m, n);
  const size_t N = (size_t)m * n;
  const float* __restrict__ c = in.c[b];
  const float* __restrict__ s = in.s[b];
  double* __restrict__ X0 = W.p[b] + off.X(0);
  double* __restrict__ V = W.p[b] + off.V;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) {
    const double t = __dsub_rn((double)s[e], (double)c[e]);
    V[e] = t;
    X0[e] = __dadd_rn(k ? X0[e] : 0.0, t);
    acc = __dadd_rn(acc, __dmul_rn(t, t));
  }
  acc = f64_block_sum(acc);
  if (threadIdx.x == 0) partials[(size_t)b * stride + blockIdx.x] = acc;
}

// G_i <- w_i * (tau_i^T tau_i) with w_i = 1 / n_i (0 where n_i is not positive); G = 0 + G_i (k = 0) or G + G_i; the partial of
// sum G_i^2.
__global__ __launch_bounds__(256) void wudi_gacc_kernel(const f64_tab_t W, int k, int m, int n, double* __restrict__ partials,
                                                        int stride) {
  const int b = blockIdx.y;
  const wudi_off_t off(m, n);
  const size_t N = (size_t)n * n;
  double* __restrict__ G = W.p[b] + off.G;
  double* __restrict__ Gi = W.p[b] + off.Gi;
  const double sq = W.p[b][WUDI_SQ + k];
  const double w = sq > 0.0 ? __ddiv_rn(1.0, sq) : 0.0;
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) {
    const double g = __dmul_rn(w, Gi[e]);
    Gi[e] = g;
    G[e] = __dadd_rn(k ? G[e] : 0.0, g);
    acc = __dadd_rn(acc, __dmul_rn(g, g));
  }
  acc = f64_block_sum(acc);
  if (threadIdx.x == 0) partials[(size_t)b * stride + blockIdx.x] = acc;
}

// M = V = 0 (adjacent in the working set): the setup kept tau_i there.
__global__ __launch_bounds__(256) void wudi_clear_kernel(const f64_tab_t W, int m, int n) {
  const wudi_off_t off(m, n);
  double* __restrict__ M = W.p[blockIdx.y] + off.M;
  const size_t N = 2 * (size_t)m * n;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) M[e] = 0.0;
}

// Adam step t of every matrix: tile (blockIdx.y, blockIdx.x) of matrix blockIdx.z accumulates (X_{t-1} G)[i][j] over the n
// reduction columns -- X row-major and G read as G[j][k] (it is symmetric): both operands with the reduction index contiguous --
// and per element, in torch.optim.Adam's order, one rounding per operation:
//   d = xg - B;  g = 2 d;  M = beta1 M + (1 - beta1) g;  V = beta2 V + ((1 - beta2) g) g
//   X_t = X_{t-1} - step * (M / (sqrt(V) / bc2s + eps))          step = lr / (1 - beta1^t), bc2s = sqrt(1 - beta2^t): host doubles
// X_t goes to the OTHER buffer.  The tile's share of <X_{t-1}, X_{t-1} G - 2 B> goes to its own slot of `partials`.
struct wudi_step_t {
  int m, n, t, slot;
  double beta1, beta2, eps, step, bc2s;
};
__global__ __launch_bounds__(256, 4) void wudi_step_kernel(const f64_tab_t W, const wudi_step_t p, double* __restrict__ partials,
                                                           int stride, int sum_parts) {
  __shared__ double sa[F64_LDS_DOUBLES], sb[F64_LDS_DOUBLES];
  const int m = p.m, n = p.n;
  const wudi_off_t off(m, n);
  double* __restrict__ work = W.p[blockIdx.z];
  const double* __restrict__ G = work + off.G;
  const double* __restrict__ Bm = work + off.B;
  const double* __restrict__ X = work + off.X((p.t - 1) & 1);
  double* __restrict__ Xn = work + off.X(p.t & 1);
  double* __restrict__ M = work + off.M;
  double* __restrict__ V = work + off.V;
  const int i0 = blockIdx.y * F64_TILE, j0 = blockIdx.x * F64_TILE;
  f64_acc_t acc;
  f64_tile_mac<true, true>(acc.v, 0, n,
                           [&](int k, int c) { return i0 + c < m ? X[(size_t)(i0 + c) * n + k] : 0.0; },
                           [&](int k, int c) { return j0 + c < n ? G[(size_t)(j0 + c) * n + k] : 0.0; }, sa, sb);
  const double omb1 = __dsub_rn(1.0, p.beta1), omb2 = __dsub_rn(1.0, p.beta2);
  double share = 0.0;
  acc.for_each(i0, j0, m, n, [&](int i, int j, double xg) {
    const size_t e = (size_t)i * n + j;
    const double x = X[e], bv = Bm[e];
    const double g = __dmul_rn(2.0, __dsub_rn(xg, bv));
    const double mo = __dadd_rn(__dmul_rn(p.beta1, M[e]), __dmul_rn(omb1, g));
    const double vo = __dadd_rn(__dmul_rn(p.beta2, V[e]), __dmul_rn(__dmul_rn(omb2, g), g));
    const double denom = __dadd_rn(__ddiv_rn(__dsqrt_rn(vo), p.bc2s), p.eps);
    M[e] = mo;
    V[e] = vo;
    Xn[e] = __dsub_rn(x, __dmul_rn(p.step, __ddiv_rn(mo, denom)));
    share = __dadd_rn(share, __dmul_rn(x, __dsub_rn(xg, __dmul_rn(2.0, bv))));
  });
  share = f64_block_sum(share);
  if (threadIdx.x == 0) {
    const int tiles = gridDim.x * gridDim.y;
    partials[(size_t)blockIdx.z * stride + sum_parts + (size_t)p.slot * tiles + blockIdx.y * gridDim.x + blockIdx.x] = share;
  }
}

// K = ((0 + n_0 q_0) + n_1 q_1) + ... with q_i = ||G_i||_F^2;  loss_first = K + the fold of slot 0;  loss_last = K + the fold of
// slot `last`: one wave per matrix.
__global__ __launch_bounds__(64) void wudi_loss_kernel(const double* __restrict__ partials, int stride, int sum_parts, int tiles, int last,
                                                       int S, const f64_tab_t W) {
  const double* __restrict__ p = partials + (size_t)blockIdx.x * stride + sum_parts;
  const double first = f64_wave_fold(p, tiles);
  const double later = f64_wave_fold(p + (size_t)last * tiles, tiles);
  if (threadIdx.x == 0) {
    double* __restrict__ head = W.p[blockIdx.x];
    double K = 0.0;
    for (int i = 0; i < S; ++i) K = __dadd_rn(K, __dmul_rn(head[WUDI_SQ + i], head[WUDI_GSQ + i]));
    head[WUDI_K] = K;
    head[WUDI_LOSS0] = __dadd_rn(first, K);
    head[WUDI_LOSS0 + 1] = __dadd_rn(later, K);
  }
}

// dst = fl32(c + lam * X_T): product, sum, ONE rounding to fp32.  A thread reads its elements of c before it writes them: dst may
// be c, or a source (no source is read here).
__global__ __launch_bounds__(256) void wudi_apply_kernel(const f32_in_tab_t in, const f32_out_tab_t dst, const f64_tab_t W, int m, int n,
                                                         int buf, double lam) {
  const int b = blockIdx.y;
  const wudi_off_t off(m, n);
  const size_t N = (size_t)m * n;
  const float* c = in.c[b];
  float* out = dst.p[b];
  const double* __restrict__ X = W.p[b] + off.X(buf);
  for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; e < N; e += (size_t)gridDim.x * 1024) {
    const int cnt = N - e < 4 ? (int)(N - e) : 4;
    float cv[4], o[4];
    f32_load4(c, e, cnt, cv);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __double2float_rn(__dadd_rn((double)cv[j], __dmul_rn(lam, j < cnt ? X[e + j] : 0.0)));
    f32_store4(out, e, cnt, o);
  }
}

static int wudi_shape(int m, int n, int count) {
  if (m <= 0 || n <= 0 || f64_count(count)) return VLM_ERR_ARG;
  return m > 65535 * F64_TILE ? VLM_ERR_ARG : VLM_OK;  // (the tile grid's y; element offsets are size_t throughout)
}

extern "C" int vlm_wudi_parts(int m, int n) { return m > 0 && n > 0 ? wudi_parts(m, n) : 0; }

extern "C" size_t vlm_wudi_work_doubles(int m, int n) {
  return m > 0 && n > 0 ? VLM_WUDI_HEAD + 2 * (size_t)n * n + 5 * (size_t)m * n : 0;
}

extern "C" size_t vlm_wudi_state_offset(int m, int n, int iters) {
  return m > 0 && n > 0 && iters >= 0 ? wudi_off_t(m, n).X(iters & 1) : 0;
}

extern "C" int vlm_wudi_prepare(const float* const* c_list, const float* const* src_list, int S, int m, int n, double* const* work_list,
                                double* partials, int count, void* stream) {
  if (wudi_shape(m, n, count) || S < 1 || S > VLM_MERGE_MAX_SRC || !src_list || !partials) return VLM_ERR_ARG;
  f32_in_tab_t in;
  f64_tab_t W;
  int rc = f32_ptrs(c_list, count, in.c);
  for (int k = 0; k < S && !rc; ++k) rc = f32_ptrs(src_list + (size_t)k * count, count, in.s);  // (checked before anything is launched)
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const wudi_off_t off(m, n);
  const int stride = wudi_parts(m, n);
  const int parts_mn = f64_elem_parts((size_t)m * n), parts_nn = f64_elem_parts((size_t)n * n);
  const void* tau[VLM_F64_MAX_BATCH];
  const double* gi_in[VLM_F64_MAX_BATCH];
  double* gi[VLM_F64_MAX_BATCH];
  double* bm[VLM_F64_MAX_BATCH];
  for (int i = 0; i < count; ++i) {
    tau[i] = work_list[i] + off.V;
    gi[i] = work_list[i] + off.Gi;
    gi_in[i] = gi[i];
    bm[i] = work_list[i] + off.B;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int k = 0; k < S; ++k) {
    f32_ptrs(src_list + (size_t)k * count, count, in.s);
    hipLaunchKernelGGL(wudi_tau_kernel, dim3(parts_mn, count), dim3(256), 0, s, in, W, k, m, n, partials, stride);
    VLM_CHECK_LAUNCH();
    rc = f64_fold(partials, stride, parts_mn, W, WUDI_SQ + k, count, s);
    if (rc) return rc;
    // G_i = tau^T tau, scaled by w_i and added to G; then B (+)= tau G_i, G_i read through its transpose (it is symmetric)
    rc = vlm_gemm_f64_batched(1, 0, n, n, m, 1.0, tau, n, 0, reinterpret_cast<const double* const*>(tau), n, 0.0, gi, n, count, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(wudi_gacc_kernel, dim3(parts_nn, count), dim3(256), 0, s, W, k, m, n, partials, stride);
    VLM_CHECK_LAUNCH();
    rc = f64_fold(partials, stride, parts_nn, W, WUDI_GSQ + k, count, s);
    if (rc) return rc;
    rc = vlm_gemm_f64_batched(0, 1, m, n, n, 1.0, tau, n, 0, gi_in, n, k ? 1.0 : 0.0, bm, n, count, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(wudi_clear_kernel, dim3(parts_mn, count), dim3(256), 0, s, W, m, n);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_wudi_step(double* const* work_list, int m, int n, int t, double step, double bc2s, double beta1, double beta2,
                             double eps, double* partials, int count, void* stream) {
  if (wudi_shape(m, n, count) || t < 1 || !partials || !(step > 0.0) || !(bc2s > 0.0) || !(eps > 0.0)) return VLM_ERR_ARG;
  f64_tab_t W;
  int rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  const wudi_step_t p = {m, n, t, t == 1 ? 0 : 1, beta1, beta2, eps, step, bc2s};
  dim3 grid((n + F64_TILE - 1) / F64_TILE, (m + F64_TILE - 1) / F64_TILE, count);
  hipLaunchKernelGGL(wudi_step_kernel, grid, dim3(256), 0, (hipStream_t)stream, W, p, partials, wudi_parts(m, n), wudi_sum_parts(m, n));
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_wudi_finish(double* const* work_list, const float* const* c_list, float* const* dst_list, int S, int m, int n,
                               int iters, double lam, double* partials, int count, void* stream) {
  if (wudi_shape(m, n, count) || S < 1 || S > VLM_MERGE_MAX_SRC || iters < 1 || !dst_list || !partials) return VLM_ERR_ARG;
  f32_in_tab_t in;
  f32_out_tab_t dst;
  f64_tab_t W;
  int rc = f32_ptrs(c_list, count, in.c);
  if (!rc) rc = f32_ptrs(dst_list, count, dst.p);
  if (!rc) rc = f64_tab(work_list, count, W);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(wudi_loss_kernel, dim3(count), dim3(64), 0, s, partials, wudi_parts(m, n), wudi_sum_parts(m, n), wudi_tiles(m, n),
                     iters == 1 ? 0 : 1, S, W);
  VLM_CHECK_LAUNCH();
  hipLaunchKernelGGL(wudi_apply_kernel, dim3(f64_elem_parts((size_t)m * n), count), dim3(256), 0, s, in, dst, W, m, n, iters & 1, lam);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
