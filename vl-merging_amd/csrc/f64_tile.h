// The 64 x 64 output tile of the float64 kernels (csrc/f64ops.hip, csrc/wudi.hip) on v_mfma_f64_16x16x4_f64: the staged
// accumulation over the reduction index and a wave's share of the tile.
//
// MFMA f64 16x16x4 operand layout: A[16][4]: lane l holds A[l & 15][l >> 4]; B[4][16]: lane l holds B[l >> 4][l & 15];
// C/D[16][16]: register r of lane l holds row 4*r + (l >> 4) of column l & 15.
#pragma once
#include "vlm_common.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define F64_TILE 64   // output tile per workgroup (4 waves, each 32 x 32 = 2 x 2 MFMA blocks)
#define F64_KC 16     // reduction rows staged per step

// One 64x64 output tile's accumulation over reduction rows [k0, k1): A-side and B-side panels are staged as
// [F64_KC][64 + 1] doubles.  a(k, i) / b(k, j) are fetched through the functors (any layout / element type).
// A_KC / B_KC: the operand is stored with the REDUCTION index contiguous (a row-major A, a transposed B): consecutive lanes then
// fetch consecutive k of one row / column (16 x 8 B = one 128-B line per 16 lanes) instead of 64 different lines per wave
// instruction -- round 5: RegMean's W G products and every GEMM of the blocked Cholesky / solves read at least one operand that way.
// LDS images of a staged panel (round 5; conflict-free by the ds_read_b64 / ds_write_b64 lane-group rules, where the round-2
// [16][64 + 1] image put the two reduction rows a 32-lane group reads on the same banks: every MFMA operand read took 2 x):
//   operand stored with the OUTPUT index contiguous:    [kk][64 + 16]  (row stride 160 words = 32 mod 64: rows kk, kk + 1 in different halves)
//   operand stored with the REDUCTION index contiguous: [c][16 + 2]    (row stride 36 words: 16 consecutive c land on 16 distinct bank quads)
#define F64_LDS_DOUBLES 1280  // max(16 x 80, 64 x 18)
template <bool KC>
__device__ __forceinline__ int f64_lds_at(int kk, int c) { return KC ? c * (F64_KC + 2) + kk : kk * (F64_TILE + 16) + c; }

template <bool A_KC = false, bool B_KC = false, typename FA, typename FB>
__device__ __forceinline__ void f64_tile_mac(f64x4 (&acc)[2][2], int k0, int k1, FA a_at, FB b_at, double* sa, double* sb) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  // The next step's panel elements are requested into registers BEFORE the current step's MFMAs (round 5: the load -> LDS ->
  // barrier -> MFMA chain of one step used to run back to back: the global-load latency was exposed once per 16 reduction rows)
  constexpr int PER = (F64_KC * F64_TILE) / 256;
  double ra[PER], rb[PER];
  auto fetch = [&](int k) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u;
      const int ka = A_KC ? (e & (F64_KC - 1)) : (e >> 6), ca = A_KC ? (e / F64_KC) : (e & 63);
      const int kb = B_KC ? (e & (F64_KC - 1)) : (e >> 6), cb = B_KC ? (e / F64_KC) : (e & 63);
      ra[u] = k + ka < k1 ? a_at(k + ka, ca) : 0.0;
      rb[u] = k + kb < k1 ? b_at(k + kb, cb) : 0.0;
    }
  };
  if (k0 < k1) fetch(k0);
  for (int k = k0; k < k1; k += F64_KC) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u;
      sa[f64_lds_at<A_KC>(A_KC ? (e & (F64_KC - 1)) : (e >> 6), A_KC ? (e / F64_KC) : (e & 63))] = ra[u];
      sb[f64_lds_at<B_KC>(B_KC ? (e & (F64_KC - 1)) : (e >> 6), B_KC ? (e / F64_KC) : (e & 63))] = rb[u];
    }
    __syncthreads();
    if (k + F64_KC < k1) fetch(k + F64_KC);
#pragma unroll
    for (int k4 = 0; k4 < F64_KC; k4 += 4) {
      const int kk = k4 + (lane >> 4), c = lane & 15;
      const double a0 = sa[f64_lds_at<A_KC>(kk, wi + c)], a1 = sa[f64_lds_at<A_KC>(kk, wi + 16 + c)];
      const double b0 = sb[f64_lds_at<B_KC>(kk, wj + c)], b1 = sb[f64_lds_at<B_KC>(kk, wj + 16 + c)];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

// A wave's share of a 64 x 64 output tile: the 2 x 2 MFMA blocks of its 32 x 32 quarter, zero on construction.
struct f64_acc_t {
  f64x4 v[2][2];
  __device__ __forceinline__ f64_acc_t() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) v[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
  }
  // fn(i, j, value) for every element this lane holds of the tile at (i0, j0) that lies inside the rows x cols matrix
  template <typename F>
  __device__ __forceinline__ void for_each(int i0, int j0, int rows, int cols, F fn) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + wi + 16 * a + 4 * r + (lane >> 4), j = j0 + wj + 16 * b + (lane & 15);
          if (i < rows && j < cols) fn(i, j, v[a][b][r]);
        }
  }
};
