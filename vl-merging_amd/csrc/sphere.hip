// Spherical merge (SLERP for two sources, the weighted Karcher mean of the directions for more; mergekit's nuslerp / karcher /
// multislerp family) over every output tensor of an all_moe -> ufo merge.  No reference site: the reference repository has no such
// merge.  The rule, INCLUDING the order of every floating-point operation, is written down in include/vlm_hip.h and restated in
// numpy and python doubles by tests/sphere_restatement.py.  Steps 1, 2 and 4 and every operation of step 3 but acos / sin / cos are
// held to that restatement bit for bit; the three library functions are held to a bound on the coefficients (2^-44 of the
// largest), and the output to step 4 fed the device's own coefficients.
//
// The first method of the family whose coefficients are one scalar PER SOURCE and per group (a tensor or a row), made by a small
// iterative solve on the device from the group's S x S Gram matrix:
//   tensor groups   Model Stock's three launches (stock.hip): vlm_sphere_reduce_kernel is its reducer (gram_reduce.h's rule in
//                   chunk_records.h's run, the same sums byte for byte; a job without a base streams without one),
//                   vlm_sphere_fold_kernel adds a job's records in
//                   chunk order and has one lane do step 3, vlm_sphere_apply_kernel is the chunk table again with S coefficients
//                   loaded on entering a job where Model Stock loads one scale.
//   row groups      ONE launch, vlm_sphere_rows_kernel, over tiles of whole rows (della_tiles.h).  Per tile: every load of the base
//                   and all sources is issued (non-temporal, 16 B when row_len % 4 == 0, scalar otherwise), the values stay in
//                   registers as in della.hip until the task vectors are made and put in LDS (64 KiB); step 2 reads them from there in
//                   the pinned order, one row per wave at a time (row r of a batch of 256 goes to wave r % 4, and lane r / 4 of
//                   that wave keeps its sums); step 3 then runs ONE ROW PER LANE, all the batch's rows at once; the coefficients
//                   go to LDS (and to coef_out) and step 4 takes the task vectors from LDS again and the base from the registers it
//                   has stayed in.  The inputs are read from HBM once.
// The fold also zeroes the results of the row jobs, whose counters the row kernel then raises by integer atomics (the maximum of
// the non-negative doubles `resid` is the integer maximum of their bits), so nothing depends on the order workgroups run in.
// -ffp-contract=off and the __f*_rn / __d*_rn forms: one rounding per operation, no FMA.
#include "vlm_common.h"
#include "chunk_walk.h"
#include "gram_reduce.h"
#include "della_tiles.h"
#include "sphere_plan.h"
#include <math.h>

#define SPHERE_THREADS CHUNK_THREADS
#define SPHERE_REDUCE_BLOCKS_PER_CU 12   // Model Stock's grids (stock.hip): the same kernels' shapes
#define SPHERE_APPLY_BLOCKS_PER_CU 96
#define SPHERE_ROWS_BLOCKS_PER_CU 12     // DELLA's: two workgroups are resident per CU (68 KiB of LDS each), the rest queue
#define SPHERE_BATCH 256                 // rows of a tile whose step 3 runs at once: one per thread
#define SPHERE_EDGE 0x1p-20
#define SPHERE_QMIN 0x1p-40

static_assert(sizeof(vlm_sphere_job_t) == 112 && sizeof(vlm_sphere_header_t) == 72 && sizeof(vlm_sphere_result_t) == 176,
              "the ABI's sizes");
static_assert(offsetof(vlm_sphere_result_t, dot) == VLM_MERGE_MAX_SRC * 8 && offsetof(vlm_sphere_result_t, coef64) == STOCK_SUMS * 8,
              "a result begins as a record does");
static_assert(VLM_DELLA_MAX_ROW == DELLA_TILE_FLOATS && DELLA_TILE_FLOATS == 16 * SPHERE_THREADS, "a thread holds four float4 of a tile");
static_assert(SPHERE_BATCH == SPHERE_THREADS && SPHERE_THREADS == 4 * 64, "a batch deals one row to every lane of four waves");

struct sphere_view_t {
  const vlm_sphere_header_t* hdr;
  const vlm_sphere_job_t* jobs;
  const chunk_t* chunks;
  const della_tile_t* tiles;
  const uint64_t* first;
  double* records;               // [n_chunks][STOCK_SUMS]
  vlm_sphere_result_t* results;  // [n_jobs]
};

__device__ __forceinline__ sphere_view_t sphere_view(unsigned char* ws) {
  sphere_view_t v;
  v.hdr = reinterpret_cast<const vlm_sphere_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_sphere_job_t*>(ws + v.hdr->jobs_off);
  v.chunks = reinterpret_cast<const chunk_t*>(ws + v.hdr->chunks_off);
  v.tiles = reinterpret_cast<const della_tile_t*>(ws + v.hdr->tiles_off);
  v.first = reinterpret_cast<const uint64_t*>(ws + v.hdr->first_off);
  v.records = reinterpret_cast<double*>(ws + v.hdr->records_off);
  v.results = reinterpret_cast<vlm_sphere_result_t*>(ws + v.hdr->results_off);
  return v;
}

// what step 3 gives for one group
struct sphere_coef_t {
  double coef64[VLM_MERGE_MAX_SRC];
  double rho, resid;
  float coef32[VLM_MERGE_MAX_SRC];
  uint32_t status;
};

// nrm2 of step 3: v' C v, i outer, j inner, from +0.0
template <int S>
__device__ __forceinline__ double sphere_nrm2(const double (&v)[S], const double (&C)[S][S]) {
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) t = __dadd_rn(t, __dmul_rn(__dmul_rn(v[i], v[j]), C[i][j]));
  return t;
}

// Step 3 for a group of S sources with the sums g and the weights w[0 .. S): every loop over the sources has a compile-time bound,
// so nothing is indexed at run time and nothing lives in scratch.
template <int S>
__device__ __forceinline__ void sphere_solve(const stock_acc_t<S>& g, const double* w, sphere_coef_t& o) {
#pragma unroll
  for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) {
    o.coef64[m] = 0.0;
    o.coef32[m] = 0.0f;
  }
  o.rho = 0.0;
  o.resid = 0.0;
  double ws = 0.0;
#pragma unroll
  for (int m = 0; m < S; ++m)
    if (g.sq[m] > 0.0) ws = __dadd_rn(ws, w[m]);
  if (!(ws > 0.0)) {
    o.status = VLM_SPHERE_ZERO;
    return;
  }
  double ww[S], n[S], C[S][S], a[S];
#pragma unroll
  for (int m = 0; m < S; ++m) {
    ww[m] = g.sq[m] > 0.0 ? __ddiv_rn(w[m], ws) : 0.0;
    n[m] = __dsqrt_rn(g.sq[m]);
  }
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (i == j) {
        C[i][j] = 1.0;
      } else {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double d = g.dot[hi * (hi - 1) / 2 + lo];
        C[i][j] = (ww[i] > 0.0 && ww[j] > 0.0) ? __ddiv_rn(d, __dmul_rn(n[i], n[j])) : 0.0;
      }
    }
  double rho = 0.0;
#pragma unroll
  for (int m = 0; m < S; ++m) rho = __dadd_rn(rho, __dmul_rn(ww[m], n[m]));
  o.rho = rho;
#pragma unroll
  for (int m = 0; m < S; ++m) a[m] = ww[m];
  const double q0 = sphere_nrm2<S>(a, C);
  if (!(q0 > SPHERE_QMIN)) {
    o.status = VLM_SPHERE_LINEAR;
#pragma unroll
    for (int m = 0; m < S; ++m) {
      o.coef64[m] = ww[m];
      o.coef32[m] = __double2float_rn(ww[m]);
    }
    return;
  }
  {
    const double r = __dsqrt_rn(q0);
#pragma unroll
    for (int m = 0; m < S; ++m) a[m] = __ddiv_rn(a[m], r);
  }
  double vn = 0.0;
#pragma unroll 1
  for (int it = 0; it < VLM_SPHERE_ITERS; ++it) {
    double v[S];
#pragma unroll
    for (int m = 0; m < S; ++m) v[m] = 0.0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      if (ww[i] > 0.0) {
        double ci = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) ci = __dadd_rn(ci, __dmul_rn(a[j], C[j][i]));
        double k;
        if (ci >= 1.0 - SPHERE_EDGE) {
          k = 1.0;
        } else if (ci <= -1.0 + SPHERE_EDGE) {
          k = 0.0;
        } else {
          const double th = acos(ci);
          k = __ddiv_rn(th, sin(th));
        }
        const double wk = __dmul_rn(ww[i], k);
#pragma unroll
        for (int j = 0; j < S; ++j)
          v[j] = __dadd_rn(v[j], __dmul_rn(wk, __dsub_rn(j == i ? 1.0 : 0.0, __dmul_rn(ci, a[j]))));
      }
    }
    const double q = sphere_nrm2<S>(v, C);
    if (!(q > 0.0)) {
      vn = 0.0;  // the step has vanished
      break;
    }
    vn = __dsqrt_rn(q);
    double sn, cv;
    sincos(vn, &sn, &cv);  // the library's sin and cos of one argument, sharing its reduction
    const double sv = __ddiv_rn(sn, vn);
    double b[S];
#pragma unroll
    for (int m = 0; m < S; ++m) b[m] = __dadd_rn(__dmul_rn(cv, a[m]), __dmul_rn(sv, v[m]));
    const double q2 = sphere_nrm2<S>(b, C);
    if (!(q2 > SPHERE_QMIN)) break;
    const double r = __dsqrt_rn(q2);
#pragma unroll
    for (int m = 0; m < S; ++m) a[m] = __ddiv_rn(b[m], r);
  }
  o.status = VLM_SPHERE_OK;
  o.resid = vn;
#pragma unroll
  for (int m = 0; m < S; ++m) {
    const double c = ww[m] > 0.0 ? __ddiv_rn(__dmul_rn(rho, a[m]), n[m]) : 0.0;
    o.coef64[m] = c;
    o.coef32[m] = __double2float_rn(c);
  }
}

// ------------------------------------------------------------------------------------------------------------ tensor groups
__global__ __launch_bounds__(STOCK_THREADS) void vlm_sphere_reduce_kernel(unsigned char* __restrict__ ws) {
  // vlm_stock_reduce_kernel over this plan's tables; a job without a base streams without one
  const sphere_view_t w = sphere_view(ws);
  chunk_reduce_run<STOCK_SUMS>(
      w.chunks, w.jobs, w.hdr->n_chunks, w.first, w.records, [](uint32_t) {},
      [](const vlm_sphere_job_t& j, uint64_t start4, double* r) {
        with_nsrc(j.n_src, [&](auto S) {
          if (j.base) stock_chunk<S(), true>(j, start4, r);
          else stock_chunk<S(), false>(j, start4, r);
        });
      },
      [](const vlm_sphere_job_t& j, int k) { return stock_slot_used(k, j.n_src); });
}

__global__ __launch_bounds__(STOCK_FOLD_THREADS) void vlm_sphere_fold_kernel(unsigned char* __restrict__ ws) {
  __shared__ double sums[STOCK_SUMS];
  const sphere_view_t w = sphere_view(ws);
  const int k = threadIdx.x;
  // a workgroup per job; the grid is fixed (the job count lives in the header, on the device), so it strides over the jobs
  for (uint64_t job = blockIdx.x; job < w.hdr->n_jobs; job += gridDim.x) {
    const vlm_sphere_job_t j = w.jobs[job];
    vlm_sphere_result_t* out = &w.results[job];
    if (j.row_len != 0) {  // a row job: its counters start the run at zero (block-uniform branch)
      if (k < (int)(sizeof(vlm_sphere_result_t) / 8)) reinterpret_cast<uint64_t*>(out)[k] = 0;
      continue;
    }
    if (k < STOCK_SUMS) {
      const double* rec = w.records + k;
      const uint64_t c0 = w.first[job], c1 = w.first[job + 1];
      double sum = 0.0;
      CHUNK_FOLD_RECORDS(sum, rec, STOCK_SUMS, c0, c1);
      sums[k] = sum;
    }
    __syncthreads();
    if (k == 0) {
      sphere_coef_t o;
      with_nsrc(j.n_src, [&](auto S) __attribute__((always_inline)) {
        stock_acc_t<S()> g;
        g.clear();
#pragma unroll
        for (int m = 0; m < S(); ++m) g.sq[m] = sums[m];
#pragma unroll
        for (int p = 0; p < stock_acc_t<S()>::NP; ++p) g.dot[p] = sums[VLM_MERGE_MAX_SRC + p];
        sphere_solve<S()>(g, j.w, o);
      });
#pragma unroll
      for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) {
        out->sq[m] = sums[m];
        out->coef64[m] = o.coef64[m];
        out->coef32[m] = o.coef32[m];
      }
#pragma unroll
      for (int p = 0; p < STOCK_PAIRS; ++p) out->dot[p] = sums[VLM_MERGE_MAX_SRC + p];
      out->rho = o.rho;
      out->resid = o.resid;
      out->status = o.status;
      out->reserved = 0;
      out->rows_linear = 0;
      out->rows_zero = 0;
      out->resid_max = 0.0;
      if (j.coef_out) {
        f32x4 c;
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) c[m] = o.coef32[m];
        *reinterpret_cast<f32x4*>(j.coef_out) = c;
      }
    }
    __syncthreads();  // the next job's sums overwrite these
  }
}

// Steps 1 and 4 as chunk_stream's rule.
template <int S, bool BASE>
struct sphere_apply_rule {
  const float (&cf)[VLM_MERGE_MAX_SRC];  // workgroup-uniform: the job's, loaded on entering it
  const float& lam;
  __device__ __forceinline__ chunk_no_prep prep(uint64_t) const { return {}; }
  __device__ __forceinline__ float elem(const chunk_no_prep&, int, float c, const float* wv) const {
    float d = 0.0f;
#pragma unroll
    for (int m = 0; m < S; ++m) d = __fadd_rn(d, __fmul_rn(cf[m], BASE ? __fsub_rn(wv[m], c) : wv[m]));
    return BASE ? __fadd_rn(c, __fmul_rn(lam, d)) : d;
  }
};

__global__ __launch_bounds__(STOCK_THREADS) void vlm_sphere_apply_kernel(unsigned char* __restrict__ ws) {
  const sphere_view_t w = sphere_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_chunks, &c0, &c1)) return;
  float cf[VLM_MERGE_MAX_SRC] = {0.0f, 0.0f, 0.0f, 0.0f};
  float lam = 0.0f;
  chunk_run(
      w.chunks, w.jobs, c0, c1,
      [&](uint32_t cur) {
#pragma unroll
        for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) cf[m] = w.results[cur].coef32[m];
        lam = w.jobs[cur].lam;
      },
      [&](const vlm_sphere_job_t& j, uint64_t start4) {
        with_nsrc(j.n_src, [&](auto S) {
          if (j.base) {
            sphere_apply_rule<S(), true> rule{cf, lam};
            chunk_stream<S(), true, true>(j, start4, rule);
          } else {
            sphere_apply_rule<S(), false> rule{cf, lam};
            chunk_stream<S(), false, true>(j, start4, rule);
          }
        });
      },
      [&](uint32_t) {});
}

// --------------------------------------------------------------------------------------------------------------- row groups
// the LDS of a workgroup: 68 KiB
struct sphere_lds_t {
  float x[VLM_MERGE_MAX_SRC][DELLA_TILE_FLOATS];   // the tile's task vectors (step 1), per source, at the element's place in the tile
  float coef[SPHERE_BATCH][VLM_MERGE_MAX_SRC];     // coef32 of the batch's rows
};

// what a thread gathers for the job's counters
struct sphere_counts_t {
  uint32_t linear, zero;
  double resid;
};

// One tile: rows [row0, row0 + rows of the tile) of job j, which has `rows` rows; `wts`: the job's weights in the workspace.
// VEC: row_len % 4 == 0, so the tile begins on a float4 of the tensor, a float4 lies in one row and a thread owns float4
// t + 256 u of the tile (u < 4): all its loads are issued before the first use, and the base stays in registers until step 4.
// Otherwise (no shape of a real checkpoint: a row length that is no multiple of 4) a thread walks elements t, t + 256, ... in plain
// loops and reads the base a second time, through L2, in step 4: sixteen unrolled scalar places per thread beside step 3 spill.
// Every index into the tile is below T <= DELLA_TILE_FLOATS, every row index below R <= T.
template <int S, bool VEC>
__device__ __forceinline__ void sphere_tile(const vlm_sphere_job_t& j, const double* wts, uint32_t row0, uint64_t rows,
                                            sphere_lds_t& s, sphere_counts_t& n) {
  constexpr int U = 4;
  const uint32_t L = j.row_len, per = della_tile_rows(L);
  const uint64_t left = rows - row0;
  const uint32_t R = left < per ? (uint32_t)left : per;                // rows of the tile
  const uint32_t T = R * L;                                            // elements of the tile, <= DELLA_TILE_FLOATS
  const uint64_t e0 = (uint64_t)row0 * L;                              // the tile's first element in the tensor
  const bool has_base = j.base != nullptr;
  // the tile's own pointers (workgroup-uniform), so that a thread's indices are 32-bit places in the tile
  const float* base = has_base ? reinterpret_cast<const float*>(j.base) + e0 : nullptr;
  float* dst = reinterpret_cast<float*>(j.dst) + e0;
  const float* src[S];
#pragma unroll
  for (int m = 0; m < S; ++m) src[m] = reinterpret_cast<const float*>(j.src[m]) + e0;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  f32x4 b[VEC ? U : 1];  // VEC: the base, from the loads to step 4
  if constexpr (VEC) {
    f32x4 v[S][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i4 = tid + (uint32_t)u * SPHERE_THREADS;
      if (4 * i4 < T) {
#pragma unroll
        for (int m = 0; m < S; ++m) v[m][u] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(src[m])[i4]);
        b[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (has_base) b[u] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(base)[i4]);
      }
    }
    __syncthreads();  // the loads are in flight; step 4 of the tile before no longer reads the task vectors in LDS
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i4 = tid + (uint32_t)u * SPHERE_THREADS;
      if (4 * i4 < T) {
#pragma unroll
        for (int m = 0; m < S; ++m) {
          f32x4 x = v[m][u];
          if (has_base) {
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = __fsub_rn(x[c], b[u][c]);  // step 1
          }
          *reinterpret_cast<f32x4*>(&s.x[m][4 * i4]) = x;
        }
      }
    }
  } else {
    __syncthreads();  // step 4 of the tile before (which reads other threads' places) no longer reads the task vectors in LDS
#pragma unroll 1
    for (uint32_t li = tid; li < T; li += SPHERE_THREADS) {
      const float c = has_base ? __builtin_nontemporal_load(&base[li]) : 0.0f;
#pragma unroll
      for (int m = 0; m < S; ++m) {
        const float x = __builtin_nontemporal_load(&src[m][li]);
        s.x[m][li] = has_base ? __fsub_rn(x, c) : x;                   // step 1
      }
    }
  }
  __syncthreads();  // the tile's task vectors are in LDS; the coefficients of the tile before are no longer read
  for (uint32_t batch0 = 0; batch0 < R; batch0 += SPHERE_BATCH) {
    if (batch0) __syncthreads();  // the coefficients of the batch before are no longer read
    // step 2: row batch0 + wave + 4 i is reduced by this wave as its i-th; lane i keeps the sums
    stock_acc_t<S> mine;
    mine.clear();
    for (uint32_t i = 0; i < 64 && batch0 + wave + 4 * i < R; ++i) {   // wave-uniform bounds
      const float* xr = &s.x[0][(batch0 + wave + 4 * i) * L];
      stock_acc_t<S> acc;
      acc.clear();
      stock_reduce_rule<S> rule{acc};
      for (uint32_t e = lane; e < L; e += 64) {                         // lane l: elements l, l + 64, ... in rising order
        float wv[S];
#pragma unroll
        for (int m = 0; m < S; ++m) wv[m] = xr[m * DELLA_TILE_FLOATS + e];
        rule.elem(chunk_no_prep{}, 0, 0.0f, wv);                        // x - (+0.0) is x
      }
#pragma unroll
      for (int m = 0; m < S; ++m) {
        const double t = chunk_wave_sum(acc.sq[m]);
        if ((uint32_t)lane == i) mine.sq[m] = t;
      }
#pragma unroll
      for (int p = 0; p < stock_acc_t<S>::NP; ++p) {
        const double t = chunk_wave_sum(acc.dot[p]);
        if ((uint32_t)lane == i) mine.dot[p] = t;
      }
    }
    // step 3: one row per lane
    const uint32_t rb = wave + 4 * lane, r = batch0 + rb;              // rb < SPHERE_BATCH
    if (r < R) {
      sphere_coef_t o;
      sphere_solve<S>(mine, wts, o);  // the weights are read where they are used, not carried through the tile
      f32x4 c;
#pragma unroll
      for (int m = 0; m < VLM_MERGE_MAX_SRC; ++m) c[m] = o.coef32[m];
      *reinterpret_cast<f32x4*>(&s.coef[rb][0]) = c;
      if (j.coef_out) reinterpret_cast<f32x4*>(j.coef_out)[(uint64_t)row0 + r] = c;
      n.linear += o.status == VLM_SPHERE_LINEAR ? 1u : 0u;
      n.zero += o.status == VLM_SPHERE_ZERO ? 1u : 0u;
      n.resid = o.resid > n.resid ? o.resid : n.resid;
    }
    __syncthreads();
    // step 4 for the elements of the batch's rows: the task vectors come back from LDS (held in registers across step 3 they spill)
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t i4 = tid + (uint32_t)u * SPHERE_THREADS;
        const uint32_t at = (4 * i4 < T ? 4 * i4 / L : 0xffffffffu) - batch0;  // L % 4 == 0: a float4 lies in one row
        if (4 * i4 < T && at < SPHERE_BATCH) {
          const f32x4 cf = *reinterpret_cast<const f32x4*>(&s.coef[at][0]);
          f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int m = 0; m < S; ++m) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(&s.x[m][4 * i4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) d[c] = __fadd_rn(d[c], __fmul_rn(cf[m], x[c]));
          }
          if (has_base) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d[c] = __fadd_rn(b[u][c], __fmul_rn(j.lam, d[c]));
          }
          __builtin_nontemporal_store(d, &reinterpret_cast<f32x4*>(dst)[i4]);
        }
      }
    } else {
      const uint32_t lo = batch0 * L, left_rows = R - batch0;
      const uint32_t hi = lo + (left_rows < SPHERE_BATCH ? left_rows : SPHERE_BATCH) * L;  // the batch's elements: [lo, hi)
#pragma unroll 1
      for (uint32_t li = lo + tid; li < hi; li += SPHERE_THREADS) {
        const f32x4 cf = *reinterpret_cast<const f32x4*>(&s.coef[li / L - batch0][0]);
        float d = 0.0f;
#pragma unroll
        for (int m = 0; m < S; ++m) d = __fadd_rn(d, __fmul_rn(cf[m], s.x[m][li]));
        if (has_base) d = __fadd_rn(__builtin_nontemporal_load(&base[li]), __fmul_rn(j.lam, d));
        __builtin_nontemporal_store(d, &dst[li]);
      }
    }
  }
}

// a workgroup's counts for a job, into the job's result: wave sums and maxima by shuffles, then one atomic per wave and counter
__device__ __forceinline__ void sphere_flush_counts(sphere_counts_t& n, vlm_sphere_result_t* out) {
  uint32_t lin = n.linear, zero = n.zero;
  u64_t rb = (u64_t)__double_as_longlong(n.resid);  // non-negative doubles order as their bits do
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lin += __shfl_xor(lin, off, 64);
    zero += __shfl_xor(zero, off, 64);
    const u64_t o = __shfl_xor(rb, off, 64);
    rb = o > rb ? o : rb;
  }
  if ((threadIdx.x & 63) == 0) {
    if (lin) __hip_atomic_fetch_add(reinterpret_cast<u64_t*>(&out->rows_linear), (u64_t)lin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (zero) __hip_atomic_fetch_add(reinterpret_cast<u64_t*>(&out->rows_zero), (u64_t)zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rb) __hip_atomic_fetch_max(reinterpret_cast<u64_t*>(&out->resid_max), rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  n.linear = n.zero = 0;
  n.resid = 0.0;
}

__global__ __launch_bounds__(SPHERE_THREADS, 2) void vlm_sphere_rows_kernel(unsigned char* __restrict__ ws) {
  __shared__ sphere_lds_t s;
  const sphere_view_t w = sphere_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_tiles, &c0, &c1)) return;
  sphere_counts_t n = {0u, 0u, 0.0};
  uint64_t rows = 0;
  const double* wts = nullptr;  // the job's weights, in the workspace
  chunk_run(
      w.tiles, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_sphere_job_t jn = w.jobs[cur];
        rows = jn.n_elem / jn.row_len;
        wts = w.jobs[cur].w;
      },
      [&](const vlm_sphere_job_t& j, uint64_t row0) __attribute__((always_inline)) {
        with_nsrc(j.n_src, [&](auto S) __attribute__((always_inline)) {
          if ((j.row_len & 3u) == 0) sphere_tile<S(), true>(j, wts, (uint32_t)row0, rows, s, n);
          else sphere_tile<S(), false>(j, wts, (uint32_t)row0, rows, s, n);
        });
      },
      [&](uint32_t cur) { sphere_flush_counts(n, &w.results[cur]); });
}

// --------------------------------------------------------------------------------------------------------------------- host
// fills every offset of `h`; returns the total size
static size_t sphere_layout(vlm_sphere_header_t* h, uint64_t n_jobs, uint64_t n_chunks, uint64_t n_tiles) {
  chunk_layout_t at = chunk_layout_head<vlm_sphere_header_t, vlm_sphere_job_t>(h, n_jobs, n_chunks);
  h->n_tiles = n_tiles;
  h->tiles_off = at.take(n_tiles * sizeof(della_tile_t));
  records_parts(at, h, STOCK_SUMS * sizeof(double), sizeof(vlm_sphere_result_t));  // the record plan's, behind the tiles
  return at.off;
}

extern "C" size_t vlm_sphere_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  vlm_sphere_header_t h;  // every job may be of either kind
  return sphere_layout(&h, (uint64_t)n_jobs, chunks_bound(n_jobs, total_elems), della_tiles_bound(n_jobs, total_elems));
}

extern "C" int vlm_sphere_plan_upload(const vlm_sphere_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  for (int i = 0; i < n_jobs; ++i) {
    const int rc = sphere_job_check(jobs[i]);  // sphere_plan.h: the checks, the counts and the tables need no HIP
    if (rc != VLM_OK) return rc;
  }
  std::vector<uint64_t> first((size_t)n_jobs + 1);
  uint64_t n_chunks = 0, n_tiles = 0;
  sphere_count(jobs, n_jobs, first.data(), &n_chunks, &n_tiles);
  if (!chunk_count_ok(n_chunks) || !chunk_count_ok(n_tiles)) return VLM_ERR_UNSUPPORTED;
  vlm_sphere_header_t hdr;
  const size_t total = sphere_layout(&hdr, (uint64_t)n_jobs, n_chunks, n_tiles);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the records begin: they and the results are device-made (every run overwrites all of them)
  std::vector<unsigned char> img(hdr.records_off, 0);
  memcpy(img.data(), &hdr, sizeof(hdr));
  memcpy(img.data() + hdr.jobs_off, jobs, (size_t)n_jobs * sizeof(vlm_sphere_job_t));
  sphere_tables_fill(reinterpret_cast<chunk_t*>(img.data() + hdr.chunks_off), reinterpret_cast<della_tile_t*>(img.data() + hdr.tiles_off),
                     jobs, n_jobs);
  memcpy(img.data() + hdr.first_off, first.data(), first.size() * sizeof(uint64_t));
  return chunk_upload(workspace, img, 0, (hipStream_t)stream);
}

extern "C" int vlm_sphere_run(void* workspace, void* stream) {
  if (!workspace) return VLM_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // four launches, stream-ordered, no host synchronisation: the sizes of the plan live in the workspace header (a kernel whose
  // table is empty returns at once), the coefficients the apply pass reads in the results the fold has written; the fold zeroes
  // the row jobs' results before the row kernel counts into them
  hipLaunchKernelGGL(vlm_sphere_reduce_kernel, chunk_grid(SPHERE_REDUCE_BLOCKS_PER_CU), dim3(STOCK_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_sphere_fold_kernel, chunk_grid(1), dim3(STOCK_FOLD_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_sphere_apply_kernel, chunk_grid(SPHERE_APPLY_BLOCKS_PER_CU), dim3(STOCK_THREADS), 0, s, ws);
  hipLaunchKernelGGL(vlm_sphere_rows_kernel, chunk_grid(SPHERE_ROWS_BLOCKS_PER_CU), dim3(SPHERE_THREADS), 0, s, ws);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
