// DELLA merge (magnitude-ranked drop and rescale; Deep et al. 2024) over every output tensor of an all_moe -> ufo merge.
// No reference site: the reference repository has no DELLA.  The rule is written down in include/vlm_hip.h and restated in
// numpy by tests/della_restatement.py; the kernel is held to that restatement bit for bit.
//
// The keep probability of an entry depends on the RANK of its magnitude inside its row, so the unit of work is not a 16-KiB chunk
// but a tile of whole rows (della_tiles.h: as many rows as fit in 4096 elements).  One streaming pass, DARE's traffic -- 4 (S + 1) B
// read and 4 B written per element -- with the ranks made in LDS:
//   vlm_della_clear_kernel   a tiny launch: the counters of every job start the run at zero.
//   vlm_della_apply_kernel   one launch over the plan's tile table.  A workgroup owns a CONTIGUOUS run of tiles (chunk_walk.h's
//                            chunk_run over records of chunk_t's shape).  Entering a job it builds the job's table
//                            rank -> keep threshold (step 3) in LDS.  Per tile: every load of the base and all sources is issued
//                            (non-temporal, 16 B when row_len % 4 == 0, scalar otherwise) and the values stay in registers; then,
//                            one source after the other, the tile's composites (row in tile, key, index in tile) are sorted by a
//                            bitonic network in LDS (up to DELLA_PASS_BITS strides per pass, in registers), position - row start
//                            is the rank, its threshold is scattered back to the element's place, and steps 4-5 run on the
//                            registers; steps 6-7, the store, the counters.
// The composite is unique per element, so the network needs no stability: equal keys are ordered by index as the rule says, and a
// tile's rows sort apart without segment logic.  A partial tile sorts the next power of two with sentinels above every composite.
// The draws are DARE's (philox.h), per float4 of the FLAT index: a tile of a job whose row_len is no multiple of 4 may begin inside
// a Philox block, so the scalar path draws the block of each element's own flat index.
// Integer counters only, so nothing depends on the order workgroups run in.  -ffp-contract=off and __f*_rn: one rounding per
// operation, no FMA.  The source-count dispatch, the combine rule (steps 6-7), the run loop, the counter flush and clear are
// chunk_walk.h's, the per-job checks, the layout cursor, the upload and the two-launch run chunk_plan.h's.  The workspace's view and
// layout stay this file's own: its header names tiles (n_tiles, tiles_off) where the counter plan of dare.hip and tall.hip names
// chunks, and the shared forms would need a parameter that exists for this file alone.
#include "vlm_common.h"
#include "philox.h"
#include "chunk_walk.h"
#include "della_tiles.h"

#define DELLA_THREADS CHUNK_THREADS   // chunk_flush_counts reduces CHUNK_THREADS / 64 waves
#define DELLA_BLOCKS_PER_CU 12        // the family's widest grid; two are resident per CU (66 KiB of LDS each), the rest queue and
                                      // even out the tail (docs/experiments.md, "DELLA merge": 8 and 32 were timed too)

static_assert(VLM_DELLA_COUNTERS == VLM_TIES_COUNTERS, "della.hip counts into chunk_walk.h's ties_counts_t");
static_assert(VLM_DELLA_MAX_ROW == DELLA_TILE_FLOATS, "a row is at most one tile");
static_assert(DELLA_TILE_FLOATS == 16 * DELLA_THREADS, "a thread holds 16 elements of a tile");

#define DELLA_PASS_BITS 3  // strides per pass of the sort: 8 slots (16 VGPRs) per thread.  With 4 (16 slots) the kernel spills VGPRs
                           // beside the 80 data registers of a four-source tile at two waves per SIMD.
#define DELLA_LI_BITS 12   // index in tile, row in tile: below DELLA_TILE_FLOATS
#define DELLA_KEY_BITS 31

struct della_view_t {
  const vlm_della_header_t* hdr;
  const vlm_della_job_t* jobs;
  const della_tile_t* tiles;
  u64_t* counters;
};

__device__ __forceinline__ della_view_t della_view(unsigned char* ws) {
  della_view_t v;
  v.hdr = reinterpret_cast<const vlm_della_header_t*>(ws);
  v.jobs = reinterpret_cast<const vlm_della_job_t*>(ws + v.hdr->jobs_off);
  v.tiles = reinterpret_cast<const della_tile_t*>(ws + v.hdr->tiles_off);
  v.counters = reinterpret_cast<u64_t*>(ws + v.hdr->counters_off);
  return v;
}

// what a job's scalars come to, workgroup-uniform
struct della_param_t {
  uint64_t seed;
  uint64_t rows;     // n_elem / row_len
  uint32_t stream;
  bool rescale;
  float lam;
};

// the LDS of a workgroup: 66 KiB and the counters' reduction
struct della_lds_t {
  u64_t sort[DELLA_TILE_FLOATS + DELLA_TILE_FLOATS / 16];  // the composites of one source of the tile, at DELLA_PAD(slot)
  uint32_t thr[DELLA_TILE_FLOATS];   // per element of the tile: kb - 1 of its rank (kept iff u <= kb - 1; kb = 2^32 fits)
  uint32_t kb1[VLM_DELLA_MAX_ROW];   // per rank of the job: kb - 1 (step 3)
  u64_t red[(DELLA_THREADS / 64) * VLM_DELLA_COUNTERS];
};

// step 3 for every rank of the job, once per entry into the job
__device__ __forceinline__ void della_thresholds(const vlm_della_job_t& j, uint32_t* kb1) {
  const uint64_t lo = j.keep_lo, span = j.keep_hi - j.keep_lo, L = j.row_len;
  __syncthreads();  // the table of the job before is no longer read
  for (uint32_t r = threadIdx.x; r < L; r += DELLA_THREADS) {
    const uint64_t kb = L > 1 ? lo + span * r / (L - 1) : lo + (span >> 1);
    kb1[r] = (uint32_t)(kb - 1);
  }
  __syncthreads();
}

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1 (the per-source registers need constant indices)
template <int I, int N, class F>
__device__ __forceinline__ void della_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    della_static_for<I + 1, N>(f);
  }
}

// the place in the tile of a thread's unit u (a float4 or an element), component c
template <int C>
__device__ __forceinline__ uint32_t della_li(int u, int c) {
  return (threadIdx.x + (uint32_t)u * DELLA_THREADS) * C + (uint32_t)c;
}

// Slot i of the sort lives at DELLA_PAD(i): one unused slot after every 16, so that the slots the lanes of a wave take together in
// one pass (a thread's own lie 1, 8 or 64 apart) spread over the LDS banks: bank arithmetic, not timed against the plain layout
// (docs/experiments.md, "DELLA merge").
#define DELLA_PAD(i) ((i) + ((i) >> 4))

// The merge steps of phase k with the strides 2^(s + B - 1) .. 2^s, in ONE pass over LDS: a thread takes the 2^B slots that differ
// in the index bits s .. s + B - 1 (all in one half of a k-block: 2^(s + B) <= k), does the B compare-exchange steps on them in
// registers and puts them back.  Ascending where the index bit k is clear.
template <int B>
__device__ __forceinline__ void della_merge_pass(u64_t* sort, uint32_t N, uint32_t k, uint32_t s) {
  constexpr int G = 1 << B;
  const uint32_t low = (1u << s) - 1;
  for (uint32_t g = threadIdx.x; g < (N >> B); g += DELLA_THREADS) {
    const uint32_t first = ((g & ~low) << B) | (g & low);
    const bool up = (first & k) == 0;
    u64_t x[G];
#pragma unroll
    for (int j = 0; j < G; ++j) x[j] = sort[DELLA_PAD(first + ((uint32_t)j << s))];
#pragma unroll
    for (int b = B - 1; b >= 0; --b) {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if ((j & (1 << b)) == 0) {
          const u64_t lo = x[j], hi = x[j | (1 << b)];
          const bool swap = (lo > hi) == up;
          x[j] = swap ? hi : lo;
          x[j | (1 << b)] = swap ? lo : hi;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) sort[DELLA_PAD(first + ((uint32_t)j << s))] = x[j];
  }
  __syncthreads();
}

// The ranks of one source's task vector in the tile, as thresholds: s.thr[li] = kb1[rank of element li in its row].
// key[u * C + c]: the key of the thread's element della_li<C>(u, c); T elements in the tile, N slots in the sort.
template <int U, int C>
__device__ __forceinline__ void della_rank(const uint32_t (&key)[U * C], uint32_t T, uint32_t N, uint32_t L, della_lds_t& s) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t first = della_li<C>(u, 0);
    if (first < N) {
      const u64_t row = first / L;  // C = 4: L % 4 == 0, a float4 lies in one row
#pragma unroll
      for (int c = 0; c < C; ++c)
        s.sort[DELLA_PAD(first + c)] =
            first + c < T ? (row << (DELLA_KEY_BITS + DELLA_LI_BITS)) | ((u64_t)key[u * C + c] << DELLA_LI_BITS) | (first + c)
                          : ~(u64_t)0;  // a sentinel: above every composite
    }
  }
  __syncthreads();
  // the bitonic network over N = 2^n slots, ascending.  Phase k = 2^a merges with the strides 2^(a-1) .. 1; up to DELLA_PASS_BITS
  // consecutive strides are one pass over LDS (della_merge_pass).  N, a, the strides are workgroup-uniform.
  for (uint32_t a = 1; (1u << a) <= N; ++a) {
    for (uint32_t top = a; top > 0;) {
      const uint32_t bits = top < DELLA_PASS_BITS ? top : DELLA_PASS_BITS;
      top -= bits;
      if (bits == 3) della_merge_pass<3>(s.sort, N, 1u << a, top);
      else if (bits == 2) della_merge_pass<2>(s.sort, N, 1u << a, top);
      else della_merge_pass<1>(s.sort, N, 1u << a, top);
    }
  }
  // position pos holds the element of rank pos - row * L of row `row`: its threshold goes to the element's own place
  for (uint32_t pos = threadIdx.x; pos < T; pos += DELLA_THREADS) {
    const u64_t x = s.sort[DELLA_PAD(pos)];
    const uint32_t at = (uint32_t)x & (DELLA_TILE_FLOATS - 1), r = (uint32_t)(x >> (DELLA_KEY_BITS + DELLA_LI_BITS));
    s.thr[at] = s.kb1[pos - r * L];
  }
  __syncthreads();
}

// One tile: rows [row0, row0 + rows of the tile) of job j.  VEC: row_len % 4 == 0, so the tile begins on a float4 of the tensor,
// a float4 lies in one row and a thread owns float4 t + 256 u of the tile (u < 4); otherwise it owns element t + 256 u (u < 16).
template <int NSRC, bool VEC>
__device__ __forceinline__ void della_tile(const vlm_della_job_t& j, uint32_t row0, const della_param_t& p, della_lds_t& s,
                                           ties_counts_t& n) {
  constexpr int U = VEC ? 4 : 16, C = VEC ? 4 : 1, E = U * C;
  const uint32_t L = j.row_len, per = della_tile_rows(L);
  const uint64_t left = p.rows - row0;
  const uint32_t T = (left < per ? (uint32_t)left : per) * L;          // elements of the tile, <= DELLA_TILE_FLOATS
  const uint32_t N = T <= 1 ? 1u : 1u << (32 - __clz(T - 1));          // slots of the sort
  const uint64_t e0 = (uint64_t)row0 * L;                              // the tile's first element in the tensor
  float b[E], v[NSRC][E];  // the base; per source W_m, then t_m, then tt_m
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (della_li<C>(u, 0) < T) {
      if constexpr (VEC) {
        const uint64_t i4 = (e0 >> 2) + threadIdx.x + u * DELLA_THREADS;
#pragma unroll
        for (int m = 0; m < NSRC; ++m) {
          const f32x4 x = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(j.src[m])[i4]);
#pragma unroll
          for (int c = 0; c < 4; ++c) v[m][u * 4 + c] = x[c];
        }
        const f32x4 x = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(j.base)[i4]);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[u * 4 + c] = x[c];
      } else {
        const uint64_t i = e0 + della_li<C>(u, 0);
#pragma unroll
        for (int m = 0; m < NSRC; ++m) v[m][u] = __builtin_nontemporal_load(&reinterpret_cast<const float*>(j.src[m])[i]);
        b[u] = __builtin_nontemporal_load(&reinterpret_cast<const float*>(j.base)[i]);
      }
    }
  }
  uint32_t any = 0;  // bit k: some source keeps the thread's element k
  della_static_for<0, NSRC>([&](auto M) __attribute__((always_inline)) {
    constexpr int m = M();
    uint32_t key[E];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int k = u * C + c;
        const bool in = della_li<C>(u, 0) < T;
        if (in) v[m][k] = __fsub_rn(v[m][k], b[k]);                       // step 1
        key[k] = in ? __float_as_uint(v[m][k]) & 0x7fffffffu : 0u;        // step 2
      }
    della_rank<U, C>(key, T, N, L, s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (della_li<C>(u, 0) < T) {
        philox4_t dr = {};
        if constexpr (VEC) dr = dare_draw4(p.seed, p.stream, (uint32_t)m, (uint32_t)((e0 >> 2) + threadIdx.x + u * DELLA_THREADS));
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int k = u * C + c;
          uint32_t draw;                                                 // step 4
          if constexpr (VEC) {
            draw = dr.w[c];
          } else {
            const uint64_t i = e0 + della_li<C>(u, 0);
            draw = philox_word(dare_draw4(p.seed, p.stream, (uint32_t)m, (uint32_t)(i >> 2)), (uint32_t)i & 3u);
          }
          const uint32_t kb1 = s.thr[della_li<C>(u, c)];
          const bool kept = draw <= kb1;                                 // step 5: (uint64) u < kb
          const float kbf = kb1 == 0xffffffffu ? 4294967296.0f : __uint2float_rn(kb1 + 1u);
          const float scale = p.rescale ? __fdiv_rn(4294967296.0f, kbf) : 1.0f;
          v[m][k] = kept ? __fmul_rn(v[m][k], scale) : 0.0f;
          n.c[m] += kept ? 1u : 0u;
          any |= kept ? 1u << k : 0u;
        }
      }
    }
  });
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (della_li<C>(u, 0) < T) {
      float o[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int k = u * C + c;
        float tt[NSRC];
#pragma unroll
        for (int m = 0; m < NSRC; ++m) tt[m] = v[m][k];
        const int some = (int)((any >> k) & 1u);
        o[c] = j.mode == VLM_DELLA_TIES                                  // steps 6-7 (chunk_walk.h)
                   ? combine<NSRC, COMBINE_TIES>(b[k], tt, some, p.lam, n.c[TIES_CONFLICT], n.c[TIES_EMPTY])
                   : combine<NSRC, COMBINE_LINEAR>(b[k], tt, some, p.lam, n.c[TIES_CONFLICT], n.c[TIES_EMPTY]);
      }
      if constexpr (VEC) {
        f32x4 x;
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = o[c];
        __builtin_nontemporal_store(x, &reinterpret_cast<f32x4*>(j.dst)[(e0 >> 2) + threadIdx.x + u * DELLA_THREADS]);
      } else {
        __builtin_nontemporal_store(o[0], &reinterpret_cast<float*>(j.dst)[e0 + della_li<C>(u, 0)]);
      }
    }
  }
}

__global__ __launch_bounds__(DELLA_THREADS) void vlm_della_clear_kernel(unsigned char* __restrict__ ws) {
  const della_view_t w = della_view(ws);
  chunk_clear_counts(w.counters, w.hdr->n_jobs * VLM_DELLA_COUNTERS);
}

__global__ __launch_bounds__(DELLA_THREADS, 2) void vlm_della_apply_kernel(unsigned char* __restrict__ ws) {
  __shared__ della_lds_t s;
  const della_view_t w = della_view(ws);
  uint64_t c0, c1;
  if (!chunk_my_run(w.hdr->n_tiles, &c0, &c1)) return;
  ties_counts_t n;
#pragma unroll
  for (int k = 0; k < VLM_DELLA_COUNTERS; ++k) n.c[k] = 0;
  della_param_t p = {0, 0, 0, false, 0.0f};
  chunk_run(
      w.tiles, w.jobs, c0, c1,
      [&](uint32_t cur) {
        const vlm_della_job_t jn = w.jobs[cur];
        p.seed = jn.seed;
        p.rows = jn.n_elem / jn.row_len;
        p.stream = jn.stream;
        p.rescale = jn.rescale != 0;
        p.lam = jn.lam;
        della_thresholds(jn, s.kb1);
      },
      [&](const vlm_della_job_t& j, uint64_t row0) __attribute__((always_inline)) {
        with_nsrc(j.n_src, [&](auto S) __attribute__((always_inline)) {
          if ((j.row_len & 3u) == 0) della_tile<S(), true>(j, (uint32_t)row0, p, s, n);
          else della_tile<S(), false>(j, (uint32_t)row0, p, s, n);
        });
      },
      [&](uint32_t cur) { chunk_flush_counts(n.c, s.red, w.counters + (uint64_t)cur * VLM_DELLA_COUNTERS); });
}

// fills every offset of `h` for n_jobs jobs and n_tiles tiles; returns the total size
static size_t della_layout(vlm_della_header_t* h, uint64_t n_jobs, uint64_t n_tiles) {
  chunk_layout_t at;
  at.take(sizeof(vlm_della_header_t));
  h->n_jobs = n_jobs;
  h->n_tiles = n_tiles;
  h->jobs_off = at.take(n_jobs * sizeof(vlm_della_job_t));
  h->tiles_off = at.take(n_tiles * sizeof(della_tile_t));
  h->counters_off = at.take(n_jobs * VLM_DELLA_COUNTERS * sizeof(uint64_t));
  return at.off;
}

extern "C" size_t vlm_della_plan_bytes(int n_jobs, uint64_t total_elems) {
  if (n_jobs < 0) return 0;
  vlm_della_header_t h;
  return della_layout(&h, (uint64_t)n_jobs, della_tiles_bound(n_jobs, total_elems));
}

extern "C" int vlm_della_plan_upload(const vlm_della_job_t* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!jobs || n_jobs <= 0 || !chunk_ptr_ok(workspace)) return VLM_ERR_ARG;
  uint64_t n_tiles = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const vlm_della_job_t& j = jobs[i];
    if (j.n_elem == 0 || (j.mode != VLM_DELLA_LINEAR && j.mode != VLM_DELLA_TIES) || (j.rescale != 0 && j.rescale != 1))
      return VLM_ERR_ARG;
    if (j.keep_lo < 1 || j.keep_lo > j.keep_hi || j.keep_hi > (1ull << 32)) return VLM_ERR_ARG;
    const int rc = chunk_job_check(j, CHUNK_OVERLAP_NONE, true);
    if (rc != VLM_OK) return rc;
    if (j.row_len < 1 || j.row_len > VLM_DELLA_MAX_ROW) return VLM_ERR_UNSUPPORTED;
    if (j.n_elem % j.row_len != 0) return VLM_ERR_ARG;
    if (!della_rows_ok(j.n_elem, j.row_len)) return VLM_ERR_UNSUPPORTED;
    n_tiles += della_tiles_of(j.n_elem, j.row_len);
  }
  if (!chunk_count_ok(n_tiles)) return VLM_ERR_UNSUPPORTED;
  vlm_della_header_t hdr;
  const size_t total = della_layout(&hdr, (uint64_t)n_jobs, n_tiles);
  if (total > workspace_bytes) return VLM_ERR_WORKSPACE;
  // the host image ends where the counters begin: they are device-made (every run zeroes them first)
  std::vector<unsigned char> img(hdr.counters_off, 0);
  memcpy(img.data(), &hdr, sizeof(hdr));
  memcpy(img.data() + hdr.jobs_off, jobs, (size_t)n_jobs * sizeof(vlm_della_job_t));
  della_tile_fill(reinterpret_cast<della_tile_t*>(img.data() + hdr.tiles_off), jobs, n_jobs);
  return chunk_upload(workspace, img, 0, (hipStream_t)stream);
}

extern "C" int vlm_della_run(void* workspace, void* stream) {
  return counts_run(workspace, stream, vlm_della_clear_kernel, vlm_della_apply_kernel, chunk_grid(DELLA_BLOCKS_PER_CU));
}
