/* vlm_hip.h -- C ABI of libvlm_hip.so: the MI355X (gfx950) hot path of ylsung/vl-merging.
 *
 * The reference (/root/reference) is 100 % Python and has no native boundary of its own; every entry
 * point below replaces a stock-PyTorch op site of the reference's hot path and cites it (file:line under
 * /root/reference/src).  Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless named *_host;
 *   - every call is stream-ordered on `stream` (a hipStream_t passed as void*), re-entrant, allocates
 *     nothing: the caller owns outputs and workspaces;
 *   - return 0 on success, a negative VLM_ERR_* otherwise; nothing throws across the boundary;
 *   - process-wide state is limited to (1) the diagnostic switch VLM_GEMM_CUS, read ONCE from the environment at first use
 *     (a thread-safe function-local static, immutable afterwards; the merge kernel's grid and cache policy are fixed:
 *     docs/experiments.md, "Merge kernel: grid and cache policy") and (2) the hooks vlm_gemm_set_big_tile_mode and vlm_set_cu_budget (one atomic int each).  None changes results
 *     beyond the fp32 summation order of a GEMM or of the bias-table gradient.
 *
 * Token layout ("segment-major"): a pass over B samples with n0 text and n1 image tokens per sample keeps
 * activations as a [rows, D] matrix whose rows are  base0 + b*n0 + t  (t < n0)  and  base1 + b*n1 + (t-n0).
 * Modality-specific experts (all_moe) then see contiguous row ranges (vision_transformer.py:607-681 slices
 * and torch.cat's per layer instead).
 */
#ifndef VLM_HIP_H
#define VLM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLM_OK 0
#define VLM_ERR_ARG (-1)
#define VLM_ERR_LAUNCH (-2)
#define VLM_ERR_WORKSPACE (-3)
#define VLM_ERR_UNSUPPORTED (-4)

#define VLM_ABI_VERSION 11
int vlm_abi_version(void);
/* Number of compute units grid sizing and split-K slice counts plan for, or negative error: the current device's count,
 * or the smaller budget set by VLM_GEMM_CUS=n (environment, read once) / vlm_set_cu_budget(n) -- room for RCCL's kernels
 * in a data-parallel job (0 or negative: back to the device's count).  Results do not depend on it beyond fp32 summation
 * order (the number of K slices of a wgrad). */
int vlm_device_cus(void);
int vlm_set_cu_budget(int cus);
/* Measurement tool (no reference counterpart; run.py:263-288's DDP gets its contention from NCCL): `workgroups` workgroups of
 * `threads` threads that each allocate `lds_bytes` of LDS and spin for `microseconds` on `stream` -- the single-GPU stand-in for
 * the compute units a gradient collective's kernels hold during backward (ddp.FlatGradReducer(standin=...)). */
int vlm_debug_occupy(int workgroups, int threads, int lds_bytes, int microseconds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Checkpoint merge (K12/K13/K14-bias): modules/vilt_module.py:533-638 (merge_weights),
 * :640-746 (sum_task_vectors), :436-457/:486-529 (regmean's plain averages).
 * One job = one output tensor.  Arithmetic is fp32, unfused (no FMA), in source order:
 *   VLM_MERGE_LERP    : acc = 0;        acc = acc + ratio[m] * src[m]          (:590-601)
 *   VLM_MERGE_TASKVEC : acc = base;     acc = acc + ratio[m] * (src[m] - acc)  (:700-706, in-place alias
 *                       of the central tensor => recurrence, SURVEY.md 8a checklist item 8)
 *   VLM_MERGE_MEAN    : acc = 0;        acc = acc + src[m];  acc / n_src       (:436-457)
 * dst may alias base.  Bit-exact with the reference's CPU path.
 */
#define VLM_MERGE_LERP 0
#define VLM_MERGE_TASKVEC 1
#define VLM_MERGE_MEAN 2
#define VLM_MERGE_MAX_SRC 4

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem], TASKVEC only (central weight) */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  float ratio[VLM_MERGE_MAX_SRC];
  int32_t n_src;
  int32_t mode;
  uint64_t n_elem;
} vlm_merge_job_t;

/* Bytes of device workspace a plan for n_jobs jobs over total_elems elements needs. */
size_t vlm_merge_plan_bytes(int n_jobs, uint64_t total_elems);
/* Build the chunk table on the host and copy jobs + table into `workspace`.  The source is a temporary pageable host
 * buffer, so the call SYNCHRONISES `stream` before it returns (once per merge plan; vlm_merge_run is asynchronous). */
int vlm_merge_plan_upload(const vlm_merge_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Run an uploaded plan: ONE kernel launch over all jobs. */
int vlm_merge_run(const void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TIES merge (trim, elect sign, disjoint mean; Yadav et al. 2023), csrc/ties.hip.  NO REFERENCE SITE: the reference has
 * no TIES; the arithmetic below is the specification and is pinned to a numpy restatement of it (tests/ties_restatement.py),
 * not to the reference.  One job = one output tensor with central tensor c (base), sources W_0 .. W_{S-1}, scale lam;
 * fp32, one rounding per operation, no FMA, source order:
 *   1. t_m = W_m - c
 *   2. key(x) = bits(x) & 0x7fffffff;  thr_m = the k[m]-th largest key(t_m[i]) of the tensor;
 *      tt_m[i] = t_m[i] if key(t_m[i]) >= thr_m (all ties at the threshold are kept), else +0.0
 *   3. s = ((0 + tt_0) + tt_1) + ...;  the sign is taken by comparison (s > 0, s < 0): -0.0 counts as zero
 *   4. source m agrees at i iff (s > 0 and tt_m > 0) or (s < 0 and tt_m < 0);  num = sum of the agreeing tt_m from +0.0 in
 *      source order, cnt = how many agree;  d = num / float(cnt) if cnt > 0 else +0.0
 *   5. dst = c + lam * d
 * Non-finite inputs are outside the contract.  dst must not overlap base or a source of its own job (the selection passes re-read
 * them; vlm_ties_plan_upload rejects a job whose dst byte range meets one of its inputs' -- overlap ACROSS jobs is the caller's to avoid).
 * k[m] is computed by the caller (1 <= k[m] <= n_elem).
 */
typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t k[VLM_MERGE_MAX_SRC];        /* entries to keep per source (step 2) */
  uint64_t n_elem;
  int32_t n_src;
  float lam;
} vlm_ties_job_t;

/* What a plan's workspace holds, for callers that read results back: the workspace BEGINS with this header (byte offsets from
 * its start).  Jobs keep their upload order; the (job, source) pairs ("units") are numbered job-major, source-minor. */
typedef struct {
  uint64_t n_jobs, n_units, n_chunks;
  uint64_t jobs_off;      /* vlm_ties_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t unit0_off;     /* uint32 [n_jobs]: first unit of each job */
  uint64_t units_off;     /* {uint32 job, uint32 source} [n_units] */
  uint64_t state_off;     /* vlm_ties_state_t [n_units] */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_TIES_COUNTERS] */
  uint64_t hist_off;      /* uint64 [n_units][2048]: selection histograms, zero between runs */
} vlm_ties_header_t;
typedef struct {
  uint32_t key;       /* after a run: thr_m as a key (= the bits of the threshold magnitude) */
  uint32_t reserved;
  uint64_t rank;      /* after a run: 1 + how many of the keys equal to thr_m rank above the k-th place */
} vlm_ties_state_t;
/* per job after a run: kept[0 .. MAX_SRC) = entries kept per source (step 2), then `conflict` = elements where the kept sources
 * hold both a positive and a negative entry, then `empty` = elements with cnt == 0 (step 4) */
#define VLM_TIES_COUNTERS (VLM_MERGE_MAX_SRC + 2)

/* Bytes of device workspace a TIES plan for n_jobs jobs over total_elems elements needs (jobs, chunk table, selection state,
 * histograms, counters).  No reference site. */
size_t vlm_ties_plan_bytes(int n_jobs, uint64_t total_elems);
/* Build the chunk table on the host, copy header + jobs + tables into `workspace` (16-byte aligned) and zero the histograms.
 * Like vlm_merge_plan_upload the call SYNCHRONISES `stream` before it returns (pageable temporary source); it is the last
 * host synchronisation of a plan.  Implements no step of the rule; no reference site. */
int vlm_ties_plan_upload(const vlm_ties_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: steps 1-2 (three histogram launches over all jobs, 11 + 10 + 10 key bits, each followed by a tiny launch
 * that picks the bin of the k-th largest key on the device) and steps 1-5 plus the counters (one launch); seven launches, no
 * host synchronisation.  May be called again on the same workspace and gives the same bytes: the run zeroes its own
 * histograms and counters on the stream.  One run at a time per workspace.  No reference site. */
int vlm_ties_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DARE merge (drop and rescale; Yu et al. 2023, "Language Models are Super Mario"), csrc/dare.hip.  NO REFERENCE SITE: the
 * reference has no DARE; the arithmetic below is the specification and is pinned to a numpy restatement of it
 * (tests/dare_restatement.py), not to the reference.  One job = one output tensor with central tensor c (base), sources
 * W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), scalars lam and rescale (fp32), keep_below (in [1, 2^32]), seed, stream, mode;
 * fp32, one rounding per operation, no FMA, source order:
 *   1. t_m = W_m - c
 *   2. the draw of element i of source m:  u_m[i] = word (i & 3) of Philox4x32-10 with counter (i >> 2, 0, m, stream) and
 *      key (seed & 0xffffffff, seed >> 32): multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on counter word 2), key
 *      increments 0x9E3779B9 and 0xBB67AE85, ten rounds, the key bumped after each (csrc/philox.h).  i >> 2 < 2^32 always.
 *      One Philox call serves one float4 of one source; the ragged end of a tensor uses the same definition.
 *   3. kept = (uint64) u_m[i] < keep_below;  tt_m = t_m * rescale if kept else +0.0
 *   4. VLM_DARE_LINEAR: d = ((0 + tt_0) + tt_1) + ...
 *      VLM_DARE_TIES:   steps 3-4 of the TIES rule above on these tt_m (sign elected by comparison of the sum; d = mean of
 *                       the agreeing entries, +0.0 if none agrees)
 *   5. dst = c + lam * d
 * The mask costs no memory and a draw is a pure function of (seed, stream, m, i): the result does not depend on the grid, the
 * chunking, the position of the job in a plan or how often the plan runs.
 * Counters per job (uint64; integer atomics only): kept[0 .. MAX_SRC), then `conflict` = elements whose kept entries hold both a
 * positive and a negative value (tt_m > 0, tt_m < 0; both modes), then `empty` = elements where no source is kept (LINEAR) or
 * none agrees (TIES).
 * The pass is elementwise: dst may be EXACTLY base or EXACTLY one of the job's sources; any other overlap of dst's byte range with
 * an input's is VLM_ERR_ARG (overlap ACROSS jobs is the caller's to avoid).  Non-finite inputs are outside the contract.
 */
#define VLM_DARE_LINEAR 0
#define VLM_DARE_TIES 1

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t keep_below;                  /* step 3: 1 .. 2^32; 2^32 keeps everything */
  uint64_t seed;
  uint64_t n_elem;
  int32_t n_src;
  int32_t mode;                         /* VLM_DARE_LINEAR | VLM_DARE_TIES */
  float lam;
  float rescale;                        /* step 3: the caller's 1 / (1 - p), or 1 */
  uint32_t stream;                      /* counter word 3: which tensor */
  uint32_t reserved;
} vlm_dare_job_t;

/* The workspace of a DARE plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_chunks;
  uint64_t jobs_off;      /* vlm_dare_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_DARE_COUNTERS]: kept per source, conflict, empty */
} vlm_dare_header_t;
#define VLM_DARE_COUNTERS (VLM_MERGE_MAX_SRC + 2)

/* Bytes of device workspace a DARE plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table, counters).
 * No reference site. */
size_t vlm_dare_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_ties_plan_upload, except that dst may equal base or a source exactly; plus keep_below in
 * [1, 2^32] and a valid mode), build the chunk table on the host and copy header + jobs + table into `workspace` (16-byte
 * aligned).  SYNCHRONISES `stream` before it returns (pageable temporary source); it is the last host synchronisation of a plan.
 * Implements no step of the rule; no reference site. */
int vlm_dare_plan_upload(const vlm_dare_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: a tiny launch that zeroes the counters, then ONE streaming launch over all jobs (steps 1-5 and the
 * counters); no host synchronisation.  May be called again on the same workspace and gives the same bytes and counters.  One run
 * at a time per workspace.  No reference site. */
int vlm_dare_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Expert-pair statistics (L2 distance, cosine similarity, soft sign dissimilarity and its truncated form, sign conflicts),
 * csrc/pairstats.hip.  NO REFERENCE SITE: the reference ships no such measure; the arithmetic below is the specification and is
 * pinned to a numpy restatement of it (tests/pairstats_restatement.py), not to the reference.  One job = one tensor with sources
 * W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), an optional central tensor c (base, may be NULL) and one threshold key tkey[m]
 * per source.  A job writes no tensor.  Per element i; fp32 operations round once, no FMA; "f64" = the operand widened exactly
 * and the operation done in double, one rounding:
 *   1. x_m = W_m - c (fp32) with a base, else x_m = W_m;  key(x) = bits(x) & 0x7fffffff (the TIES key);  in_m = key(x_m) >= tkey[m]
 *   2. per source:  sq[m] += f64(x_m) * f64(x_m);  nnz[m] += (x_m != 0)
 *   3. per pair (a, b), a < b < S, in slot b (b - 1) / 2 + a (the slot does not depend on S):
 *        den = |x_a| + |x_b| (fp32);  live = den > 0;  r = |x_a + x_b| / den (fp32, correctly rounded) if live else +0.0
 *        conf = (x_a > 0 and x_b < 0) or (x_a < 0 and x_b > 0);  t = live and (in_a or in_b)
 *        dot += f64(x_a) * f64(x_b);  dist2 += d * d with d = f64(x_a) - f64(x_b);  ssd += f64(r);  tssd += t ? f64(r) : +0.0
 *        live += live;  conflict += conf;  tlive += t;  tconflict += (t and conf)
 * The order of summation is part of the rule, so a result is the same bytes whatever the grid, the job's place in a plan or the
 * number of runs.  Every accumulation starts at +0.0.
 *   thread     thread t of a 16-KiB chunk (256 threads) adds its float4s u = 0 .. 3 (float4 index start4 + t + 256 u) and in each
 *              the components 0 .. 3, in that order; then the ragged-tail element 4 n4 + t (n4 = n_elem / 4) if the chunk owns the
 *              tail and t < (n_elem & 3).  A thread with nothing in range contributes +0.0.
 *   wave       the 64 lanes are folded by halves, offsets 32, 16, 8, 4, 2, 1: after the first fold lane l holds v_l + v_{l+32}
 *   workgroup  the four waves are added as ((w0 + w1) + w2) + w3: the chunk's record
 *   job        the records of a job are added one after the other in chunk order
 * The integer statistics are plain sums.  Slots of sources and pairs a job does not have are zero.  Non-finite inputs are
 * outside the contract.  The derived measures (sqrt(dist2), dot / sqrt(sq_a sq_b), 1 - ssd / live, ...) are the caller's.
 */
#define VLM_PAIRSTATS_PAIRS 6   /* VLM_MERGE_MAX_SRC (VLM_MERGE_MAX_SRC - 1) / 2 */

typedef struct {
  const void* base;                     /* f32 [n_elem]: the central tensor c, or NULL */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t n_elem;
  uint32_t tkey[VLM_MERGE_MAX_SRC];     /* step 1: threshold keys; 0 puts every entry in */
  int32_t n_src;
  int32_t reserved;
} vlm_pairstats_job_t;

/* The workspace of a pair-statistics plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_chunks;
  uint64_t jobs_off;      /* vlm_pairstats_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t first_off;     /* uint64 [n_jobs + 1]: the first chunk of each job, then n_chunks */
  uint64_t records_off;   /* vlm_pairstats_result_t [n_chunks]: one record per chunk, overwritten by every run */
  uint64_t results_off;   /* vlm_pairstats_result_t [n_jobs]: overwritten by every run */
} vlm_pairstats_header_t;

/* per job after a run (and per chunk in between): 28 doubles, then 28 counts */
typedef struct {
  double sq[VLM_MERGE_MAX_SRC];
  double dot[6];
  double dist2[6];
  double ssd[6];
  double tssd[6];
  uint64_t nnz[VLM_MERGE_MAX_SRC];
  uint64_t live[6];
  uint64_t conflict[6];
  uint64_t tlive[6];
  uint64_t tconflict[6];
} vlm_pairstats_result_t;

/* Bytes of device workspace a pair-statistics plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table,
 * first-chunk table, one record per chunk, one result per job).  No reference site. */
size_t vlm_pairstats_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (pointers non-NULL and 16-byte aligned, base may be NULL; 1 <= n_src <= VLM_MERGE_MAX_SRC and n_elem > 0, else
 * VLM_ERR_ARG; a length or chunk count past 32 bits of float4s is VLM_ERR_UNSUPPORTED), build the chunk table on the host and
 * copy header + jobs + tables into `workspace` (16-byte aligned).  SYNCHRONISES `stream` before it returns (pageable temporary
 * source); it is the last host synchronisation of a plan.  Implements no step of the rule; no reference site. */
int vlm_pairstats_plan_upload(const vlm_pairstats_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes,
                              void* stream);
/* Run an uploaded plan: ONE streaming launch over all jobs (steps 1-3, one record per chunk), then one launch that adds every
 * job's records in chunk order; no atomics, no clearing launch, no host synchronisation.  The inputs are only read.  May be
 * called again on the same workspace and gives the same bytes.  One run at a time per workspace.  No reference site. */
int vlm_pairstats_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model Breadcrumbs merge (magnitude band trim; Davari & Belilovsky 2023), csrc/band.hip.  NO REFERENCE SITE: the reference has
 * no such merge; the arithmetic below is the specification and is pinned to a numpy restatement of it
 * (tests/band_restatement.py), not to the reference.  One job = one output tensor with central tensor c (base), sources
 * W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), scale lam, mode, and two ranks per source computed by the caller: k_hi[m] and
 * k_lo[m] with 0 <= k_hi[m] < k_lo[m] <= n_elem; fp32, one rounding per operation, no FMA, source order;
 * key(x) = bits(x) & 0x7fffffff (the TIES key):
 *   1. t_m = W_m - c
 *   2. thr_lo_m = the k_lo[m]-th largest key(t_m[i]) of the tensor;
 *      thr_hi_m = the k_hi[m]-th largest key if k_hi[m] >= 1, else 0x80000000 (above every key: nothing is an outlier);
 *      out_m[i]  = key(t_m[i]) >= thr_hi_m                      (the outliers)
 *      kept_m[i] = key(t_m[i]) >= thr_lo_m and not out_m[i]     (the band)
 *      tt_m[i]   = t_m[i] if kept_m[i] else +0.0
 *      So every entry equal to the lower threshold is kept (as in TIES), every entry equal to the upper threshold is dropped, and
 *      a source whose two thresholds are the same key contributes nothing: a defined result, not an error.
 *   3. VLM_BAND_LINEAR: d = ((0 + tt_0) + tt_1) + ...
 *      VLM_BAND_TIES:   steps 3-4 of the TIES rule above on these tt_m (sign elected by comparison of the sum; d = mean of
 *                       the agreeing entries, +0.0 if none agrees)
 *   4. dst = c + lam * d
 * With k_hi = 0 and VLM_BAND_TIES this is the TIES rule with k = k_lo.
 * Counters per job (uint64; integer atomics only, so nothing depends on the order workgroups run in): kept[0 .. MAX_SRC) =
 * entries with kept_m, then outlier[0 .. MAX_SRC) = entries with out_m, then `conflict` = elements whose kept entries hold both
 * a positive and a negative value (tt_m > 0, tt_m < 0; both modes), then `empty` = elements where no source's entry is kept
 * (LINEAR) or none agrees (TIES).
 * dst must not overlap base or a source of its own job (the selection passes re-read them; vlm_band_plan_upload rejects such a
 * job as vlm_ties_plan_upload does -- overlap ACROSS jobs is the caller's to avoid).  Non-finite inputs are outside the contract.
 */
#define VLM_BAND_LINEAR 0
#define VLM_BAND_TIES 1

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t k_hi[VLM_MERGE_MAX_SRC];     /* step 2: the largest k_hi entries per source are outliers; 0: none */
  uint64_t k_lo[VLM_MERGE_MAX_SRC];     /* step 2: entries below the k_lo-th largest are dropped */
  uint64_t n_elem;
  int32_t n_src;
  int32_t mode;                         /* VLM_BAND_LINEAR | VLM_BAND_TIES */
  float lam;
  uint32_t reserved;
} vlm_band_job_t;

/* The workspace of a band plan BEGINS with this header (byte offsets from its start): vlm_ties_header_t's fields with the band
 * types behind them.  Jobs keep their upload order; the (job, source) pairs ("units") are numbered job-major, source-minor. */
typedef struct {
  uint64_t n_jobs, n_units, n_chunks;
  uint64_t jobs_off;      /* vlm_band_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t unit0_off;     /* uint32 [n_jobs]: first unit of each job */
  uint64_t units_off;     /* {uint32 job, uint32 source} [n_units] */
  uint64_t state_off;     /* vlm_band_state_t [n_units] */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_BAND_COUNTERS] */
  uint64_t hist_off;      /* uint64 [n_units][2048]: selection histograms (pass 0: one of 2048 bins serves both ranks; passes 1
                             and 2: 1024 bins for k_lo, then 1024 for k_hi), zero between runs */
} vlm_band_header_t;
typedef struct {
  uint32_t key_lo;    /* after a run: thr_lo_m as a key (= the bits of the threshold magnitude) */
  uint32_t key_hi;    /* after a run: thr_hi_m as a key; 0x80000000 when k_hi = 0 */
  uint64_t rank_lo;   /* after a run: 1 + how many of the keys equal to thr_lo_m rank above the k_lo-th place */
  uint64_t rank_hi;   /* the same for thr_hi_m and k_hi; 0 when k_hi = 0 */
} vlm_band_state_t;
/* per job after a run: kept[0 .. MAX_SRC), outlier[0 .. MAX_SRC), conflict, empty (see above) */
#define VLM_BAND_COUNTERS (2 * VLM_MERGE_MAX_SRC + 2)

/* Bytes of device workspace a band plan for n_jobs jobs over total_elems elements needs (jobs, chunk table, selection state,
 * histograms, counters): what a TIES plan needs but for the wider jobs, states and counters.  No reference site. */
size_t vlm_band_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_ties_plan_upload; a valid mode and 0 <= k_hi[m] < k_lo[m] <= n_elem, else VLM_ERR_ARG),
 * build the chunk table on the host, copy header + jobs + tables into `workspace` (16-byte aligned) and zero the histograms.
 * SYNCHRONISES `stream` before it returns (pageable temporary source); it is the last host synchronisation of a plan.
 * Implements no step of the rule; no reference site. */
int vlm_band_plan_upload(const vlm_band_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: step 2's two thresholds per source by ONE radix select (three histogram launches over all jobs, 11 + 10 +
 * 10 key bits -- the first histogram serves both ranks, the later ones count each rank's prefix in its half of the bins -- each
 * followed by a tiny launch that picks both bins on the device), then steps 1-4 plus the counters (one launch); seven launches,
 * four streaming passes, no host synchronisation.  May be called again on the same workspace and gives the same bytes and
 * counters: the run zeroes its own histograms and counters on the stream.  One run at a time per workspace.  No reference site. */
int vlm_band_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DELLA merge (magnitude-ranked drop and rescale; Deep et al. 2024, "DELLA-Merging: Reducing Interference in Model Merging
 * through Magnitude-Based Sampling"), csrc/della.hip.  NO REFERENCE SITE: the reference has no DELLA; the arithmetic below is the
 * specification and is pinned to a numpy restatement of it (tests/della_restatement.py), not to the reference.  One job = one
 * output tensor with central tensor c (base), sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), n_elem and row_len = L with
 * 1 <= L <= VLM_DELLA_MAX_ROW and n_elem % L == 0, the window keep_lo, keep_hi (1 <= keep_lo <= keep_hi <= 2^32), seed, stream,
 * mode, lam (fp32) and rescale (0 | 1); fp32, one rounding per operation, no FMA, source order:
 *   1. t_m = W_m - c
 *   2. key(x) = bits(x) & 0x7fffffff (the TIES key).  The row of element i is i / L.  r_m[i] = the number of elements j of the
 *      same row with key(t_m[j]) < key(t_m[i]), or with equal keys and j < i: a permutation of 0 .. L-1 in every row, rank 0 the
 *      smallest magnitude; ties, zeros and +-x pairs are ordered by index.
 *   3. kb_m[i] = keep_lo + floor((keep_hi - keep_lo) * r_m[i] / (L - 1)) for L > 1, in unsigned 64-bit integers (the product is
 *      below 2^44);  for L = 1: keep_lo + ((keep_hi - keep_lo) >> 1).
 *   4. u_m[i] = step 2 of the DARE rule above: word (i & 3) of Philox4x32-10 with counter (i >> 2, 0, m, stream) and key
 *      (seed & 0xffffffff, seed >> 32); i is the FLAT index in the tensor, not the index in the row.
 *   5. kept = (uint64) u_m[i] < kb_m[i];  scale = rescale ? 4294967296.0f / (float) kb_m[i] : 1.0f (the conversion rounds to
 *      nearest even, the division is correctly rounded);  tt_m = t_m * scale if kept else +0.0
 *   6. VLM_DELLA_LINEAR: d = ((0 + tt_0) + tt_1) + ...
 *      VLM_DELLA_TIES:   steps 3-4 of the TIES rule above on these tt_m
 *   7. dst = c + lam * d
 * With keep_lo == keep_hi the ranks drop out and steps 4-7 are the DARE rule with keep_below = keep_lo and rescale = scale.
 * Nothing in the result depends on the grid, on where a job stands in a plan or on how often the plan runs.
 * Counters per job (uint64; integer atomics only), DARE's: kept[0 .. MAX_SRC), then `conflict`, then `empty`.
 * dst must not overlap base or a source of its own job (vlm_della_plan_upload rejects such a job as vlm_ties_plan_upload does --
 * overlap ACROSS jobs is the caller's to avoid).  Non-finite inputs are outside the contract.
 */
#define VLM_DELLA_LINEAR 0
#define VLM_DELLA_TIES 1
#define VLM_DELLA_MAX_ROW 4096

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t keep_lo;                     /* step 3: the keep threshold of rank 0, 1 .. keep_hi */
  uint64_t keep_hi;                     /* step 3: the keep threshold of rank L - 1, keep_lo .. 2^32 */
  uint64_t seed;
  uint64_t n_elem;
  uint32_t row_len;                     /* L: 1 .. VLM_DELLA_MAX_ROW, divides n_elem */
  int32_t n_src;
  int32_t mode;                         /* VLM_DELLA_LINEAR | VLM_DELLA_TIES */
  int32_t rescale;                      /* step 5: 0 | 1 */
  float lam;
  uint32_t stream;                      /* counter word 3: which tensor */
} vlm_della_job_t;

/* The workspace of a DELLA plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_tiles;
  uint64_t jobs_off;      /* vlm_della_job_t [n_jobs] */
  uint64_t tiles_off;     /* {uint32 job, uint32 first row} [n_tiles]: a tile is as many whole rows as fit in 4096 elements */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_DELLA_COUNTERS]: kept per source, conflict, empty */
} vlm_della_header_t;
#define VLM_DELLA_COUNTERS (VLM_MERGE_MAX_SRC + 2)

/* Bytes of device workspace a DELLA plan for n_jobs jobs over total_elems elements needs (header, jobs, tile table, counters).
 * No reference site. */
size_t vlm_della_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_ties_plan_upload; row_len in [1, VLM_DELLA_MAX_ROW] and fewer than 2^32 rows, else
 * VLM_ERR_UNSUPPORTED; n_elem % row_len == 0, 1 <= keep_lo <= keep_hi <= 2^32, a valid mode and rescale in {0, 1}, else
 * VLM_ERR_ARG), build the tile table on the host and copy header + jobs + table into `workspace` (16-byte aligned).
 * SYNCHRONISES `stream` before it returns (pageable temporary source); it is the last host synchronisation of a plan.
 * Implements no step of the rule; no reference site. */
int vlm_della_plan_upload(const vlm_della_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: a tiny launch that zeroes the counters, then ONE streaming launch over all jobs (steps 1-7 and the
 * counters; the ranks of a tile's rows are made in LDS, so the inputs are read once); no host synchronisation.  May be called
 * again on the same workspace and gives the same bytes and counters.  One run at a time per workspace.  No reference site. */
int vlm_della_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model Stock merge (angle-derived interpolation ratio; Jang, Yun & Han, ECCV 2024), csrc/stock.hip.  NO REFERENCE SITE: the
 * reference has no such merge; the arithmetic below is the specification and is pinned to a numpy restatement of it
 * (tests/stock_restatement.py), not to the reference.  One job = one output tensor with central tensor c (base, required) and
 * sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC); no scalar parameter.  fp32 operations round once, no FMA; "f64" = the
 * operand widened exactly and the operation done in double, one rounding:
 *   1. x_m = W_m - c (fp32)
 *   2. sq[m] = sum f64(x_m) * f64(x_m);  per pair (a, b), a < b < S, in slot b (b - 1) / 2 + a:  dot[p] = sum f64(x_a) * f64(x_b).
 *      These are steps 2-3 of the pair-statistics rule above restricted to these two sums, in that rule's order of summation
 *      (thread, wave by halves, ((w0 + w1) + w2) + w3, records in chunk order, every sum from +0.0): sq and dot are the bytes
 *      vlm_pairstats_run leaves for the same inputs with a base.
 *   3. per job, in f64, one rounding per operation:
 *        den_p = sqrt(sq[a] * sq[b]);  cos_p = den_p > 0 ? dot[p] / den_p : +0.0
 *        cos = (((+0.0 + cos_0) + cos_1) + ...) / NP,  NP = S (S - 1) / 2
 *        cc = cos > 0 ? (cos < 1 ? cos : 1.0) : 0.0   (decided by these comparisons: a NaN gives 0)
 *        t = (S * cc) / (1 + (S - 1) * cc)
 *        S = 1 has no pair: cos = +0.0 is recorded and t = 1.0
 *        scale = f32(t / S): f64 division, then one rounding to fp32
 *   4. d = ((+0.0 + x_0) + x_1) + ... (fp32, source order);  dst = c + scale * d
 * This is t * mean(W) + (1 - t) * c with the paper's t = N cos / (1 + (N - 1) cos), cos the mean pairwise cosine of the task
 * vectors.  Clamping cos to [0, 1] keeps t in [0, 1] (the formula has a pole at cos = -1 / (N - 1)): experts that point apart
 * get the anchor back.  Non-finite inputs are outside the contract.  dst must not overlap base or a source of its own job (two
 * passes read them; vlm_stock_plan_upload rejects such a job as vlm_ties_plan_upload does -- overlap ACROSS jobs is the
 * caller's to avoid).  A run leaves the same bytes whatever the grid, the job's place in a plan or the number of runs: no
 * atomics, nothing to clear.  Step 3 runs on the device: fp64 multiply, divide and square root are correctly rounded there.
 */
typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t n_elem;
  int32_t n_src;
  int32_t reserved;
} vlm_stock_job_t;

/* The workspace of a Model Stock plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_chunks;
  uint64_t jobs_off;      /* vlm_stock_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t first_off;     /* uint64 [n_jobs + 1]: the first chunk of each job, then n_chunks */
  uint64_t records_off;   /* double [n_chunks][10]: one record per chunk, sq[4] then dot[6], overwritten by every run */
  uint64_t results_off;   /* vlm_stock_result_t [n_jobs]: overwritten by every run */
} vlm_stock_header_t;
#define VLM_STOCK_SUMS (VLM_MERGE_MAX_SRC + VLM_PAIRSTATS_PAIRS)   /* the doubles of a record */

/* per job after a run; slots of sources and pairs a job does not have are zero */
typedef struct {
  double sq[VLM_MERGE_MAX_SRC];         /* step 2 */
  double dot[6];
  double cos_pair[6];                   /* step 3: cos_p */
  double cos;                           /* the mean, unclamped */
  double t;
  float scale;                          /* f32(t / S): what step 4 multiplies by */
  uint32_t reserved;
} vlm_stock_result_t;

/* Bytes of device workspace a Model Stock plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table,
 * first-chunk table, one record per chunk, one result per job).  No reference site. */
size_t vlm_stock_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_ties_plan_upload: pointers non-NULL and 16-byte aligned, base required, 1 <= n_src <=
 * VLM_MERGE_MAX_SRC and n_elem > 0, dst's byte range meets no input's, else VLM_ERR_ARG; a length or chunk count past 32 bits of
 * float4s is VLM_ERR_UNSUPPORTED), build the chunk table on the host and copy header + jobs + tables into `workspace` (16-byte
 * aligned; VLM_ERR_WORKSPACE if it is too small).  SYNCHRONISES `stream` before it returns (pageable temporary source); it is
 * the last host synchronisation of a plan.  Implements no step of the rule; no reference site. */
int vlm_stock_plan_upload(const vlm_stock_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: three launches, stream-ordered, and nothing else -- the reducer over all jobs (steps 1-2, one record per
 * chunk), the fold (a job's records in chunk order, then step 3: the whole result), the apply pass (steps 1 and 4, `scale`
 * read from the job's result); no host synchronisation.  May be called again on the same workspace and gives the same bytes.
 * One run at a time per workspace.  No reference site. */
int vlm_stock_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SCE merge (select, calculate, erase; Wan et al. 2024, "FuseChat: Knowledge Fusion of Chat Models"; the `sce` method of
 * mergekit), csrc/sce.hip.  NO REFERENCE SITE: the reference has no such merge; the arithmetic below is the specification and is
 * pinned to a numpy restatement of it (tests/sce_restatement.py), not to the reference.  One job = one output tensor with central
 * tensor c (base, required), sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), a rank k (1 <= k <= n_elem) and a scale lam.
 * fp32 operations round once, no FMA, fp32 division is correctly rounded; "f64" = the operand widened exactly and the operation
 * done in double, one rounding; key(x) = bits(x) & 0x7fffffff (the TIES key):
 *   1. x_m = W_m - c (fp32)
 *   2. per element:  mean = (((+0.0 + x_0) + x_1) + ...) / f32(S);  e_m = x_m - mean;
 *      q = ((+0.0 + e_0 e_0) + e_1 e_1) + ...;  var = q / f32(S)
 *   3. select: thr = the k-th largest key(var[i]) of the tensor;  sel[i] = key(var[i]) >= thr (every element equal to the
 *      threshold is selected, as in TIES)
 *   4. calculate: sq[m] = sum over the tensor of (sel ? f64(x_m) * f64(x_m) : +0.0), in the pair-statistics rule's order of
 *      summation (thread, wave by halves, ((w0 + w1) + w2) + w3, records in chunk order, every sum from +0.0)
 *   5. per job, in f64, on the device:  tot = ((+0.0 + sq[0]) + sq[1]) + ...;
 *      w_m = tot > 0 ? f32(sq[m] / tot) : f32(1.0 / S)   (the comparison decides: a NaN gives the uniform weights)
 *   6. erase, per element:  tt_m = sel ? x_m : +0.0;  s = ((+0.0 + tt_0) + tt_1) + ...;
 *      source m agrees iff (s > 0 and tt_m > 0) or (s < 0 and tt_m < 0) (the TIES election);  over the agreeing m, in source
 *      order:  num = ((+0.0 + w_a tt_a) + w_b tt_b) + ...,  den = ((+0.0 + w_a) + w_b) + ...;  d = den > 0 ? num / den : +0.0
 *   7. dst = c + lam * d
 * Counters per job (integer atomics only): `kept` = elements with sel (ONE count, not one per source), `conflict` = elements
 * with a positive and a negative value among the tt_m, `empty` = elements where no entry agrees.
 * Two differences from mergekit's form, on purpose:  k is the caller's rank over ALL n_elem elements (the host passes
 * K = max(1, min(n, ceil(density n))), the TIES count; mergekit takes int(density * count_nonzero(var)));  a zero sum s elects
 * nothing (mergekit elects + and clamps the denominator at 1e-6).
 * S = 1 is the task-vector job: every var is +0.0, everything is selected, w_0 = 1, dst = c + lam * x_0.  k = n_elem goes through
 * the same path with thr the smallest key.  Non-finite inputs are outside the contract.  dst must not overlap base or a source
 * of its own job (five passes read them; vlm_sce_plan_upload rejects such a job as vlm_ties_plan_upload does -- overlap ACROSS
 * jobs is the caller's to avoid).
 */
typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  uint64_t k;                           /* elements to select (step 3) */
  uint64_t n_elem;
  int32_t n_src;
  float lam;
} vlm_sce_job_t;

/* The workspace of an SCE plan BEGINS with this header (byte offsets from its start): vlm_ties_header_t's fields -- with ONE
 * selection unit per job, so n_units == n_jobs and a job's state is its whole result -- then the reducer's two tables. */
typedef struct {
  uint64_t n_jobs, n_units, n_chunks;
  uint64_t jobs_off;      /* vlm_sce_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t unit0_off;     /* uint32 [n_jobs]: the unit of each job (its own index) */
  uint64_t units_off;     /* {uint32 job, uint32 0} [n_units] */
  uint64_t state_off;     /* vlm_sce_result_t [n_jobs]: overwritten by every run */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_SCE_COUNTERS] */
  uint64_t hist_off;      /* uint64 [n_jobs][2048]: selection histograms, zero between runs */
  uint64_t first_off;     /* uint64 [n_jobs + 1]: the first chunk of each job, then n_chunks */
  uint64_t records_off;   /* double [n_chunks][VLM_MERGE_MAX_SRC]: one record of sq per chunk, overwritten by every run */
} vlm_sce_header_t;
/* per job after a run; slots of sources a job does not have are zero */
typedef struct {
  uint32_t key;       /* step 3: thr as a key (= the bits of the threshold variance) */
  uint32_t reserved;
  uint64_t rank;      /* 1 + how many of the keys equal to thr rank above the k-th place */
  double sq[VLM_MERGE_MAX_SRC];         /* step 4 */
  double tot;                           /* step 5 */
  float w[VLM_MERGE_MAX_SRC];           /* step 5: what step 6 multiplies by */
} vlm_sce_result_t;
/* per job after a run: kept, conflict, empty */
#define VLM_SCE_COUNTERS 3

/* Bytes of device workspace an SCE plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table, unit and
 * first-chunk tables, one result and one histogram per job, counters, one record per chunk).  No reference site. */
size_t vlm_sce_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_ties_plan_upload: pointers non-NULL and 16-byte aligned, base required, 1 <= n_src <=
 * VLM_MERGE_MAX_SRC and n_elem > 0, 1 <= k <= n_elem, dst's byte range meets no input's, else VLM_ERR_ARG; a length or chunk
 * count past 32 bits of float4s is VLM_ERR_UNSUPPORTED), build the chunk table on the host, copy header + jobs + tables into
 * `workspace` (16-byte aligned; VLM_ERR_WORKSPACE if it is too small) and zero the histograms.  SYNCHRONISES `stream` before it
 * returns (pageable temporary source); it is the last host synchronisation of a plan.  Implements no step of the rule; no
 * reference site. */
int vlm_sce_plan_upload(const vlm_sce_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: nine launches, stream-ordered, and nothing else -- steps 1-3 (three histogram launches over all jobs,
 * 11 + 10 + 10 bits of key(var), each followed by the tiny launch that picks the bin of the k-th largest key), the reducer
 * (steps 1-4 with the threshold read from the job's result, one record per chunk), the fold (a job's records in chunk order,
 * then step 5: the whole result) and the apply pass (steps 1-3 again and 6-7 with thr and w read from the job's result, plus the
 * counters); no host synchronisation.  var and sel are recomputed by every pass: nothing per element is stored between passes,
 * so a run streams the inputs five times and writes the output once.  May be called again on the same workspace and gives the
 * same bytes and counters: the run zeroes its own histograms and counters on the stream.  One run at a time per workspace.
 * No reference site. */
int vlm_sce_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spherical merge: SLERP for two sources, the weighted Karcher (Riemannian) mean of the directions for more (mergekit's
 * `nuslerp` with its `row_wise` option, `karcher`, `multislerp`), csrc/sphere.hip.  NO REFERENCE SITE: the reference has no such
 * merge; the arithmetic below is the specification and is pinned to a restatement of it in numpy and python doubles
 * (tests/sphere_restatement.py), not to the reference.  One job = one output tensor with sources W_0 .. W_{S-1} (1 <= S <=
 * VLM_MERGE_MAX_SRC), an optional central tensor c (base, may be NULL), weights w[m] >= 0 (doubles, not all zero), lam (fp32) and
 * row_len: 0 = the GROUP is the whole tensor, otherwise 1 <= row_len <= VLM_DELLA_MAX_ROW divides n_elem and a group is a row.
 * The coefficients are one scalar per source and per group.  fp32 and f64 operations round once, no FMA; "f64" = the operand
 * widened exactly and the operation done in double:
 *   1. x_m = W_m - c (fp32);  x_m = W_m without a base
 *   2. per group:  sq[m] = sum f64(x_m) * f64(x_m);  per pair (a, b), a < b < S, in slot b (b - 1) / 2 + a:
 *      dot[p] = sum f64(x_a) * f64(x_b).
 *      Tensor groups: step 2 of the Model Stock rule above, order of summation included (csrc/gram_reduce.h serves both): sq and
 *      dot are the bytes vlm_stock_run leaves for the same inputs.
 *      Row groups: lane l of 64 adds the products of the row's elements l, l + 64, l + 128, ... in rising order, from +0.0; the 64
 *      lane sums are folded by halves (l + 32 into l, then 16, 8, 4, 2, 1).  The order depends on row_len alone.
 *   3. per group, in f64, in the order written; ITERS = 24, EDGE = 2^-20, QMIN = 2^-40; acos, sin, cos are the device library's
 *      f64 functions, everything else is one correctly rounded operation:
 *        ws = ((+0.0 + w[m0]) + w[m1]) + ... over the m with sq[m] > 0, in source order
 *        if not ws > 0:  status = ZERO;  coef64[:] = +0.0;  rho = resid = +0.0;  done
 *        ww[m] = sq[m] > 0 ? w[m] / ws : +0.0;   n[m] = sqrt(sq[m])
 *        C[i][i] = 1;  C[i][j] = (ww[i] > 0 and ww[j] > 0) ? dot[slot(i, j)] / (n[i] * n[j]) : +0.0
 *        nrm2(v):  t = +0.0;  for i: for j:  t = t + (v[i] * v[j]) * C[i][j]          (i, j over 0 .. S-1, i outer)
 *        rho = ((+0.0 + ww[0] * n[0]) + ww[1] * n[1]) + ...
 *        a = ww;  q = nrm2(a)
 *        if not q > QMIN:  status = LINEAR;  coef64[m] = ww[m];  resid = +0.0;  done       (antipodal: plain interpolation)
 *        r = sqrt(q);  a[j] = a[j] / r;  vn = +0.0
 *        repeat ITERS times (no tolerance test: the count is part of the rule):
 *          v[:] = +0.0
 *          for i with ww[i] > 0, in order:
 *            ci = ((+0.0 + a[0] * C[0][i]) + a[1] * C[1][i]) + ...
 *            k = 1 if ci >= 1 - EDGE;  k = 0 if ci <= -1 + EDGE;  else th = acos(ci), k = th / sin(th)
 *            for j:  v[j] = v[j] + (ww[i] * k) * ((j == i ? 1.0 : +0.0) - ci * a[j])
 *          q = nrm2(v);  if not q > 0: vn = +0.0, break            (the step has vanished)
 *          vn = sqrt(q);  cv = cos(vn);  sv = sin(vn) / vn (the library's sincos);  b[j] = cv * a[j] + sv * v[j]
 *          q2 = nrm2(b);  if not q2 > QMIN: break
 *          r = sqrt(q2);  a[j] = b[j] / r
 *        status = OK;  coef64[m] = ww[m] > 0 ? (rho * a[m]) / n[m] : +0.0;  resid = vn (the size of the last step)
 *        coef32[m] = f32(coef64[m])     (one rounding)
 *   4. per element, fp32:  d = +0.0;  for m in order: d = d + coef32[m] * x_m (multiply, then add);
 *      dst = c + lam * d with a base;  dst = d without one (then lam must be 1.0).
 * This is the weighted Karcher mean of the unit vectors x_m / |x_m|, iterated in the coordinates of the sources themselves (so it
 * needs the S x S Gram matrix and no second reduction), scaled by the weighted mean rho of the norms.  For S = 2 and
 * w = (1 - t, t) it is SLERP(t) of the directions with the norm interpolated linearly: mergekit's `nuslerp`.  mergekit's plain
 * `slerp` does NOT renormalise (it interpolates the unnormalised tensors with the angle's weights); that form is not offered.
 * An exactly opposite pair with equal weights takes LINEAR; with unequal weights the iteration converges to the heavier side.
 * Inputs without a unique mean (more directions than dimensions, say) stay finite and deterministic but are sensitive to the last
 * bits of acos / sin / cos.  Non-finite inputs are outside the contract.
 * Per job after a run, vlm_sphere_result_t.  A tensor job fills sq, dot, coef64, coef32, rho, resid and status; a row job leaves
 * those zero and fills the row counters: rows_linear and rows_zero (integer atomics) and resid_max (the maximum of non-negative
 * doubles, taken as an integer maximum of their bits: order-free).  coef_out, where given, receives coef32 of every group
 * (float [n_groups][VLM_MERGE_MAX_SRC], slots past S zero; n_groups = 1 for a tensor job).
 * A run leaves the same bytes whatever the grid, the job's place in a plan or the number of runs.  dst must not overlap base or
 * a source of its own job; coef_out must meet none of the job's tensors (overlap ACROSS jobs is the caller's to avoid).
 */
#define VLM_SPHERE_OK 0
#define VLM_SPHERE_LINEAR 1
#define VLM_SPHERE_ZERO 2
#define VLM_SPHERE_ITERS 24

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c, or NULL */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each */
  void* coef_out;                       /* device f32 [n_groups][VLM_MERGE_MAX_SRC], 16-byte aligned, or NULL */
  double w[VLM_MERGE_MAX_SRC];          /* step 3: the weights, >= 0, finite, not all zero */
  uint64_t n_elem;
  uint32_t row_len;                     /* 0: one group, the tensor; else 1 .. VLM_DELLA_MAX_ROW, divides n_elem: a group is a row */
  int32_t n_src;
  float lam;                            /* step 4; 1.0 without a base */
  uint32_t reserved;
} vlm_sphere_job_t;

/* The workspace of a spherical plan BEGINS with this header (byte offsets from its start); jobs keep their upload order.  Tensor
 * jobs own the chunks, row jobs the tiles: first[i] == first[i + 1] for a row job. */
typedef struct {
  uint64_t n_jobs, n_chunks, n_tiles;
  uint64_t jobs_off;      /* vlm_sphere_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table of the tensor jobs */
  uint64_t tiles_off;     /* {uint32 job, uint32 first row} [n_tiles]: the row jobs' tiles, as many whole rows as fit in 4096 elements */
  uint64_t first_off;     /* uint64 [n_jobs + 1]: the first chunk of each job, then n_chunks */
  uint64_t records_off;   /* double [n_chunks][10]: one record per chunk, sq[4] then dot[6], overwritten by every run */
  uint64_t results_off;   /* vlm_sphere_result_t [n_jobs]: overwritten by every run */
} vlm_sphere_header_t;

/* per job after a run; slots of sources and pairs a job does not have are zero */
typedef struct {
  double sq[VLM_MERGE_MAX_SRC];         /* step 2 (tensor job) */
  double dot[6];
  double coef64[VLM_MERGE_MAX_SRC];     /* step 3 (tensor job) */
  double rho;
  double resid;
  float coef32[VLM_MERGE_MAX_SRC];      /* what step 4 multiplies by */
  uint32_t status;                      /* VLM_SPHERE_OK | _LINEAR | _ZERO (tensor job; a row job: OK) */
  uint32_t reserved;
  uint64_t rows_linear;                 /* row job: rows whose status is LINEAR */
  uint64_t rows_zero;                   /* row job: rows whose status is ZERO */
  double resid_max;                     /* row job: the largest resid of its rows */
} vlm_sphere_result_t;

/* Bytes of device workspace a spherical plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk and tile
 * tables, first-chunk table, one record per chunk, one result per job).  No reference site. */
size_t vlm_sphere_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_stock_plan_upload, but base may be NULL; coef_out NULL or 16-byte aligned and meeting none of
 * the job's tensors; every w[m], m < n_src, finite and >= 0 and not all of them zero; row_len == 0, or n_elem % row_len == 0 with
 * 1 <= row_len <= VLM_DELLA_MAX_ROW; lam == 1 without a base; else VLM_ERR_ARG; a length, chunk, tile or row count past 32 bits
 * is VLM_ERR_UNSUPPORTED), build both tables on the host and copy header + jobs + tables into `workspace` (16-byte aligned;
 * VLM_ERR_WORKSPACE if it is too small).  SYNCHRONISES `stream` before it returns (pageable temporary source); it is the last
 * host synchronisation of a plan.  Implements no step of the rule; no reference site. */
int vlm_sphere_plan_upload(const vlm_sphere_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: four launches, stream-ordered, and nothing else -- for the tensor jobs Model Stock's three (the reducer,
 * steps 1-2; the fold, a job's records in chunk order, then step 3 by one lane: the whole result -- it also zeroes the row jobs'
 * results; the apply pass, steps 1 and 4 with coef32 read from the job's result), for the row jobs ONE launch over their tiles
 * (steps 1-4: a tile's inputs are read from memory once, its task vectors are kept in LDS for steps 2 and 4, step 3 runs one row per
 * lane); no host synchronisation.  May be called again on the same workspace and gives the same bytes.  One run at a time per
 * workspace.  No reference site. */
int vlm_sphere_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Consensus merge with TALL masks (Wang et al., "Localizing Task Information for Improved Model Merging and Compression", ICML
 * 2024), csrc/tall.hip.  NO REFERENCE SITE: the reference has no such merge; the arithmetic below is the specification and is
 * pinned to a numpy restatement of it (tests/tall_restatement.py), not to the reference.  One VLM_TALL_CONSENSUS job = one output
 * tensor with central tensor c (base, required), sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), tall_lambda >= 0 (fp32), an
 * integer k in [0, S] and lam (fp32); fp32, one rounding per operation, no FMA, source order:
 *   1. x_m = W_m - c
 *   2. d = ((0 + x_0) + x_1) + ...                  (the multi-task vector, in the order of the LINEAR combine)
 *   3. r_m = d - x_m;  keep_m = |x_m| >= tall_lambda * |r_m|   (the product rounds once; the comparison is >=, so a NaN keeps
 *      nothing and 0 >= 0 keeps a zero entry, as in the paper)
 *   4. votes = sum_m keep_m;  sel = votes >= k
 *   5. dst = c + lam * (sel ? d : +0.0)
 *   6. if the job has masks: word w of source m's mask has bit b (bit 0 = least significant) equal to keep_m[32 w + b].  A mask
 *      has ceil(n_elem / 32) 32-bit words; every word is written by every run, and the bits at positions >= n_elem are 0.  On a
 *      little-endian host the mask reads as numpy.unpackbits(words.view(uint8), bitorder="little")[:n_elem].
 * k = 0 is plain task arithmetic, c + lam * d; k = 2 drops what only one expert cares about ("selfish") and what none does
 * ("catastrophic").  S = 1 keeps everything (r_0 = 0).
 * Counters per job (uint64; integer atomics only, so nothing depends on the order workgroups run in), in the slots of the TIES
 * counters: kept[0 .. MAX_SRC) = the bits set in mask m, then `selected` = the elements with sel, then `empty` = the elements
 * with votes == 0.
 * A VLM_TALL_RESTORE job rebuilds one expert from the unified tensor: n_src = 1, src[0] = u, base = c, mask[0] = a packed mask
 * (an INPUT), and dst[i] = bit_i ? u[i] : c[i] -- a select, no arithmetic; k, tall_lambda and lam are not read (k in [0, 1] and
 * tall_lambda >= 0 are still checked).  With u the k = 0, lam = 1 output of the rule above this is float32(c + keep_m * d), the
 * paper's reconstruction.  Its counters: kept[0] = the elements taken from u; `selected` and `empty` stay 0.  The mask is read
 * up to word ceil(n_elem / 32) - 1 and no further; bits at positions >= n_elem are ignored.  One job restores one expert: a second
 * expert is a second job that reads u and c again.
 * Both ops are elementwise: dst may be EXACTLY base or EXACTLY one of the job's sources; any other overlap of dst's byte range with
 * an input's is VLM_ERR_ARG, and so is a mask whose 4 ceil(n_elem / 32) bytes meet dst, the base, a source or another mask of the
 * same job (overlap ACROSS jobs is the caller's to avoid).  Non-finite inputs are outside the contract.  A run leaves the same
 * bytes, words and counters whatever the grid, the job's place in a plan or the number of runs.
 */
#define VLM_TALL_CONSENSUS 0
#define VLM_TALL_RESTORE 1

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each; RESTORE: src[0] = the unified tensor u */
  void* mask[VLM_MERGE_MAX_SRC];        /* u32 [ceil(n_elem / 32)] each, 16-byte aligned.  CONSENSUS: outputs, all NULL or all
                                           n_src set; RESTORE: mask[0] is the input */
  uint64_t n_elem;
  int32_t n_src;
  int32_t op;                           /* VLM_TALL_CONSENSUS | VLM_TALL_RESTORE */
  int32_t k;                            /* step 4: 0 .. n_src */
  float tall_lambda;                    /* step 3: >= 0 */
  float lam;                            /* step 5 */
  uint32_t reserved;
} vlm_tall_job_t;

/* The workspace of a consensus plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_chunks;
  uint64_t jobs_off;      /* vlm_tall_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t counters_off;  /* uint64 [n_jobs][VLM_TALL_COUNTERS]: kept per source, selected, empty */
} vlm_tall_header_t;
#define VLM_TALL_COUNTERS (VLM_MERGE_MAX_SRC + 2)

/* Bytes of device workspace a consensus plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table,
 * counters).  The masks are the caller's tensors, not part of the workspace.  No reference site. */
size_t vlm_tall_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_dare_plan_upload on dst, base, the sources and the length; a valid op, k in [0, n_src] and
 * tall_lambda >= 0 and not NaN; a RESTORE job has n_src == 1 and mask[0]; a CONSENSUS job has no mask or one per source; every mask
 * 16-byte aligned and clear of the job's tensors and other masks; else VLM_ERR_ARG), build the chunk table on the host and copy
 * header + jobs + table into `workspace` (16-byte aligned; VLM_ERR_WORKSPACE if it is too small).  SYNCHRONISES `stream` before it
 * returns (pageable temporary source); it is the last host synchronisation of a plan.  Implements no step of the rule; no
 * reference site. */
int vlm_tall_plan_upload(const vlm_tall_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: a tiny launch that zeroes the counters, then ONE streaming launch over all jobs of both ops (steps 1-6
 * and the counters; the select of a RESTORE job); no host synchronisation.  May be called again on the same workspace and gives
 * the same bytes, mask words and counters.  One run at a time per workspace.  No reference site. */
int vlm_tall_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EMR-Merging (Huang et al., "EMR-Merging: Tuning-Free High-Performance Model Merging", NeurIPS 2024: elect, mask and rescale),
 * csrc/emr.hip.  NO REFERENCE SITE: the reference has no such merge; the arithmetic below is the specification and is pinned to a
 * numpy restatement of it (tests/emr_restatement.py), not to the reference.  One VLM_EMR_MERGE job = one output tensor with central
 * tensor c (base, required), sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), a scale lam (fp32) and either no mask pointers
 * or one per source.  fp32 operations round once, no FMA; "f64" = the operand widened exactly and the operation done in double,
 * one rounding:
 *   1. x_m = W_m - c
 *   2. s = ((+0.0 + x_0) + x_1) + ... in source order; its sign is taken by comparison (s > 0, s < 0): -0.0 and NaN count as zero
 *      (step 3 of the TIES rule)
 *   3. agree_m = (s > 0 and x_m > 0) or (s < 0 and x_m < 0)
 *      e = max over the agreeing m of |x_m|, from +0.0 (exact: the order does not matter)
 *      u = s > 0 ? e : (s < 0 ? -e : +0.0)             (the unified task vector; where s != 0 a source agrees, so u != 0 there)
 *   4. dst = c + lam * u
 *   5. if the job has masks: bit i of mask m is agree_m at element i, in the packed layout of the consensus merge above, without
 *      change: ceil(n_elem / 32) little-endian 32-bit words, element i is bit i & 31 of word i >> 5, the bits at positions >=
 *      n_elem are 0, every word is written exactly once by every run.
 *   6. per job and source, in f64:  a[m] = sum f64(|x_m|);  b[m] = sum (agree_m ? f64(e) : +0.0).  The order of summation is the
 *      family's (thread, wave by halves, ((w0 + w1) + w2) + w3, the records of a job in chunk order, every sum from +0.0): a thread
 *      adds its float4s u = 0 .. 3 in order and in each the components in order.  THE RAGGED TAIL DIFFERS FROM THE PAIR
 *      STATISTICS': the n_elem & 3 tail elements belong to the ONE thread that stands at the partial float4 n4 = n_elem >> 2 --
 *      thread n4 & 255 of the chunk that owns the tail (thread 0, in a fifth slot, when n4 is a positive multiple of 1024) -- and
 *      their addends enter that thread's sums after its float4s, in element order.
 *   7. rescale[m] = b[m] > 0 ? f32(a[m] / b[m]) : +0.0f: f64 division, then one rounding to fp32, on the device.
 * Exact integer counts per job: kept[m] = the bits set in mask m (counted with or without masks), zero = the elements with s
 * neither > 0 nor < 0, conflict = the elements whose x_m hold both a positive and a negative entry.  A chunk's record holds a[4],
 * b[4] and these six counts AS DOUBLES (14 doubles; integers are exact in a double below 2^53, and a job has fewer than 2^34
 * elements), so one record writer and one fold serve sums and counts; the result holds the counts as uint64.
 * A VLM_EMR_RESTORE job rebuilds one expert: n_src = 1, src[0] = uni (a unified tensor), base = c, mask[0] = a packed mask (an
 * INPUT) and the job scalar rescale, finite and >= 0:  t = uni - c;  y = bit_i ? t : +0.0;  dst = c + rescale * y -- three fp32
 * roundings.  Its only count is kept[0], the bits set among the first n_elem; lam is not read.  The mask is read up to word
 * ceil(n_elem / 32) - 1 and no further; bits at positions >= n_elem are ignored.  With uni the lam = 1 output of the rule above
 * this is the paper's W_pre + lambda_t * M_t * tau_uni UP TO THE ROUNDING OF c + u: uni - c is not u bit for bit, and the restore
 * rule is defined on what the checkpoint holds, not on u.
 * Two deliberate departures from the paper's code: (i) rescalers are per tensor (per job), not per model -- layers here have
 * different expert sets, so a per-model sum over tensors has no meaning; (ii) an element with s == 0 contributes nothing (u = 0,
 * no bit set), where the paper's code gives it a negative sign.
 * Both ops are one elementwise pass in which every load of a float4 precedes its store: dst may be EXACTLY base or EXACTLY one of
 * the job's sources; any other overlap of dst's byte range with an input's is VLM_ERR_ARG, and so is a mask that is not 16-byte
 * aligned or whose 4 ceil(n_elem / 32) bytes meet dst, the base, a source or another mask of the same job (overlap ACROSS jobs is
 * the caller's to avoid).  Non-finite inputs are outside the contract.  A run has no atomics and nothing to clear: it leaves the
 * same bytes, words and results whatever the grid, the job's place in a plan or the number of runs.
 */
#define VLM_EMR_MERGE 0
#define VLM_EMR_RESTORE 1

typedef struct {
  void* dst;                            /* f32 [n_elem] */
  const void* base;                     /* f32 [n_elem]: the central tensor c */
  const void* src[VLM_MERGE_MAX_SRC];   /* f32 [n_elem] each; RESTORE: src[0] = the unified tensor */
  void* mask[VLM_MERGE_MAX_SRC];        /* u32 [ceil(n_elem / 32)] each, 16-byte aligned.  MERGE: outputs, all NULL or all n_src
                                           set; RESTORE: mask[0] is the input */
  uint64_t n_elem;
  int32_t n_src;
  int32_t op;                           /* VLM_EMR_MERGE | VLM_EMR_RESTORE */
  float lam;                            /* MERGE, step 4 */
  float rescale;                        /* RESTORE: finite, >= 0 (MERGE: not read) */
} vlm_emr_job_t;

/* The workspace of an EMR plan BEGINS with this header (byte offsets from its start); jobs keep their upload order. */
typedef struct {
  uint64_t n_jobs, n_chunks;
  uint64_t jobs_off;      /* vlm_emr_job_t [n_jobs] */
  uint64_t chunks_off;    /* the 16-KiB chunk table */
  uint64_t first_off;     /* uint64 [n_jobs + 1]: the first chunk of each job, then n_chunks */
  uint64_t records_off;   /* double [n_chunks][14]: one record per chunk, a[4], b[4], kept[4], zero, conflict, overwritten by every run */
  uint64_t results_off;   /* vlm_emr_result_t [n_jobs]: overwritten by every run */
} vlm_emr_header_t;
#define VLM_EMR_SUMS (3 * VLM_MERGE_MAX_SRC + 2)   /* the doubles of a record */

/* per job after a run; slots a job does not have (sources past n_src; for RESTORE everything but kept[0]) are zero */
typedef struct {
  double abs_sum[VLM_MERGE_MAX_SRC];    /* step 6: a[m] */
  double uni_sum[VLM_MERGE_MAX_SRC];    /* step 6: b[m] */
  uint64_t kept[VLM_MERGE_MAX_SRC];
  uint64_t zero;
  uint64_t conflict;
  float rescale[VLM_MERGE_MAX_SRC];     /* step 7 */
} vlm_emr_result_t;

/* Bytes of device workspace an EMR plan for n_jobs jobs over total_elems elements needs (header, jobs, chunk table, first-chunk
 * table, one record per chunk, one result per job).  The masks are the caller's tensors, not part of the workspace.  No reference
 * site. */
size_t vlm_emr_plan_bytes(int n_jobs, uint64_t total_elems);
/* Check the jobs (the checks of vlm_dare_plan_upload on dst, base, the sources and the length: pointers non-NULL and 16-byte
 * aligned, base required, 1 <= n_src <= VLM_MERGE_MAX_SRC and n_elem > 0, dst's byte range meets an input's only where it is that
 * input exactly; a valid op; a RESTORE job has n_src == 1, mask[0] and a finite rescale >= 0; a MERGE job has no mask or one per
 * source; every mask 16-byte aligned and clear of the job's tensors and other masks; else VLM_ERR_ARG; a length or chunk count past
 * 32 bits of float4s is VLM_ERR_UNSUPPORTED), build the chunk table on the host and copy header + jobs + tables into `workspace`
 * (16-byte aligned; VLM_ERR_WORKSPACE if it is too small).  SYNCHRONISES `stream` before it returns (pageable temporary source);
 * it is the last host synchronisation of a plan.  Implements no step of the rule; no reference site. */
int vlm_emr_plan_upload(const vlm_emr_job_t* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Run an uploaded plan: ONE streaming launch over all jobs of both ops (steps 1-6 and the counts, one record per chunk; the rule
 * of a RESTORE job), then the fold of every job's records in chunk order, which ends in step 7 and writes every job's whole
 * vlm_emr_result_t; no host synchronisation.  May be called again on the same workspace and gives the same bytes, mask words and
 * results.  One run at a time per workspace.  No reference site. */
int vlm_emr_run(void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogue (K1/K6/K8/K9/K10): replaces F.linear at
 * modules/vision_transformer.py:335 (qkv + cat(q_bias,0,v_bias)), :360 (proj), :291/:295 (fc1/fc2),
 * LayerScale + residual at :586/:603 (x + drop_path(gamma * branch)), heads.py:14,27,36,49, and the
 * autograd backward of each (dgrad / wgrad).
 *   C[M,N] = epilogue( op(A)[M,K] . op(B)[K,N] ),   fp32 accumulation
 *   ta=0: A is [M][K] (K contiguous)   ta=1: A is [K][M]
 *   tb=0: B is [N][K] (nn.Linear weight layout)   tb=1: B is [K][N]
 *   v   = alpha*acc + bias[n]
 *   act = NONE/GELU : if aux != NULL, aux[m,n] = bf16(v) (pre-activation / pre-LayerScale branch output)
 *         GELU      : v = gelu_erf(v)               (vision_transformer.py:292, exact erf GELU)
 *         GELU_BWD  : v = v * gelu_erf'(aux[m,n])   (aux is an INPUT: the saved pre-activation)
 *         GELU_DERIV: aux[m,n] = bf16(gelu_erf'(v)); v = gelu_erf(v)   (aux REQUIRED: the forward pass saves the derivative --
 *                     one erf / exp evaluation serves both -- so that the backward epilogue is a multiplication)
 *         MUL_AUX   : v = v * aux[m,n]              (aux is an INPUT: the derivative GELU_DERIV saved)
 *   out = residual[m,n] + row_scale[m] * col_scale[n] * v     (each factor optional)
 *   C   = out  (bf16 or f32)  or  C += out (f32, accumulate != 0)
 *   col_sum[n] += sum_m C[m,n] (optional, fp32 atomics, value before the bf16 rounding): the bias gradient of the
 *         layer whose dY this GEMM produces (fc1 bias from the GELU-backward dgrad), saving a pass over dY
 * Requirements: lda, ldb multiples of 8; ldc, ld_aux, ld_res multiples of 4; 16-B aligned bases; K % 64 == 0
 * unless both operands are K-strided (ta=1 and tb=1).  Ragged M and N are handled in hardware.
 */
#define VLM_ACT_NONE 0
#define VLM_ACT_GELU 1
#define VLM_ACT_GELU_BWD 2
#define VLM_ACT_GELU_DERIV 3
#define VLM_ACT_MUL_AUX 4

typedef struct {
  const float* bias;       /* f32 [N] or NULL */
  const float* col_scale;  /* f32 [N] or NULL (LayerScale gamma) */
  const float* row_scale;  /* f32 [M] or NULL (DropPath keep-mask / keep_prob per row) */
  const float* residual;   /* f32 [M, ld_res] or NULL */
  int64_t ld_res;
  void* aux;               /* bf16 [M, ld_aux] or NULL */
  int64_t ld_aux;
  int32_t act;
  float alpha;
  int32_t accumulate;
  int32_t reserved;
  float* col_sum;          /* f32 [N] or NULL: accumulated column sums of the values written to C */
  float* col_sum_ws;       /* optional with col_sum (N % 128 == 0): f32 [M/128][2][N]; complete 128-row tiles store their
                              column sums at [tile][0][:] instead of adding them to col_sum -- the caller folds rows
                              0 .. M/128-1 into col_sum with vlm_colreduce_batch; the ragged last tile still adds directly */
  float* splitk_ws;        /* optional scratch for ta = tb = 1 (wgrad) calls: with it the reduction over K may be cut into
                              slices that store fp32 tiles [slice][M][N] here and are added into C by a second launch on
                              the same stream (no float atomics); NULL or too small: the atomic split-K path.  The caller
                              keeps one scratch per stream that runs such calls */
  uint64_t splitk_ws_bytes;
} vlm_epilogue_t;

int vlm_gemm_bf16(int ta, int tb, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                  int ldc, int c_is_f32, const vlm_epilogue_t* epi, void* stream);
/* vlm_gemm_bf16 with a row vector: row_live is f32 [M] (or NULL: the call above).  A row is DEAD where its entry is 0.0f; only
 * zero is tested, the vector's other values are never used (DropPath's per-row factors, 0 or 1 / keep, serve as they are).
 * A 256-row tile of the 256x256 kernel whose rows inside [0, M) are ALL dead skips its operand loads and its K loop and runs
 * its normal epilogue on accumulators that are +0: it writes epilogue(0) -- bias, gelu(bias), gelu'(bias) into aux, or
 * residual + row_scale * col_scale * bias -- and the column sums of those values; no output row is left unwritten.  Every
 * other tile computes exactly what vlm_gemm_bf16 computes, and so does every tile of a call that the 128x128 kernel serves and
 * of the residual variant that also stores aux (same results, no skip).  row_live needs the 4-byte alignment of a float only.  The caller promises
 * that nothing it uses depends on the dead rows' products: in the forward pass their branch is multiplied by a zero
 * row_scale, in the backward pass the dead rows of A are exact zeros, so the skipped products are zeros too.  No reference
 * site (timm's DropPath, vision_transformer.py:586/:603, computes the dropped branch and multiplies it by 0). */
int vlm_gemm_bf16_live(int ta, int tb, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                       int ldc, int c_is_f32, const vlm_epilogue_t* epi, const float* row_live, void* stream);
/* Grouped form of the ta = tb = 0 call (K9): row ranges of ONE activation matrix go through DIFFERENT weights -- the
 * modality experts of an all_moe block act on the text rows and on the image rows of the segment-major token matrix
 * (modules/vision_transformer.py:607-681: x[:, :max_text_len] through mlp['l'] / attn['l'], the rest through ['v'], then
 * torch.cat) -- in one launch: the groups' 256-row tiles form one grid, so the small expert's tiles fill the large one's
 * rounds instead of under-filling a launch of their own.  A, C, residual, aux and row_scale are the WHOLE matrices
 * (a group's rows are [row0, row0 + rows) of each); bias, col_sum and col_sum_ws come per group (col_sum_ws rows are
 * counted from the group's row0) and must be NULL in `epi`, as must splitk_ws; accumulate is not supported.  Groups are
 * ascending and disjoint; empty groups are allowed.  Shapes the 256x256 kernel does not serve run as one vlm_gemm_bf16
 * call per group on the same stream: same results either way. */
#define VLM_GEMM_MAX_GROUPS 4
typedef struct {
  int32_t row0, rows;
  const void* B;        /* bf16 [N][ldb]: this group's weight (nn.Linear layout) */
  int32_t ldb;
  int32_t reserved;
  const float* bias;    /* f32 [N] or NULL */
  float* col_sum;       /* f32 [N] or NULL */
  float* col_sum_ws;    /* as vlm_epilogue_t.col_sum_ws: f32 [rows/128][2][N] */
} vlm_gemm_group_t;
int vlm_gemm_bf16_grouped(int n_groups, const vlm_gemm_group_t* groups, int N, int K, const void* A, int lda, void* C,
                          int ldc, int c_is_f32, const vlm_epilogue_t* epi, void* stream);
/* Grouped weight gradients (the autograd backward of the grouped call): for every group of TOKEN rows [row0, row0 + rows) of
 * A = dY [tokens][lda] and B = X [tokens][ldb] (both bf16, token-major: ta = tb = 1 of vlm_gemm_bf16),
 *   C_g[M,N] (+)= A[rows_g]^T . B[rows_g]      (f32, ldc; accumulate per group)
 * in one launch of the 256x256 wgrad kernel plus one reduce launch: the K slices of all groups share one round of
 * workgroups, each group's share following its token count (the plan of vlm_gemm_wgrad_batch below, over row ranges).  splitk_ws as in vlm_epilogue_t (without it, or for shapes the
 * kernel does not serve: one vlm_gemm_bf16 call per group on the same stream; an empty group leaves C_g unchanged when
 * accumulating and zeroes it otherwise). */
typedef struct {
  int32_t row0, rows;
  float* C;
  int32_t accumulate;
  int32_t reserved;
} vlm_wgrad_group_t;
int vlm_gemm_wgrad_grouped(int n_groups, const vlm_wgrad_group_t* groups, int M, int N, const void* A, int lda,
                           const void* B, int ldb, int ldc, float* splitk_ws, uint64_t splitk_ws_bytes, void* stream);
/* Batched weight gradients: n <= VLM_GEMM_MAX_GROUPS problems that reduce over the SAME T token rows, each with its own
 * operands and its own shape (the fc2, fc1, proj and qkv weight gradients of one transformer block evaluation),
 *   dW_i[M_i,N_i] (+)= dy_i[T,M_i]^T . x_i[T,N_i]      (dy, x bf16 token-major; dW f32, ldc; accumulate per problem)
 * in ONE launch of the 256x256 wgrad kernel plus ONE reduce launch.  The reduction of every problem is cut into the fewest K
 * slices whose (slice, tile) workgroups still fit one round of vlm_device_cus() compute units (at least 16 32-row steps per
 * slice): four base-width problems are 108 tiles x 2 slices, where four vlm_gemm_bf16 calls store 999 tiles of partial sums.
 * Slices are fp32 tiles in splitk_ws (as in vlm_epilogue_t, required here) and are added in slice order: no atomics, results
 * do not depend on scheduling.  Made for a second stream, where a launch that leaves compute units free wastes nothing.
 * Returns 0 after the two launches, a negative VLM_ERR_* for bad arguments, and 1 -- "not offered", NOTHING launched, the
 * caller makes one vlm_gemm_bf16(ta = tb = 1) call per problem -- unless for every problem N % 256 == 0, ldc % 4 == 0, dy, x
 * and dW are 16-byte aligned, ld_dy and ld_x are multiples of 8, M N 4 < 2^31 and T ld 2 < 2^31, and all tiles together are
 * at most vlm_device_cus() and all slices fit splitk_ws_bytes. */
typedef struct {
  const void* dy;       /* bf16 [T][ld_dy], columns 0 .. M-1 */
  int32_t ld_dy, M;
  const void* x;        /* bf16 [T][ld_x], columns 0 .. N-1 */
  int32_t ld_x, N;
  float* dW;            /* f32 [M][ldc] */
  int32_t ldc, accumulate;
} vlm_wgrad_problem_t;
int vlm_gemm_wgrad_batch(int n, const vlm_wgrad_problem_t* problems, int T, float* splitk_ws, uint64_t splitk_ws_bytes,
                         void* stream);
/* Which kernel serves ta = tb = 0 calls: 0 the 128x128 tile always, 1 by shape (default), 2 the 256x256 tile whenever the
 * call is legal for it, -1 back to the default; mode 0 also keeps wgrad (ta = tb = 1) off the 256x256 kernel.  Tests and
 * benchmarks only. */
int vlm_gemm_set_big_tile_mode(int mode);

/* ------------------------------------------------------------------------------------------------
 * Row-wise kernels (K5 + LayerScale backward + bias gradients).  D % 4 == 0, D <= 1024.
 * LayerNorm: nn.LayerNorm(eps=1e-6) modules/vision_transformer.py:831, Block.apply_ln :495-523 (a
 * modality-specific LayerNorm is one call per contiguous row range in the segment-major layout);
 * eps=1e-12 for BertEmbeddings / the MLM transform (modules/vilt_module.py:63, heads.py:43).
 *   fwd: y = (x-mean)*rstd*gamma+beta (bf16 or f32), stats[m] = {mean, rstd} (may be NULL)
 *   bwd: dx = dLN/dx (+ dres if given: the residual-path gradient, fused add); dgamma/dbeta are
 *        ACCUMULATED (atomicAdd) so grads of a weight shared by several passes add up in place.
 */
int vlm_layernorm_fwd(const float* x, int ldx, int M, int D, const float* gamma, const float* beta, float eps,
                      void* y, int ldy, int y_is_f32, float* stats, void* stream);
/* workspace (optional, f32, >= VLM_ROW_WS_BYTES(D)): per-workgroup partial column sums folded by a second tiny
 * launch (the kernel of vlm_colreduce_batch); without it the column sums fall back to (heavily contended) float atomics.
 * deferred_blocks (optional, host int*): when non-NULL the fold is NOT launched; the call stores the number of partial
 * rows it wrote to `workspace` and the caller folds several such workspaces later with ONE vlm_colreduce_batch
 * (a transformer block's backward has four row kernels: three launches saved per block evaluation). */
#define VLM_ROW_WS_BYTES(D) ((size_t)1536 * 2 * (size_t)(D) * sizeof(float))
int vlm_layernorm_bwd(const void* dy, int lddy, int dy_is_f32, const float* x, int ldx, const float* stats,
                      const float* gamma, int M, int D, const float* dres, int lddres, float* dx, int lddx,
                      float* dgamma, float* dbeta, float* workspace, size_t workspace_bytes, int* deferred_blocks,
                      void* stream);
/* vlm_layernorm_bwd followed by vlm_layerscale_bwd on the row it has just produced, in one pass: `dx` (the residual-stream
 * gradient in front of this LayerNorm) is also the gradient arriving at the LayerScale of the branch below it
 * (vision_transformer.py:586,:603), so that branch's dy / dgamma / dbias are taken while the row is in registers -- the same
 * operations in the same order as the two calls, bit for bit.  workspace / workspace_bytes in `scale`: its own partial
 * region (a second fold job when deferred: [deferred_blocks][2][D], dgamma then dbias). */
typedef struct {
  const void* y;          /* bf16 [M, D]: the branch's saved output (incl. its bias); NULL = the LayerScale is folded into the
                             branch's projection (vlm_layerscale_fold): gamma and dgamma must be NULL too, dy = bf16(row_scale dx) */
  int32_t ldy;
  const float* gamma;     /* LayerScale vector [D] or NULL (ones) */
  const float* row_scale; /* DropPath row factors [M] or NULL */
  void* dy;               /* bf16 [M, D] out */
  int32_t lddy;
  float* dgamma;          /* += sum_m row_scale*dx*y, or NULL */
  float* dbias;           /* += sum_m dy, or NULL */
  float* workspace;
  size_t workspace_bytes;
} vlm_layerscale_t;
int vlm_layernorm_bwd_scale(const void* dy, int lddy, int dy_is_f32, const float* x, int ldx, const float* stats,
                            const float* gamma, int M, int D, const float* dres, int lddres, float* dx, int lddx,
                            float* dgamma, float* dbeta, float* workspace, size_t workspace_bytes,
                            const vlm_layerscale_t* scale, int* deferred_blocks, void* stream);
#define VLM_MAX_FOLD_JOBS 16
typedef struct {
  const float* partials; /* workspace written by a deferred row kernel: [nblocks][2][D] */
  int32_t nblocks;
  int32_t D;
  float* out0;           /* += sum_b partials[b][0][:]  (dgamma) or NULL */
  float* out1;           /* += sum_b partials[b][1][:]  (dbeta / dbias) or NULL */
} vlm_fold_job_t;
int vlm_colreduce_batch(const vlm_fold_job_t* jobs_host, int n_jobs, void* stream);
/* Backward of x_new = x + row_scale[m]*gamma[n]*y[m,n] (vision_transformer.py:586,:603) w.r.t. the branch:
 *   dy = bf16(row_scale*gamma*dx); dgamma[n] += sum_m row_scale*dx*y; dbias[n] += sum_m dy.
 * y_bf16 NULL (dgamma NULL): only dy and its column sums -- the folded form of vlm_layerscale_fold (gamma normally NULL). */
int vlm_layerscale_bwd(const float* dx, int lddx, const void* y_bf16, int ldy, const float* gamma,
                       const float* row_scale, int M, int D, void* dy_bf16, int lddy, float* dgamma, float* dbias,
                       float* workspace, size_t workspace_bytes, int* deferred_blocks, void* stream);
/* LayerScale folded into the branch's output projection (vision_transformer.py:489-491, :586, :603:
 * x = x + drop_path(gamma * branch(x)), the branch ending in attn.proj / mlp.fc2).  gamma (.) (a W^T + b) = a W'^T + b' with
 * W' = diag(gamma) W and b' = gamma (.) b, so the forward / dgrad / wgrad GEMMs run on folded operands and the saved copy of
 * the branch output (and the O(M N) pass over it) goes.  One job = one weight:
 *   vlm_layerscale_fold:    shadow[n,k] = bf16(gamma[n] weight[n,k]);  bias_out[n] = gamma[n] bias[n]      (after every update)
 *   vlm_layerscale_finish:  with the RAW sums raw_w = g^T a (= dL/dW') and raw_b = colsum(g) (= dL/db'), g = bf16(row_scale dx):
 *                           dweight[n,:] += gamma[n] raw_w[n,:];  dbias[n] += gamma[n] raw_b[n];
 *                           dgamma[n] += sum_k weight[n,k] raw_w[n,k] + bias[n] raw_b[n]   (atomic: experts share gamma);
 *                           raw_w, raw_b are ZEROED (the call composes with gradient accumulation).
 * gamma NULL = ones; bias / bias_out / raw_b / dbias / dgamma may be NULL; weight, raw_w, dweight 16-byte aligned, K % 4 == 0. */
#define VLM_MAX_LAYERSCALE_JOBS 32
typedef struct {
  const float* weight;  /* fp32 master [N, K] */
  const float* gamma;   /* [N] */
  const float* bias;    /* [N] or NULL */
  void* shadow;         /* fold: bf16 [N, K] out */
  float* bias_out;      /* fold: [N] out or NULL */
  float* raw_w;         /* finish: [N, K] in, zeroed */
  float* raw_b;         /* finish: [N] in, zeroed, or NULL */
  float* dweight;       /* finish: [N, K] accumulate */
  float* dbias;         /* finish: [N] accumulate or NULL */
  float* dgamma;        /* finish: [N] accumulate (atomic) or NULL */
  int32_t N, K;
} vlm_layerscale_job_t;
int vlm_layerscale_fold(const vlm_layerscale_job_t* jobs_host, int n_jobs, void* stream);
int vlm_layerscale_finish(const vlm_layerscale_job_t* jobs_host, int n_jobs, void* stream);
/* out[n] += sum_m a[m,n] (bf16 a; N % 8 == 0): bias gradients of qkv / fc1 / heads. */
int vlm_colsum_bf16(const void* a, int lda, int M, int N, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-entropy of the MLM head (modules/objectives.py:88-143: F.cross_entropy(mlm_logits.view(-1, vocab), mlm_labels.view(-1),
 * ignore_index=-100)) on the bf16 logits [rows, ld] the decoder GEMM wrote (V valid columns, ld % 8 == 0), fp32 arithmetic:
 *   fwd: lse[r] = logsumexp(logits[r, :V]);  loss_rows[r] = lse[r] - logits[r, labels[r]], or 0 where labels[r] == ignore_index
 *        (the caller forms the mean over the rows that count);
 *   bwd: dlogits[r, c] = scale_dev[0] * (exp(logits[r, c] - lse[r]) - [c == labels[r]]) as bf16 for c < V, 0 for V <= c < ld_d
 *        and in ignored rows: written whole, padding included, so the buffer is the decoder dgrad / wgrad GEMMs' operand as it
 *        stands.  scale_dev: device scalar (upstream gradient / number of counted rows), no host round trip. */
int vlm_cross_entropy_fwd(const void* logits_bf16, int ld, int rows, int V, const int64_t* labels, int64_t ignore_index,
                          float* loss_rows, float* lse, void* stream);
int vlm_cross_entropy_bwd(const void* logits_bf16, int ld, int rows, int V, const int64_t* labels, int64_t ignore_index,
                          const float* lse, const float* scale_dev, void* dlogits_bf16, int ld_d, void* stream);

/* Round 6: the rest of the loss tail (the [B, *] algebra of modules/objectives.py that was ~120 torch-native launches per step).
 *   vlm_l2norm_fwd / _bwd: y = x / ||x||_2 per row in fp32 (the contrastive heads' feature normalisation, objectives.py:248-300,
 *        vilt_module.py:1329-1375 `/ norm(dim=-1, keepdim=True)`); backward dx = (g - y (g . y)) / ||x|| in x's dtype.
 *   vlm_contrastive: the symmetric cross-entropy of compute_ifm / compute_irtr (objectives.py:274-300, :393-445) on gathered,
 *        normalised features [n, D] (this rank's B rows first, as the reference re-inserts them, :277-286), s = exp(log_scale[0]):
 *        logits [n, n] = s img txt^T; out3 = (loss, d loss / d log_scale, s); d_img / d_txt [B, D] = gradients of the OWN rows.
 *        ws: vlm_contrastive_ws_floats(n) floats.
 *   vlm_small_cross_entropy: F.cross_entropy(logits [rows, V], labels) (mean) and dlogits [rows, V] fp32 = its gradient
 *        (compute_itm_hardneg, objectives.py:239-245: [3B, 2] logits).
 *   vlm_cross_entropy_reduce: out2 = (sum of the counted rows' losses / count, 1 / count) after vlm_cross_entropy_fwd.
 *   vlm_scale_by_scalar: out_k = in_k * scalar_dev[0] for up to 4 buffers in one launch (a scalar loss's upstream gradient). */
int vlm_l2norm_fwd(const void* x, int x_is_bf16, int ld, int rows, int D, float* y, float* inv_norm, void* stream);
int vlm_l2norm_bwd(const float* g, const float* y, const float* inv_norm, int rows, int D, void* dx, int dx_is_bf16, int ld, void* stream);
size_t vlm_contrastive_ws_floats(int n);
int vlm_contrastive(const float* all_img, const float* all_txt, int n, int B, int D, const float* log_scale, float* logits, float* out3,
                    float* d_img, float* d_txt, float* ws, void* stream);
int vlm_small_cross_entropy(const void* logits, int is_bf16, int ld, int rows, int V, const int64_t* labels, float* loss, float* dlogits,
                            void* stream);
int vlm_cross_entropy_reduce(const float* loss_rows, const int64_t* labels, int rows, int V, int64_t ignore_index, float* out2, void* stream);
int vlm_scale_by_scalar(const float* const* in, float* const* out, const int* n, int count, const float* scalar_dev, void* stream);

/* Round 6: the two ends of a pass as single launches (csrc/frontops.hip).
 *   vlm_text_rows_fwd: BertEmbeddings.forward + the modality type row (reference vilt_module.py:51-63, :1111-1113):
 *        out[r] = dropout(LayerNorm(word[ids[r]] + add0; gamma, beta, eps)) + add1, fp32 rows (leading dimension ld_out: the rows of
 *        the pass's token matrix), stats[r] = (mean, rstd).  u: optional fp32 [n, D]; an element is kept where u >= p and scaled by
 *        `scale` (nn.Dropout(p): scale = 1 / (1 - p)).  D % 4 == 0, D <= 1024.
 *   vlm_text_rows_bwd: g = gradient of those rows; adds into d_word[ids[r]] (rows with ids == padding_idx excepted: nn.Embedding's
 *        padding_idx), d_add1, d_beta, d_gamma, d_add0 (each may be null).  ws: vlm_text_rows_bwd_ws_floats(D) floats.
 *   vlm_image_rows_prep: out2[0] = conv_bias + type_row (the patch-embed GEMM's bias), out2[1] = cls + type_row (the lead row) --
 *        visual_embed's cls concat + token_type_embeddings add, vision_transformer.py:952-991, vilt_module.py:1114-1117.
 *   vlm_image_lead_rows: x[b * rows] = lead for b < B.
 *   vlm_image_rows_bwd: g fp32 [B * rows, D] -> g16 bf16 (lead rows zero: the wgrad GEMM's operand); d_bias += column sums over the
 *        patch rows, d_type_row += over all rows, d_cls += over the lead rows.  ws: vlm_image_rows_bwd_ws_floats(D) floats.
 *   vlm_tanh_fwd: y fp32 = tanh(x bf16) (Pooler, heads.py:8-19).
 *   vlm_act_bwd: dy bf16 [M, Np] (columns >= N zero) = g * act'(.): mode 0 exact GELU from the saved bf16 pre-activation (MLM
 *        transform, heads.py:36-46), mode 1 tanh from the saved fp32 output, mode 2 no activation (cast + padding; saved unused).
 *   vlm_colsum_small: out[c] += sum_r a[r][c], N <= 64 columns (ITMHead.fc bias gradient: N = 2).
 *   vlm_sample_negatives: idx[0][i] ~ softmax(sim_a[i, :]) without entry i, idx[1][i] likewise from sim_b (objectives.py:176-229:
 *        F.softmax, fill_diagonal_(0), torch.multinomial(., 1)), inverse CDF on the uniforms u[2][B]; strides in elements (logits_per_text
 *        is the transposed view of logits_per_image).
 *   vlm_weighted_sum: out[0] = sum_k weights[k] * terms[k][0] (device scalars, count <= 8): the loss sum of training_step. */
int vlm_text_rows_fwd(const int64_t* ids, int n, const float* word, int ld_word, const float* add0, const float* gamma, const float* beta,
                      float eps, const float* u, float p, float scale, const float* add1, float* out, int ld_out, float* stats, int D,
                      void* stream);
size_t vlm_text_rows_bwd_ws_floats(int D);
int vlm_text_rows_bwd(const float* g, int ld_g, const int64_t* ids, int n, const float* word, int ld_word, const float* add0,
                      const float* gamma, const float* stats, const float* u, float p, float scale, int D, float* d_word,
                      int64_t padding_idx, float* d_add1, float* d_beta, float* d_gamma, float* d_add0, float* ws, void* stream);
int vlm_image_rows_prep(const float* conv_bias, const float* type_row, const float* cls, int D, float* out2, void* stream);
int vlm_image_lead_rows(float* x, int ld_x, int B, int rows, int D, const float* lead, void* stream);
size_t vlm_image_rows_bwd_ws_floats(int D);
int vlm_image_rows_bwd(const float* g, int ld_g, int B, int rows, int D, void* g16, float* d_bias, float* d_type_row, float* d_cls, float* ws,
                       void* stream);
int vlm_tanh_fwd(const void* x_bf16, int ld_x, int M, int N, float* y, void* stream);
int vlm_act_bwd(const void* g, int g_is_f32, int ld_g, const void* saved, int ld_saved, int mode, int M, int N, int Np, void* dy_bf16,
                void* stream);
int vlm_colsum_small(const void* a_bf16, int lda, int M, int N, float* out, void* stream);
int vlm_sample_negatives(const float* sim_a, int a_row_stride, int a_col_stride, const float* sim_b, int b_row_stride, int b_col_stride, int B,
                         int n, const float* u, int64_t* idx, void* stream);
int vlm_weighted_sum(const float* const* terms, const float* weights, int count, float* out, void* stream);

/* vlm_scatter_rows: dx [R, D] (bf16 or fp32) = sum over the sources of g_k [count_k, D] placed at rows first_row + j * row_step, zero
 *        elsewhere -- the gradient of the row views a pass's result exposes (text_feats = x[:B T], the cls rows x[b T], a leading block
 *        of samples: vilt_module.py:1136-1156, objectives.py:97 `infer["text_feats"]`, heads.py:17 `hidden_states[:, 0]`) in one pass
 *        instead of autograd's zero fill + strided copy per view and an addition per extra view.  D % 4 == 0, at most 4 sources. */
typedef struct {
  const void* g; /* [count, D] rows, bf16 or fp32 */
  int g_is_f32;
  int ld;        /* row stride of g in elements */
  int first_row, row_step, count;
} vlm_scatter_src_t;
int vlm_scatter_rows(void* dx, int dx_is_f32, int ld_dx, int R, int D, const vlm_scatter_src_t* src, int n_src, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flat-buffer elementwise kernels.
 * vlm_adamw_step: transformers-4.x AdamW as instantiated at modules/vilt_utils.py:314-317
 *   (betas=(0.9, beta_2), eps=1e-8, bias-corrected step_size computed by the caller, decoupled decay applied
 *   AFTER the Adam update); also writes the bf16 shadow of the parameters (GEMM operand) and may zero the grad.
 * vlm_patch_im2col: front end of PatchEmbed (vision_transformer.py:714-728): NCHW fp32 image -> bf16 patch rows
 *   [B*(lead_rows + patches), 3*P*P] (column = c*P*P + i*P + j); lead_rows zero rows per image hold the place of
 *   the cls token (:974-975).
 */
int vlm_adamw_step(float* p, float* g, float* m, float* v, void* p_bf16, uint64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float step_size, float grad_scale, int zero_grad,
                   void* stream);
int vlm_cast_f32_bf16(const float* src, void* dst_bf16, uint64_t n, void* stream);
/* Backward of the word-embedding gather (HF BertEmbeddings.word_embeddings = nn.Embedding(vocab, D, padding_idx),
 * vilt_module.py:63, :1090; what torch's embedding_dense_backward + grad accumulation compute):
 * dW[ids[t], 0..D) += gy[t, 0..D) for every t in [0, n) with ids[t] != padding_idx (pass -1 for none).  ids are int64; a token
 * whose id lies outside [0, vocab) is skipped (nothing is written out of bounds); dW is ACCUMULATED (float atomics: the sum order of tokens sharing an id is not fixed). */
int vlm_embedding_bwd(const float* gy, int ld, const int64_t* ids, int64_t n, int D, int64_t padding_idx, float* dW, int ld_w,
                      int64_t vocab, void* stream);
/* Transposed bf16 weight shadows.  The backward of F.linear (dX = dY . W, modules/vision_transformer.py:291/:295/:335/
 * :360 through autograd) reads W [N_out, K_in] along its strided axis; with W^T [K_in, N_out] kept next to W the dgrad
 * is an ordinary K-contiguous GEMM (both operands by LDS-DMA).  One launch refreshes every listed matrix: the device
 * table holds one entry per 64x64 tile (src [rows, cols] row-major -> dst [cols, rows] row-major). */
typedef struct {
  uint64_t src;      /* bf16 device pointer */
  uint64_t dst;      /* bf16 device pointer */
  int32_t rows, cols;
  int32_t tile_row, tile_col;
} vlm_transpose_tile_t;
int vlm_transpose_bf16_tiles(const vlm_transpose_tile_t* tiles_dev, int n_tiles, void* stream);

/* DropPath (timm drop_path, modules/vision_transformer.py:446 used at :586/:603): out[row] = u[b] < keep ? 1/keep : 0
 * for every token row of sample b in the segment-major layout (text rows base0 + b*n0 + t, image rows
 * base1 + b*n1 + i); u = one uniform [0,1) draw per sample.  The result is the GEMM epilogue's row_scale. */
int vlm_droppath_rows(const float* u, float keep, int B, int n0, int n1, int base0, int base1, float* out, void* stream);
/* Every DropPath site of a pass at once: out[s][row] = u0[s][b] < keep[s] ? 1/keep[s] : 0 (image rows take u1[s][b] when u1
 * is given: two unimodal passes sharing one launch keep their own draws).  out is [n_sites, rows]. */
int vlm_droppath_sites(const float* u0, const float* u1, const float* keep, int n_sites, int B, int n0, int n1, int base0,
                       int base1, int rows, float* out, void* stream);
int vlm_patch_im2col(const float* image, void* patches_bf16, int B, int H, int W, int P, int lead_rows, void* stream);
/* ------------------------------------------------------------------------------------------------
 * float64 kernels of the merge side (csrc/f64ops.hip), all products on v_mfma_f64_16x16x4_f64.
 * Gram cache (K15, src/cache_gram_matrices.py:246-254: `G += X.to(float64)^T X` for the input X of every hooked
 * linear): vlm_gram_f64 adds X^T X of a bf16 or fp32 [M, D] activation matrix into the fp64 [D, D] accumulator on the
 * device (exact conversion, fp64 FMA chains, upper-triangular tiles mirrored on the way out).
 * RegMean (K14, src/vilt/modules/vilt_module.py:388-392, 407-434): vlm_scale_gram_f64 forms a*G + (1-a)*diag(G)
 * (optionally accumulating the sum over modalities); vlm_gemm_f64 is C = alpha*op(A) op(B) + beta*C in fp64 (A may be the
 * fp32 checkpoint weight); the reference's torch.inverse of the SPD sum is replaced by a blocked Cholesky
 * factorisation + two triangular solves, each ONE call that walks the 64-wide block columns inside the library:
 * vlm_cholesky_f64 (in-place lower factor of a contiguous SPD [n, n] matrix, the upper triangle is left undefined; *status,
 * zero on entry, gets 1 + the index of the first non-positive pivot, checked by the caller whenever it chooses to
 * synchronise) and vlm_solve_spd_right_f64 (rhs [rows, ld] <- rhs (L L^T)^-1 in place: Y L^T = rhs forward over the block
 * columns, then X L = Y backward).  vlm_accumulate_f32_f64 (dst += src) is kept for callers that already hold an fp32
 * product. */
int vlm_accumulate_f32_f64(const float* src, double* dst_f64, uint64_t n, void* stream);
int vlm_gram_f64(const void* x, int ldx, int M, int D, int x_is_f32, double* gram, void* stream);
int vlm_gemm_f64(int ta, int tb, int M, int N, int K, double alpha, const void* A, int lda, int a_is_f32, const double* B,
                 int ldb, double beta, double* C, int ldc, void* stream);
int vlm_scale_gram_f64(const double* src, double* dst, int n, double alpha, int accumulate, void* stream);
int vlm_cholesky_f64(double* A, int n, int* status, void* stream);
int vlm_solve_spd_right_f64(const double* chol, int n, double* rhs, int ld, int rows, void* stream);
/* The same product / factorisation / solve for `count` (<= 64) matrices of ONE shape in lock step: every block step is ONE launch
 * over all of them (RegMean's 36 solves of 768^2 and 12 of 3072^2, vilt_module.py:432-434: ~420 launches instead of ~5 000).  A_list /
 * chol_list / rhs_list: HOST arrays of device pointers; status: device int[count], zero on entry, verdict per matrix as in
 * vlm_cholesky_f64.  The three single-matrix calls above ARE these at count = 1: per matrix the same bits. */
int vlm_gemm_f64_batched(int ta, int tb, int M, int N, int K, double alpha, const void* const* A_list, int lda, int a_is_f32,
                         const double* const* B_list, int ldb, double beta, double* const* C_list, int ldc, int count, void* stream);
int vlm_cholesky_f64_batched(double* const* A_list, int count, int n, int* status, void* stream);
int vlm_solve_spd_right_f64_batched(double* const* chol_list, int n, double* const* rhs_list, int ld, int rows, int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Iso-C: isotropic merging (Marczak et al. 2025, "No Task Left Behind: Isotropic Model Merging with Common and Task-Specific
 * Subspaces") of a weight MATRIX, csrc/isoc.hip + csrc/f64ops.hip.  No reference site.  The rule, per destination matrix [m, n]
 * with central tensor c, sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), lam and r = min(m, n); fp32 values are widened
 * exactly, every operation is one correctly rounded fp64 operation, no FMA outside the matrix products:
 *   1. D = ((0 + (W_0 - c)) + (W_1 - c)) + ...          (the SUM of the task vectors, not their mean)
 *   2. with D = U diag(sigma) V^T the thin SVD:  Q = U V^T over the non-zero sigma (the polar factor of D);  nuclear = sum sigma
 *   3. dst = fl32(c + s * Q) with s = (lam * nuclear) / r, product, quotient, product and sum in this order, ONE rounding to fp32
 *   4. ||D||_F = 0:  dst = c bit for bit
 * Q comes from a Cholesky-based QDWH iteration instead of an SVD.  The matrix is worked on as [rows >= cols] (D^T when m < n):
 *   alpha = ||D||_F;  X_0 = D / alpha;  per step with host-made coefficients (a, b, c):
 *     Z = I + c X^T X  (vlm_iso_gram);  L = chol(Z)  (vlm_cholesky_f64_batched);  Y = X (L L^T)^-1  (vlm_solve_spd_right_f64_batched);
 *     X <- (b / c) X + (a - b / c) Y  (vlm_iso_step, which also records ||X_new - X||_F^2)
 *   then Q = X and nuclear = <X, D>  (vlm_iso_finish).
 * X_0 is never formed: the first vlm_iso_gram reads D and folds 1 / alpha^2 in from the device, the first vlm_iso_step divides by
 * alpha.  Nothing here synchronises; the caller reads the heads whenever it chooses.
 *
 * The working set of one matrix is ONE device allocation of VLM_ISO_HEAD + 3 * m * n doubles: the head, then D, X and Y, each
 * [rows][cols] row-major.  head[0] = ||D||_F^2, head[1] = <X, D>, head[2 + k] = ||X_{k+1} - X_k||_F^2 of step k < VLM_ISO_MAX_STEPS.
 * Every call takes `count` (<= 64) matrices of ONE shape in lock step; the lists are HOST arrays of device pointers.  `partials`:
 * device scratch of count * vlm_iso_parts(m, n) doubles; the sums are made in a fixed order (the same bits every run).  c, the
 * sources and dst are contiguous and 16-byte aligned; dst may be c or a source.
 *   vlm_iso_delta   D (and Y = D) and head[0] from c_list[count] and src_list[S][count]
 *   vlm_iso_gram    Z_list[b] [cols][cols] = I + f X^T X, upper-triangular tiles computed, mirrored on the way out; first: the
 *                   operand is D and f = c / head[0] (0 where head[0] is not positive), else the operand is X and f = c
 *   vlm_iso_step    X <- p X + q Y, Y <- X, head[2 + k]; first: X is D / alpha and Y is divided by alpha as well
 *   vlm_iso_finish  two phases, either or both (`phases`, a bit mask): VLM_ISO_PHASE_NUCLEAR head[1] = <X, D>; VLM_ISO_PHASE_APPLY
 *                   dst_list[b] by step 3 and 4 from head[1] as it stands.  The apply phase READS c: where dst is c, a second apply
 *                   would add the step twice -- a caller that may iterate further applies once, after its verdict (isoc.py does) */
#define VLM_ISO_HEAD 64
#define VLM_ISO_MAX_STEPS 40
#define VLM_ISO_PHASE_NUCLEAR 1
#define VLM_ISO_PHASE_APPLY 2
int vlm_iso_parts(int m, int n);
int vlm_iso_delta(const float* const* c_list, const float* const* src_list, int S, int m, int n, double* const* work_list,
                  double* partials, int count, void* stream);
int vlm_iso_gram(double* const* work_list, int rows, int cols, int first, double c, double* const* Z_list, int count, void* stream);
int vlm_iso_step(double* const* work_list, int rows, int cols, int first, double p, double q, int k, double* partials, int count,
                 void* stream);
int vlm_iso_finish(double* const* work_list, const float* const* c_list, float* const* dst_list, int m, int n, double lam,
                   double* partials, int count, int phases, void* stream);

/* ------------------------------------------------------------------------------------------------
 * WUDI-Merging (Cheng et al., ICML 2025, "Whoever Started the Interference Should End It: Guiding Data-Free Model Merging via
 * Task Vectors") of a weight MATRIX, csrc/wudi.hip + the products of csrc/f64ops.hip.  No reference site.  Per linear layer the
 * method minimises  L(X) = sum_i (1 / ||tau_i||_F^2) ||(X - tau_i) tau_i^T||_F^2  over the merged task vector X by Adam, starting
 * from the sum of the task vectors.  The rule, per destination matrix [m, n] (m = out, n = in, as stored) with central tensor c,
 * sources W_0 .. W_{S-1} (1 <= S <= VLM_MERGE_MAX_SRC), lam, iters = T >= 1, lr, beta1, beta2, eps; fp32 values are widened
 * exactly, everything elementwise is one correctly rounded fp64 operation each, no FMA outside the matrix products, whose sums
 * may run in any order:
 *   1. tau_i = W_i - c;  n_i = sum tau_i^2 in a fixed order;  w_i = 1 / n_i, 0 where n_i = 0
 *   2. G = sum_i w_i tau_i^T tau_i [n, n];  B = sum_i tau_i (w_i tau_i^T tau_i) [m, n];  K = sum_i n_i ||w_i tau_i^T tau_i||_F^2
 *      (= sum_i w_i <tau_i (tau_i^T tau_i), tau_i>), the sums over i in source order from 0
 *   3. X_0 = ((0 + tau_0) + tau_1) + ...;  M = V = 0
 *   4. for t = 1 .. T, in the operation order of torch.optim.Adam:
 *        g = 2 (X_{t-1} G - B);  loss_{t-1} = <X_{t-1}, X_{t-1} G - 2 B> + K  (= L(X_{t-1}))
 *        M = beta1 M + (1 - beta1) g;  V = beta2 V + ((1 - beta2) g) g
 *        X_t = X_{t-1} - step_t * (M / (sqrt(V) / bc2s_t + eps))   with step_t = lr / (1 - beta1^t), bc2s_t = sqrt(1 - beta2^t)
 *   5. dst = fl32(c + lam * X_T): product, sum, ONE rounding to fp32
 * The gradient of L is 2 (X G - B): the RegMean normal equation with w_i tau_i^T tau_i in place of a data Gram.  step_t and bc2s_t
 * are functions of t alone: the caller makes them as host doubles, nothing between the first launch and the last synchronises.
 *
 * The working set of one matrix is ONE device allocation of vlm_wudi_work_doubles(m, n) = VLM_WUDI_HEAD + 2 n n + 5 m n doubles:
 * the head, G, a setup scratch [n][n], then B, X (buffer 0), X (buffer 1), M and V, each [m][n] row-major.  A step READS X_{t-1}
 * from buffer (t - 1) & 1 and WRITES X_t to buffer t & 1 (every workgroup of a tile row reads the row's whole panel of X_{t-1}
 * while its neighbours store: in place would be a race); X_T starts at vlm_wudi_state_offset(m, n, T).  head[0 .. 3] = n_i,
 * head[4 .. 7] = ||w_i tau_i^T tau_i||_F^2, head[8] = K, head[9] = loss_0 = L(X_0), head[10] = loss_{T-1} = L(X_{T-1}).
 * Every call takes `count` (<= 64) matrices of ONE shape [m, n] in lock step; the lists are HOST arrays of device pointers.
 * `partials`: device scratch of count * vlm_wudi_parts(m, n) doubles that lives from prepare to finish (it carries the per-tile
 * loss shares of step 1 and of the latest later step), matrix b of a call owning doubles [b, b + 1) * vlm_wudi_parts(m, n) of it:
 * a step may run matrices that several prepare calls set up (different S) in ONE launch when their slices lie side by side, and
 * finish may again be called per slice (different lam).  Every sum is made in a fixed order without atomics (the same bits every
 * run).  c, the sources and dst are contiguous and 16-byte aligned; dst may be c or a source.
 *   vlm_wudi_prepare  steps 1 - 3 from c_list[count] and src_list[S][count] (tau_i passes through V, M and V end zero)
 *   vlm_wudi_step     step 4 for ONE t >= 1: one launch, the product X G on 64 x 64 MFMA-f64 tiles with the update in its epilogue
 *   vlm_wudi_finish   head[8 .. 10] and step 5 after `iters` steps */
#define VLM_WUDI_HEAD 16
int vlm_wudi_parts(int m, int n);
size_t vlm_wudi_work_doubles(int m, int n);
size_t vlm_wudi_state_offset(int m, int n, int iters);
int vlm_wudi_prepare(const float* const* c_list, const float* const* src_list, int S, int m, int n, double* const* work_list,
                     double* partials, int count, void* stream);
int vlm_wudi_step(double* const* work_list, int m, int n, int t, double step, double bc2s, double beta1, double beta2, double eps,
                  double* partials, int count, void* stream);
int vlm_wudi_finish(double* const* work_list, const float* const* c_list, float* const* dst_list, int S, int m, int n, int iters,
                    double lam, double* partials, int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batched float64 SVD by one-sided (Hestenes) Jacobi, csrc/jacobi.hip.  No reference site.  A matrix is worked on as [p <= q]: p rows
 * of length q, row-major (a tall matrix as its transpose: the caller stages it).  The working set of one matrix is ONE device
 * allocation of vlm_svd_work_doubles(p, q) = VLM_SVD_HEAD + p q + p p + 2 p doubles: the head, A [p][q], R [p][p], s [p], then
 * rank [p] and order [p] as int32.  A starts as the matrix and R as I (vlm_svd_reset, which also zeroes the head); both take the same
 * row rotations, so A ends as diag(s) V^T and R as U^T with  matrix = R^T A.
 *   A SWEEP is the round-robin tournament over the p rows (csrc/jacobi_schedule.h; a bye when p is odd): vlm_svd_steps(p) = p - 1
 *   (p even) or p (p odd) steps of floor(p / 2) disjoint pairs.  Every step is ONE launch over `count` (<= 64) matrices of one
 *   working shape, one workgroup per pair and matrix.  Per pair (i, j), every operation one correctly rounded fp64 operation:
 *     alpha = |a_i|^2, beta = |a_j|^2, gamma = a_i . a_j, summed in a fixed lane-then-wave order (the same bits every run);
 *     rotate iff |gamma| > sqrt(q) 2^-53 sqrt(alpha beta):
 *       zeta = (beta - alpha) / (2 gamma);  t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))  (sign(0) = 1);  c = 1 / sqrt(1 + t^2);  s = c t;
 *       a_i <- c a_i - s a_j,  a_j <- s a_i + c a_j,  and the same for rows i, j of R.
 *   head[2 + k] = the rotations of sweep k, head[32 + k] = the largest |gamma| / sqrt(alpha beta) sweep k met (k < VLM_SVD_MAX_SWEEPS):
 *   a count and a maximum, one vector atomic each per workgroup, independent of the order.  A matrix whose sweep k - 1 rotated
 *   nothing is finished: sweep k leaves it untouched (its workgroups return at once), so sweeps must be issued in order from 0
 *   on a reset head, and a caller may enqueue more sweeps than a matrix needs and read the heads once.  Nothing here synchronises.
 *   q > 8192 (a row no longer fits a workgroup's registers) is VLM_ERR_UNSUPPORTED.
 *   vlm_svd_reset   R = I, head = 0
 *   vlm_svd_sweep   all steps of sweep `sweep`
 *   vlm_svd_finish  s_j = |a_j| (fixed order);  rank[j] = the rows in front of row j by (s descending, index ascending) and
 *                   order[rank[j]] = j;  head[0] = s_max;  A's rows become the unit rows v_j = a_j / s_j -- a ZERO row where s_j = 0 or
 *                   s_j <= floor_rel * s_max (0 <= floor_rel < 1);  head[1] = the number of rows zeroed.
 *
 * TSV-M (Gargiulo et al., CVPR 2025, "Task Singular Vectors: Reducing Task Interference in Model Merging") of a weight MATRIX,
 * csrc/tsvm.hip + the SVD above + vlm_gemm_f64_batched.  No reference site.  The rule, per destination matrix [m, n] with central
 * tensor c, sources W_0 .. W_{S-1} (2 <= S <= VLM_MERGE_MAX_SRC), lam, r = min(m, n) and k = floor(r / S); fp32 values are widened
 * exactly, everything runs in float64:
 *   1. tau_i = W_i - c = U_i diag(s_i) V_i^T, the thin SVD, singular values in descending order
 *   2. expert i's first k triplets go to columns [i k, (i + 1) k) of Ucat [m, kS], scat [kS] and Vcat [n, kS]; a triplet with s = 0
 *      exactly contributes a ZERO column to Ucat and Vcat (an expert equal to c adds nothing; no arbitrary basis is injected)
 *   3. Uo = polar(Ucat), Vo = polar(Vcat) with polar(B) = sum over sigma_j > 2^-40 sigma_max of p_j q_j^T from B = P diag(sigma) Q^T
 *      (the paper's u v^T of svd(Ucat); directions the experts share exactly are dropped, and counted, not completed arbitrarily)
 *   4. dst = fl32(c + lam * (Uo diag(scat) Vo^T)): product, sum, ONE rounding to fp32
 *   5. k = 0 (r < S): the merged task vector is zero and dst = c bit for bit
 * The rule is symmetric under transposition, so everything runs in the working orientation [p <= q] of tau_i (tau_i^T when m > n).
 * polar(B^T) = polar(B)^T, and from the row-Jacobi of B^T [kS, len] it is R^T times the unit rows with floor_rel = 2^-40.
 *   vlm_tsv_delta   A of work_list[b] = src_list[b] - c_list[b] in working orientation (follow with vlm_svd_reset)
 *   vlm_tsv_gather  after vlm_svd_finish of S x count first SVDs (src_work_list[S][count], working shape [p, q]): row i k + r of the
 *                   destination's A [kS][len] = expert i's row order[r] of R (side 0, len = p) or of the unit rows (side 1, len = q),
 *                   a zero row where that s is exactly 0; side 1 also writes scat_list[b][i k + r] = that s (follow with vlm_svd_reset)
 *   vlm_tsv_apply   step 4 (and 5 at kS = 0): T = PU^T diag(scat) PV on 64 x 64 MFMA-f64 tiles from the TRANSPOSED polar factors
 *                   pu_list[b] [kS][p] and pv_list[b] [kS][q], stored to t_list[b] [p][q]; dst in the tensor's own orientation in the
 *                   epilogue.  c, the sources and dst are contiguous and 16-byte aligned; dst may be c or a source. */
#define VLM_SVD_HEAD 64
#define VLM_SVD_MAX_SWEEPS 30
size_t vlm_svd_work_doubles(int p, int q);
int vlm_svd_steps(int p);
int vlm_svd_reset(double* const* work_list, int p, int q, int count, void* stream);
int vlm_svd_sweep(double* const* work_list, int p, int q, int sweep, int count, void* stream);
int vlm_svd_finish(double* const* work_list, int p, int q, double floor_rel, int count, void* stream);
int vlm_tsv_delta(const float* const* c_list, const float* const* src_list, int m, int n, double* const* work_list, int count,
                  void* stream);
int vlm_tsv_gather(const double* const* src_work_list, int S, int p, int q, int k, int side, double* const* dst_work_list,
                   double* const* scat_list, int count, void* stream);
int vlm_tsv_apply(const double* const* pu_list, const double* const* pv_list, const double* const* scat_list,
                  const float* const* c_list, float* const* dst_list, double* const* t_list, int m, int n, int kS, double lam, int count,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused attention (K4 + K7 + K7b): softmax(scale*Q K^T + bias[h] + key mask) V, head_dim = 64.
 * Replaces Attention.forward's core, modules/vision_transformer.py:346-358, the bias materialisation
 * get_rel_pos_bias modules/vilt_module.py:1061-1064 (never formed here), and the text/image block-diagonal
 * split of separate_plain_forward / moe_forward (vision_transformer.py:567-584, :619-637).
 *   qkv       bf16 [rows, 3*H*64] = F.linear output of :335 as is (q | k | v thirds, head-major); the kernel
 *             applies `scale` (:346) to the scores.
 *   bias_t    f32 [n_cols, R]: TRANSPOSE of relative_position_bias_table [R, heads*layers]; row head_row0+h
 *             is head h of this layer.  NULL = no bias.
 *   rel_index / rel_index_t  int16 [index_rows, ld_index] and its transpose (BOTH are needed: each kernel reads the
 *             orientation whose fast axis runs along its lanes, so every index load is a coalesced 64-B row piece;
 *             the forward reads only rel_index_t): 4 x relative-position index (= byte offset into the fp32 table column,
 *             R <= 8191) in "index coordinates": text token t is position t, image token i is position pos1 + i
 *             (pos1 % 8 == 0, ld_index % 4 == 0).
 *   keep0/1   uint8 [B, n0] / [B, n1] key keep flags (text_masks; NULL = keep all), masked_fill(-inf) of :354.
 *   rows      segment-major: text (b,t) -> base0 + b*n0 + t ; image (b,i) -> base1 + b*n1 + i.
 *   mode      JOINT: every query sees text then image keys.  SEPARATE: queries see their own segment only.
 * Forward writes out bf16 [rows, H*64] (the layout :358 reshapes to) and lse f32 [H, total_rows] (log2 domain,
 * consumed by the backward).  Backward: delta = rowsum(dO*O), then dK/dV (+ the bias-table gradient, accumulated
 * into dbias_t f32 [n_cols, R]) and dQ, written into dqkv bf16 [rows, 3*H*64] (dq already carries `scale`).
 */
#define VLM_ATTN_JOINT 0
#define VLM_ATTN_SEPARATE 1

typedef struct {
  const void* qkv;
  int32_t ld_qkv;
  int32_t H;
  int32_t total_rows;
  int32_t R;
  const float* bias_t;
  const int16_t* rel_index;    /* [q position][key position] */
  const int16_t* rel_index_t;  /* its transpose [key position][q position], same leading-dimension rules */
  int32_t ld_index;
  int32_t index_rows;
  int32_t ld_index_t;
  int32_t index_t_rows;
  int32_t head_row0;
  int32_t mode;
  const uint8_t* keep0;
  const uint8_t* keep1;
  int32_t B, n0, n1, base0, base1, pos1;
  float scale;
  /* Kept query rows (the two ints this struct held in reserve; the second one sits behind dense_tiles): the outputs of the
   * first q_keep0 text and the first q_keep1 image QUERY positions of every sample are wanted, nothing else.  0 in both = all
   * (a limit past its segment is the whole segment; (k, 0) keeps no image query, (0, k) no text query).  Keys are never limited.
   *   vlm_attention_fwd launches only the 128-position query tiles that hold a kept position; a launched tile writes all its
   *     rows, the rows of out and lse in other tiles are NOT written and nobody may read them.
   *   vlm_attention_bwd / _live: the caller promises -- as for row_live -- that the dO rows outside the prefixes count as
   *     zero; they, and the out / lse rows there, are NOT read.  dQ of a kept row is what the unlimited call gives, the dQ third
   *     of every other row is written as zeros (the qkv dgrad and wgrad read every row), dK / dV / the column sums / the
   *     bias-table gradient take the kept queries only, delta is written for kept rows only.
   * The limit is honoured where vlm_attention_qkeep_served() says so: by every forward kernel, every dQ kernel and the fused
   * dK / dV / bias-gradient kernel.  A backward whose plan has the separate dK / dV kernel (no bias-table gradient asked for,
   * or a panel that does not fit) IGNORES the limit: it reads every row of dO, out and lse, so its forward must have run
   * without the limit and the dO rows outside the prefixes must hold zeros. */
  int32_t q_keep0;
  /* Dense bias (vlm_bias_dense), REQUIRED when bias_t is set: fp16 log2(e) * bias_t[c][rel_index[q][k]/4] (the
   * kernels' score accumulators are base-2 exponents) for every (layer, head) column c, stored as 4-KiB tiles in MFMA operand order (one tile
   * per 32 stationary x 64 streamed positions, vlm_bias_dense_bytes() per column); positions that are not valid
   * members of a tile's segment hold a large negative value, so ragged tiles, the text/image gap and -- in SEPARATE
   * mode -- the foreign segment mask themselves.  bias_dense: stationary = query (forward, dQ); bias_dense_t:
   * stationary = key (dK/dV).  The tables depend on (n0, n1, pos1, mode); the kernels add the slice
   * [head_row0 + h] to the score accumulators on the matrix pipe.  The bias is identical for every sample of the
   * batch, so a layer's slices stay cache-resident.  The bias-table GRADIENT still goes through rel_index. */
  const void* bias_dense;
  const void* bias_dense_t;
  int32_t dense_tiles; /* vlm_bias_dense_bytes(n0, n1, pos1, mode) / 4096 */
  int32_t q_keep1;
} vlm_attn_desc_t;

/* 1: a vlm_attention_bwd / _live of this descriptor (with a bias-table gradient when with_dbias != 0) honours q_keep0 / q_keep1;
 * 0: it ignores them (see above), or the descriptor is invalid.  The forward always honours them. */
int vlm_attention_qkeep_served(const vlm_attn_desc_t* d, int with_dbias);

/* Dense relative-position bias for all heads and layers at once (the reference's get_rel_pos_bias,
 * modules/vilt_module.py:1061-1064): out = n_cols columns of vlm_bias_dense_bytes() each.  index: int16 [pos1 + n1,
 * ld_index] relative-position index (4 x index, as in vlm_attn_desc_t.rel_index); k_major selects bias_dense_t. */
size_t vlm_bias_dense_bytes(int n0, int n1, int pos1, int mode);
int vlm_bias_dense(const float* bias_t, int n_cols, int R, const int16_t* index, int ld_index, int n0, int n1, int pos1,
                   int mode, int k_major, void* out_f16, void* stream);

int vlm_attention_fwd(const vlm_attn_desc_t* d, void* out_bf16, int ld_out, float* lse, void* stream);
/* Optional fused bias gradients: dq[s] / dv[s] (f32 [H*64], may be NULL) are ACCUMULATED with the column sums of dQ /
 * dV over the rows of segment s (0 = text rows, 1 = image rows; modality experts own different q_bias / v_bias,
 * vision_transformer.py:335), taken while the tiles are still in registers instead of re-reading dqkv. */
typedef struct {
  float* dq[2];
  float* dv[2];
} vlm_attn_colsum_t;

/* delta_ws: f32 scratch of ws_floats >= vlm_attention_bwd_ws_floats(d, .) elements: H * total_rows (rowsum(dO*O)), or
 * 3 * H * total_rows for a bias table whose gradient cannot come from the fused dK / dV / bias-gradient kernel (more than 1 024
 * positions in a part): the 16-wave bias-table-gradient kernel's C operands (-lse / (scale log2 e), -delta) live behind delta.
 * `with_dbias` no longer changes the answer (kept for the signature); a larger scratch is accepted and changes nothing: which
 * kernels run depends on the descriptor and on dbias_t alone.  dbias_t (f32 [n_cols, R], may be NULL) is ACCUMULATED by float
 * atomics.  colsum may be NULL. */
size_t vlm_attention_bwd_ws_floats(const vlm_attn_desc_t* d, int with_dbias);
int vlm_attention_bwd(const vlm_attn_desc_t* d, const void* out_bf16, int ld_out, const void* dout_bf16, int ld_dout,
                      const float* lse, float* delta_ws, size_t ws_floats, void* dqkv_bf16, int ld_dqkv, float* dbias_t,
                      const vlm_attn_colsum_t* colsum, void* stream);
/* vlm_attention_bwd with a row vector: row_live is f32 [total rows] (or NULL: the call above), DropPath's per-row factors.  A
 * (sample, segment) is DEAD where the factor of its segment's first row is 0.0f -- in JOINT mode the two segments of a sample
 * share one draw and both first rows must be zero, in SEPARATE mode each segment has its own.  The caller promises that the dO
 * rows of a dead (sample, segment) are zeros; its dQ, dK and dV rows and its share of every column sum and of the bias-table
 * gradient are then zeros as well, and the fused dK / dV / bias-gradient kernel and the hand-placed dQ stream store those zeros
 * without recomputing the sample (delta and the bias-gradient kernel's operands are still written for its rows).  The other
 * kernels of the plan compute every sample.  Every other row of dqkv is what vlm_attention_bwd writes.  No reference site. */
int vlm_attention_bwd_live(const vlm_attn_desc_t* d, const void* out_bf16, int ld_out, const void* dout_bf16, int ld_dout,
                           const float* lse, float* delta_ws, size_t ws_floats, void* dqkv_bf16, int ld_dqkv, float* dbias_t,
                           const vlm_attn_colsum_t* colsum, const float* row_live, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLM_HIP_H */
