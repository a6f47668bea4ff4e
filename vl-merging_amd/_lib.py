"""ctypes binding of libvlm_hip.so (the C ABI in include/vlm_hip.h).  Fails loudly when absent."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VLM_LIB_PATH") or os.path.join(_HERE, "lib", "libvlm_hip.so")
_lib = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t
c_u64 = ctypes.c_uint64

MERGE_LERP, MERGE_TASKVEC, MERGE_MEAN = 0, 1, 2
MERGE_MAX_SRC = 4


class MergeJob(ctypes.Structure):
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("ratio", c_float * MERGE_MAX_SRC),
        ("n_src", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("n_elem", c_u64),
    ]


TIES_COUNTERS = MERGE_MAX_SRC + 2  # VLM_TIES_COUNTERS: kept per source, conflict, empty


class TiesJob(ctypes.Structure):
    """vlm_ties_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("k", c_u64 * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("lam", c_float),
    ]


class TiesHeader(ctypes.Structure):
    """vlm_ties_header_t: the first bytes of a TIES plan's workspace (byte offsets of what a run leaves there)."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_units", "n_chunks", "jobs_off", "chunks_off", "unit0_off", "units_off",
                                     "state_off", "counters_off", "hist_off")]


class TiesState(ctypes.Structure):
    """vlm_ties_state_t."""
    _fields_ = [("key", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("rank", c_u64)]


DARE_LINEAR, DARE_TIES = 0, 1
DARE_COUNTERS = MERGE_MAX_SRC + 2  # VLM_DARE_COUNTERS: kept per source, conflict, empty


class DareJob(ctypes.Structure):
    """vlm_dare_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("keep_below", c_u64),
        ("seed", c_u64),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("lam", c_float),
        ("rescale", c_float),
        ("stream", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


BAND_LINEAR, BAND_TIES = 0, 1
BAND_COUNTERS = 2 * MERGE_MAX_SRC + 2  # VLM_BAND_COUNTERS: kept per source, outlier per source, conflict, empty


class BandJob(ctypes.Structure):
    """vlm_band_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("k_hi", c_u64 * MERGE_MAX_SRC),
        ("k_lo", c_u64 * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("lam", c_float),
        ("reserved", ctypes.c_uint32),
    ]


class BandHeader(ctypes.Structure):
    """vlm_band_header_t: the first bytes of a band plan's workspace (vlm_ties_header_t's fields)."""
    _fields_ = list(TiesHeader._fields_)


class BandState(ctypes.Structure):
    """vlm_band_state_t."""
    _fields_ = [("key_lo", ctypes.c_uint32), ("key_hi", ctypes.c_uint32), ("rank_lo", c_u64), ("rank_hi", c_u64)]


class DareHeader(ctypes.Structure):
    """vlm_dare_header_t: the first bytes of a DARE plan's workspace."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_chunks", "jobs_off", "chunks_off", "counters_off")]


TALL_CONSENSUS, TALL_RESTORE = 0, 1
TALL_COUNTERS = MERGE_MAX_SRC + 2  # VLM_TALL_COUNTERS: kept per source, selected, empty


class TallJob(ctypes.Structure):
    """vlm_tall_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("mask", c_void_p * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("op", ctypes.c_int32),
        ("k", ctypes.c_int32),
        ("tall_lambda", c_float),
        ("lam", c_float),
        ("reserved", ctypes.c_uint32),
    ]


class TallHeader(ctypes.Structure):
    """vlm_tall_header_t: the first bytes of a consensus plan's workspace."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_chunks", "jobs_off", "chunks_off", "counters_off")]


DELLA_LINEAR, DELLA_TIES = 0, 1
DELLA_COUNTERS = MERGE_MAX_SRC + 2  # VLM_DELLA_COUNTERS: kept per source, conflict, empty
DELLA_MAX_ROW = 4096                # VLM_DELLA_MAX_ROW: the longest row whose ranks one workgroup makes in LDS
ISO_HEAD = 64                       # VLM_ISO_HEAD: doubles in front of an Iso-C working set (norms, step norms)
ISO_MAX_STEPS = 40                  # VLM_ISO_MAX_STEPS
ISO_PHASE_NUCLEAR, ISO_PHASE_APPLY = 1, 2  # VLM_ISO_PHASE_*: the phases of vlm_iso_finish, a bit mask
WUDI_HEAD = 16                      # VLM_WUDI_HEAD: doubles in front of a WUDI working set (n_i, ||G_i||^2, K, the two losses)
SVD_HEAD = 64                       # VLM_SVD_HEAD: doubles in front of a Jacobi SVD working set
SVD_MAX_SWEEPS = 30                 # VLM_SVD_MAX_SWEEPS: head[2 + k] rotations, head[32 + k] largest off-diagonal ratio of sweep k
SVD_MAX_Q = 8192                    # the longest row a Jacobi workgroup holds in registers


class DellaJob(ctypes.Structure):
    """vlm_della_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("keep_lo", c_u64),
        ("keep_hi", c_u64),
        ("seed", c_u64),
        ("n_elem", c_u64),
        ("row_len", ctypes.c_uint32),
        ("n_src", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("rescale", ctypes.c_int32),
        ("lam", c_float),
        ("stream", ctypes.c_uint32),
    ]


class DellaHeader(ctypes.Structure):
    """vlm_della_header_t: the first bytes of a DELLA plan's workspace."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_tiles", "jobs_off", "tiles_off", "counters_off")]


PAIRSTATS_PAIRS = MERGE_MAX_SRC * (MERGE_MAX_SRC - 1) // 2  # VLM_PAIRSTATS_PAIRS


def pair_slot(a, b):
    """The slot of the pair (a, b), a < b, in a pair-statistics result: it does not depend on the job's source count."""
    if not 0 <= a < b < MERGE_MAX_SRC:
        raise ValueError("a pair is (a, b) with 0 <= a < b < %d, got (%r, %r)" % (MERGE_MAX_SRC, a, b))
    return b * (b - 1) // 2 + a


class PairStatsJob(ctypes.Structure):
    """vlm_pairstats_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("tkey", ctypes.c_uint32 * MERGE_MAX_SRC),
        ("n_src", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PairStatsHeader(ctypes.Structure):
    """vlm_pairstats_header_t: the first bytes of a pair-statistics plan's workspace."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_chunks", "jobs_off", "chunks_off", "first_off", "records_off", "results_off")]


class PairStatsResult(ctypes.Structure):
    """vlm_pairstats_result_t: the raw sums of one job."""
    _fields_ = ([("sq", ctypes.c_double * MERGE_MAX_SRC)]
                + [(n, ctypes.c_double * PAIRSTATS_PAIRS) for n in ("dot", "dist2", "ssd", "tssd")]
                + [("nnz", c_u64 * MERGE_MAX_SRC)]
                + [(n, c_u64 * PAIRSTATS_PAIRS) for n in ("live", "conflict", "tlive", "tconflict")])


STOCK_SUMS = MERGE_MAX_SRC + PAIRSTATS_PAIRS  # VLM_STOCK_SUMS: the doubles of a chunk's record, sq[4] then dot[6]


class StockJob(ctypes.Structure):
    """vlm_stock_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class StockHeader(ctypes.Structure):
    """vlm_stock_header_t: the first bytes of a Model Stock plan's workspace (vlm_pairstats_header_t's fields)."""
    _fields_ = list(PairStatsHeader._fields_)


class StockResult(ctypes.Structure):
    """vlm_stock_result_t: the sums, the cosines, the ratio and the scale of one job."""
    _fields_ = [("sq", ctypes.c_double * MERGE_MAX_SRC), ("dot", ctypes.c_double * PAIRSTATS_PAIRS),
                ("cos_pair", ctypes.c_double * PAIRSTATS_PAIRS), ("cos", ctypes.c_double), ("t", ctypes.c_double),
                ("scale", c_float), ("reserved", ctypes.c_uint32)]


EMR_MERGE, EMR_RESTORE = 0, 1
EMR_SUMS = 3 * MERGE_MAX_SRC + 2  # VLM_EMR_SUMS: the doubles of a chunk's record


class EmrJob(ctypes.Structure):
    """vlm_emr_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("mask", c_void_p * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("op", ctypes.c_int32),
        ("lam", c_float),
        ("rescale", c_float),
    ]


class EmrHeader(ctypes.Structure):
    """vlm_emr_header_t: the first bytes of an EMR plan's workspace (vlm_pairstats_header_t's fields)."""
    _fields_ = list(PairStatsHeader._fields_)


class EmrResult(ctypes.Structure):
    """vlm_emr_result_t: the sums, the counts and the rescalers of one job."""
    _fields_ = [("abs_sum", ctypes.c_double * MERGE_MAX_SRC), ("uni_sum", ctypes.c_double * MERGE_MAX_SRC),
                ("kept", c_u64 * MERGE_MAX_SRC), ("zero", c_u64), ("conflict", c_u64), ("rescale", c_float * MERGE_MAX_SRC)]


SCE_COUNTERS = 3  # VLM_SCE_COUNTERS: kept, conflict, empty


class SceJob(ctypes.Structure):
    """vlm_sce_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("k", c_u64),
        ("n_elem", c_u64),
        ("n_src", ctypes.c_int32),
        ("lam", c_float),
    ]


class SceHeader(ctypes.Structure):
    """vlm_sce_header_t: the first bytes of an SCE plan's workspace (vlm_ties_header_t's fields, then the reducer's two tables)."""
    _fields_ = list(TiesHeader._fields_) + [(n, c_u64) for n in ("first_off", "records_off")]


class SceResult(ctypes.Structure):
    """vlm_sce_result_t: the threshold, the sums, their total and the weights of one job."""
    _fields_ = [("key", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("rank", c_u64), ("sq", ctypes.c_double * MERGE_MAX_SRC),
                ("tot", ctypes.c_double), ("w", c_float * MERGE_MAX_SRC)]


SPHERE_OK, SPHERE_LINEAR, SPHERE_ZERO = 0, 1, 2  # VLM_SPHERE_*: the status of a group's step 3
SPHERE_ITERS = 24                                # VLM_SPHERE_ITERS


class SphereJob(ctypes.Structure):
    """vlm_sphere_job_t of include/vlm_hip.h."""
    _fields_ = [
        ("dst", c_void_p),
        ("base", c_void_p),
        ("src", c_void_p * MERGE_MAX_SRC),
        ("coef_out", c_void_p),
        ("w", ctypes.c_double * MERGE_MAX_SRC),
        ("n_elem", c_u64),
        ("row_len", ctypes.c_uint32),
        ("n_src", ctypes.c_int32),
        ("lam", c_float),
        ("reserved", ctypes.c_uint32),
    ]


class SphereHeader(ctypes.Structure):
    """vlm_sphere_header_t: the first bytes of a spherical plan's workspace."""
    _fields_ = [(n, c_u64) for n in ("n_jobs", "n_chunks", "n_tiles", "jobs_off", "chunks_off", "tiles_off", "first_off",
                                     "records_off", "results_off")]


class SphereResult(ctypes.Structure):
    """vlm_sphere_result_t: the sums, the coefficients and the status of a tensor job; the row counters of a row job."""
    _fields_ = [("sq", ctypes.c_double * MERGE_MAX_SRC), ("dot", ctypes.c_double * PAIRSTATS_PAIRS),
                ("coef64", ctypes.c_double * MERGE_MAX_SRC), ("rho", ctypes.c_double), ("resid", ctypes.c_double),
                ("coef32", c_float * MERGE_MAX_SRC), ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("rows_linear", c_u64), ("rows_zero", c_u64), ("resid_max", ctypes.c_double)]


class ScatterSrc(ctypes.Structure):
    """vlm_scatter_src_t of include/vlm_hip.h."""
    _fields_ = [("g", c_void_p), ("g_is_f32", ctypes.c_int32), ("ld", ctypes.c_int32), ("first_row", ctypes.c_int32),
                ("row_step", ctypes.c_int32), ("count", ctypes.c_int32)]


class Epilogue(ctypes.Structure):
    _fields_ = [
        ("bias", c_void_p), ("col_scale", c_void_p), ("row_scale", c_void_p), ("residual", c_void_p),
        ("ld_res", ctypes.c_int64), ("aux", c_void_p), ("ld_aux", ctypes.c_int64), ("act", ctypes.c_int32),
        ("alpha", c_float), ("accumulate", ctypes.c_int32), ("reserved", ctypes.c_int32), ("col_sum", c_void_p),
        ("col_sum_ws", c_void_p), ("splitk_ws", c_void_p), ("splitk_ws_bytes", ctypes.c_uint64),
    ]


GEMM_MAX_GROUPS = 4


class GemmGroup(ctypes.Structure):
    _fields_ = [("row0", ctypes.c_int32), ("rows", ctypes.c_int32), ("B", c_void_p), ("ldb", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("bias", c_void_p), ("col_sum", c_void_p), ("col_sum_ws", c_void_p)]


class WgradGroup(ctypes.Structure):
    _fields_ = [("row0", ctypes.c_int32), ("rows", ctypes.c_int32), ("C", c_void_p), ("accumulate", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class WgradProblem(ctypes.Structure):  # vlm_wgrad_problem_t
    _fields_ = [("dy", c_void_p), ("ld_dy", ctypes.c_int32), ("M", ctypes.c_int32), ("x", c_void_p), ("ld_x", ctypes.c_int32),
                ("N", ctypes.c_int32), ("dW", c_void_p), ("ldc", ctypes.c_int32), ("accumulate", ctypes.c_int32)]


class FoldJob(ctypes.Structure):
    _fields_ = [("partials", c_void_p), ("nblocks", ctypes.c_int32), ("D", ctypes.c_int32), ("out0", c_void_p),
                ("out1", c_void_p)]


class LayerScale(ctypes.Structure):  # vlm_layerscale_t
    _fields_ = [("y", c_void_p), ("ldy", ctypes.c_int32), ("gamma", c_void_p), ("row_scale", c_void_p), ("dy", c_void_p),
                ("lddy", ctypes.c_int32), ("dgamma", c_void_p), ("dbias", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t)]


class AttnColsum(ctypes.Structure):
    _fields_ = [("dq", c_void_p * 2), ("dv", c_void_p * 2)]


ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_GELU_DERIV, ACT_MUL_AUX = 0, 1, 2, 3, 4
ATTN_JOINT, ATTN_SEPARATE = 0, 1


class AttnDesc(ctypes.Structure):
    _fields_ = [
        ("qkv", c_void_p), ("ld_qkv", ctypes.c_int32), ("H", ctypes.c_int32), ("total_rows", ctypes.c_int32),
        ("R", ctypes.c_int32), ("bias_t", c_void_p), ("rel_index", c_void_p), ("rel_index_t", c_void_p),
        ("ld_index", ctypes.c_int32), ("index_rows", ctypes.c_int32), ("ld_index_t", ctypes.c_int32),
        ("index_t_rows", ctypes.c_int32), ("head_row0", ctypes.c_int32), ("mode", ctypes.c_int32),
        ("keep0", c_void_p), ("keep1", c_void_p),
        ("B", ctypes.c_int32), ("n0", ctypes.c_int32), ("n1", ctypes.c_int32), ("base0", ctypes.c_int32),
        ("base1", ctypes.c_int32), ("pos1", ctypes.c_int32), ("scale", c_float), ("q_keep0", ctypes.c_int32),
        ("bias_dense", c_void_p), ("bias_dense_t", c_void_p), ("dense_tiles", ctypes.c_int32), ("q_keep1", ctypes.c_int32),
    ]


class LayerScaleJob(ctypes.Structure):
    _fields_ = [("weight", c_void_p), ("gamma", c_void_p), ("bias", c_void_p), ("shadow", c_void_p), ("bias_out", c_void_p),
                ("raw_w", c_void_p), ("raw_b", c_void_p), ("dweight", c_void_p), ("dbias", c_void_p), ("dgamma", c_void_p),
                ("N", ctypes.c_int32), ("K", ctypes.c_int32)]


MAX_LAYERSCALE_JOBS = 32


class VlmError(RuntimeError):
    pass


_ERR = {-1: "VLM_ERR_ARG", -2: "VLM_ERR_LAUNCH", -3: "VLM_ERR_WORKSPACE", -4: "VLM_ERR_UNSUPPORTED"}

# name -> (restype, argtypes); every symbol include/vlm_hip.h declares
SIGNATURES = {
    "vlm_abi_version": (c_int, []),
    "vlm_device_cus": (c_int, []),
    "vlm_set_cu_budget": (c_int, [c_int]),
    "vlm_debug_occupy": (c_int, [c_int, c_int, c_int, c_int, c_void_p]),
    "vlm_layerscale_fold": (c_int, [ctypes.POINTER(LayerScaleJob), c_int, c_void_p]),
    "vlm_layerscale_finish": (c_int, [ctypes.POINTER(LayerScaleJob), c_int, c_void_p]),
    "vlm_merge_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_merge_plan_upload": (c_int, [ctypes.POINTER(MergeJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_merge_run": (c_int, [c_void_p, c_void_p]),
    "vlm_ties_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_ties_plan_upload": (c_int, [ctypes.POINTER(TiesJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_ties_run": (c_int, [c_void_p, c_void_p]),
    "vlm_dare_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_dare_plan_upload": (c_int, [ctypes.POINTER(DareJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_dare_run": (c_int, [c_void_p, c_void_p]),
    "vlm_band_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_band_plan_upload": (c_int, [ctypes.POINTER(BandJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_band_run": (c_int, [c_void_p, c_void_p]),
    "vlm_della_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_della_plan_upload": (c_int, [ctypes.POINTER(DellaJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_della_run": (c_int, [c_void_p, c_void_p]),
    "vlm_pairstats_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_pairstats_plan_upload": (c_int, [ctypes.POINTER(PairStatsJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_pairstats_run": (c_int, [c_void_p, c_void_p]),
    "vlm_stock_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_stock_plan_upload": (c_int, [ctypes.POINTER(StockJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_stock_run": (c_int, [c_void_p, c_void_p]),
    "vlm_sce_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_sce_plan_upload": (c_int, [ctypes.POINTER(SceJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_sce_run": (c_int, [c_void_p, c_void_p]),
    "vlm_sphere_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_sphere_plan_upload": (c_int, [ctypes.POINTER(SphereJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_sphere_run": (c_int, [c_void_p, c_void_p]),
    "vlm_tall_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_tall_plan_upload": (c_int, [ctypes.POINTER(TallJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_tall_run": (c_int, [c_void_p, c_void_p]),
    "vlm_emr_plan_bytes": (c_size_t, [c_int, c_u64]),
    "vlm_emr_plan_upload": (c_int, [ctypes.POINTER(EmrJob), c_int, c_void_p, c_size_t, c_void_p]),
    "vlm_emr_run": (c_int, [c_void_p, c_void_p]),
    "vlm_gemm_bf16": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                              c_int, ctypes.POINTER(Epilogue), c_void_p]),
    "vlm_gemm_bf16_live": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                   c_int, ctypes.POINTER(Epilogue), c_void_p, c_void_p]),
    "vlm_gemm_bf16_grouped": (c_int, [c_int, ctypes.POINTER(GemmGroup), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                      ctypes.POINTER(Epilogue), c_void_p]),
    "vlm_gemm_wgrad_grouped": (c_int, [c_int, ctypes.POINTER(WgradGroup), c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                       c_void_p, c_u64, c_void_p]),
    "vlm_gemm_wgrad_batch": (c_int, [c_int, ctypes.POINTER(WgradProblem), c_int, c_void_p, c_u64, c_void_p]),
    "vlm_attention_fwd": (c_int, [ctypes.POINTER(AttnDesc), c_void_p, c_int, c_void_p, c_void_p]),
    "vlm_attention_bwd_ws_floats": (c_size_t, [ctypes.POINTER(AttnDesc), c_int]),
    "vlm_attention_qkeep_served": (c_int, [ctypes.POINTER(AttnDesc), c_int]),
    "vlm_attention_bwd": (c_int, [ctypes.POINTER(AttnDesc), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                  c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "vlm_attention_bwd_live": (c_int, [ctypes.POINTER(AttnDesc), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                       c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vlm_layernorm_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int,
                                  c_void_p, c_void_p]),
    "vlm_layernorm_bwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                  c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                  ctypes.POINTER(c_int), c_void_p]),
    "vlm_layernorm_bwd_scale": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                        c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                        ctypes.POINTER(LayerScale), ctypes.POINTER(c_int), c_void_p]),
    "vlm_layerscale_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int), c_void_p]),
    "vlm_colreduce_batch": (c_int, [ctypes.POINTER(FoldJob), c_int, c_void_p]),
    "vlm_gemm_set_big_tile_mode": (c_int, [c_int]),
    "vlm_colsum_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_adamw_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_u64, c_float, c_float, c_float,
                               c_float, c_float, c_float, c_float, c_int, c_void_p]),
    "vlm_accumulate_f32_f64": (c_int, [c_void_p, c_void_p, c_u64, c_void_p]),
    "vlm_gram_f64": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_gemm_f64": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.c_double, c_void_p, c_int, c_int, c_void_p, c_int,
                             ctypes.c_double, c_void_p, c_int, c_void_p]),
    "vlm_scale_gram_f64": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_double, c_int, c_void_p]),
    "vlm_cholesky_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "vlm_solve_spd_right_f64": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "vlm_gemm_f64_batched": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.c_double, ctypes.POINTER(c_void_p), c_int, c_int,
                                     ctypes.POINTER(c_void_p), c_int, ctypes.c_double, ctypes.POINTER(c_void_p), c_int, c_int, c_void_p]),
    "vlm_cholesky_f64_batched": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_void_p, c_void_p]),
    "vlm_solve_spd_right_f64_batched": (c_int, [ctypes.POINTER(c_void_p), c_int, ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_void_p]),
    "vlm_iso_parts": (c_int, [c_int, c_int]),
    "vlm_iso_delta": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.POINTER(c_void_p),
                              c_void_p, c_int, c_void_p]),
    "vlm_iso_gram": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.c_double, ctypes.POINTER(c_void_p), c_int, c_void_p]),
    "vlm_iso_step": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, c_int, c_void_p, c_int,
                             c_void_p]),
    "vlm_iso_finish": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int,
                               ctypes.c_double, c_void_p, c_int, c_int, c_void_p]),
    "vlm_wudi_parts": (c_int, [c_int, c_int]),
    "vlm_wudi_work_doubles": (ctypes.c_size_t, [c_int, c_int]),
    "vlm_wudi_state_offset": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "vlm_wudi_prepare": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.POINTER(c_void_p),
                                 c_void_p, c_int, c_void_p]),
    "vlm_wudi_step": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, ctypes.c_double, c_void_p, c_int, c_void_p]),
    "vlm_wudi_finish": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int,
                                ctypes.c_double, c_void_p, c_int, c_void_p]),
    "vlm_svd_work_doubles": (ctypes.c_size_t, [c_int, c_int]),
    "vlm_svd_steps": (c_int, [c_int]),
    "vlm_svd_reset": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_void_p]),
    "vlm_svd_sweep": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p]),
    "vlm_svd_finish": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, ctypes.c_double, c_int, c_void_p]),
    "vlm_tsv_delta": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, ctypes.POINTER(c_void_p), c_int, c_void_p]),
    "vlm_tsv_gather": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p),
                               ctypes.POINTER(c_void_p), c_int, c_void_p]),
    "vlm_tsv_apply": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                              ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.c_double, c_int, c_void_p]),
    "vlm_cross_entropy_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p]),
    "vlm_cross_entropy_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p]),
    "vlm_l2norm_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vlm_l2norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "vlm_contrastive_ws_floats": (c_size_t, [c_int]),
    "vlm_contrastive": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "vlm_small_cross_entropy": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vlm_cross_entropy_reduce": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_int64, c_void_p, c_void_p]),
    "vlm_scale_by_scalar": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), c_int, c_void_p, c_void_p]),
    "vlm_text_rows_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_float, c_float,
                                  c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "vlm_text_rows_bwd_ws_floats": (c_size_t, [c_int]),
    "vlm_text_rows_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                  c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vlm_image_rows_prep": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "vlm_image_lead_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_image_rows_bwd_ws_floats": (c_size_t, [c_int]),
    "vlm_image_rows_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vlm_tanh_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_act_bwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_colsum_small": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_sample_negatives": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vlm_weighted_sum": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_float), c_int, c_void_p, c_void_p]),
    "vlm_scatter_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "vlm_cast_f32_bf16": (c_int, [c_void_p, c_void_p, c_u64, c_void_p]),
    "vlm_embedding_bwd": (c_int, [c_void_p, c_int, c_void_p, ctypes.c_int64, c_int, ctypes.c_int64, c_void_p, c_int,
                                  ctypes.c_int64, c_void_p]),
    "vlm_bias_dense_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "vlm_bias_dense": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p]),
    "vlm_transpose_bf16_tiles": (c_int, [c_void_p, c_int, c_void_p]),
    "vlm_droppath_sites": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
    "vlm_droppath_rows": (c_int, [c_void_p, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vlm_patch_im2col": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
}


def get_lib():
    """Load the HIP library.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VlmError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
        import torch  # noqa: F401  -- torch's bundled HIP runtime must be the one libvlm_hip.so binds to
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise VlmError(f"{what} failed: {_ERR.get(rc, rc)}")


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise VlmError("vl_merging_amd ops run on the GPU only (tensor on %s); there is no CPU path" % t.device)
