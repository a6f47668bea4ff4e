"""TIES merge, host side (no GPU): the ABI additions, the argument checks, the numpy restatement of the rule against cases small
enough to check by eye, and merge_ckpt.py's command line.  The reference has no TIES: nothing here is pinned to it."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ties_restatement import keep_count, ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32


def f32(*v):
    return np.array(v, dtype=F)


# ---------------------------------------------------------------------------------------------------------------- ABI
def header_text():
    txt = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


C_SIZES = {"void*": 8, "const void*": 8, "uint64_t": 8, "int32_t": 4, "uint32_t": 4, "float": 4}


def header_struct_size(name):
    """Size of a struct of the header whose members are naturally aligned without padding (checked: running offset % size == 0)."""
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", header_text())
    assert m, name + " is not declared"
    off = 0
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        ty, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        for n in names.split(","):
            arr = re.search(r"\[(\w+)\]", n)
            count = {"VLM_MERGE_MAX_SRC": 4}.get(arr.group(1)) if arr and not arr.group(1).isdigit() else int(arr.group(1)) if arr else 1
            assert off % C_SIZES[ty] == 0
            off += C_SIZES[ty] * count
    assert off % 8 == 0
    return off


def test_ties_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_ties_plan_bytes", "vlm_ties_plan_upload", "vlm_ties_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_abi_version() == 11


def test_ties_struct_layouts_match_the_header(pkg):
    L = importlib.import_module("vl_merging_amd._lib")
    assert ctypes.sizeof(L.TiesJob) == header_struct_size("vlm_ties_job_t") == 96
    assert ctypes.sizeof(L.TiesHeader) == header_struct_size("vlm_ties_header_t") == 80
    assert ctypes.sizeof(L.TiesState) == header_struct_size("vlm_ties_state_t") == 16
    assert L.TIES_COUNTERS == L.MERGE_MAX_SRC + 2 and "VLM_TIES_COUNTERS (VLM_MERGE_MAX_SRC + 2)" in header_text()
    assert ctypes.sizeof(L.MergeJob) == 80  # the existing job struct is untouched


def test_ties_plan_bytes_and_host_side_argument_checks(pkg):
    """vlm_ties_plan_upload rejects bad jobs before it touches the device (the checks come first, as in the merge entry points)."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_ties_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_ties_plan_bytes(1, 4096), lib.vlm_ties_plan_bytes(2, 8192)
    assert 4 * 2048 * 8 < small < big  # holds at least one job's four histograms
    job = L.TiesJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam = 0x1000, 0x2000, 2, 16, 1.0
    job.src[0], job.src[1] = 0x3000, 0x4000
    job.k[0], job.k[1] = 4, 4
    arr = (L.TiesJob * 1)(job)
    ws = ctypes.c_void_p(0x10000)
    assert lib.vlm_ties_plan_upload(arr, 1, ctypes.c_void_p(0), small, None) == -1            # no workspace
    assert lib.vlm_ties_plan_upload(arr, 0, ws, small, None) == -1                             # no jobs
    assert lib.vlm_ties_plan_upload(arr, 1, ws, 64, None) == -3                                # VLM_ERR_WORKSPACE
    for field, value in (("n_src", 0), ("n_src", 5), ("dst", 0), ("base", 0), ("dst", 0x1004), ("base", 0x2008), ("n_elem", 0),
                         ("dst", 0x2000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0)):  # dst equal to / overlapping an input
        bad = L.TiesJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert lib.vlm_ties_plan_upload((L.TiesJob * 1)(bad), 1, ws, small, None) == -1, (field, value)
    for idx, src, k in ((1, 0, 4), (1, 0x4004, 4), (0, 0x3000, 0), (0, 0x3000, 17)):
        bad = L.TiesJob.from_buffer_copy(bytes(job))
        bad.src[idx], bad.k[idx] = src, k
        assert lib.vlm_ties_plan_upload((L.TiesJob * 1)(bad), 1, ws, small, None) == -1, (idx, src, k)
    assert lib.vlm_ties_run(ctypes.c_void_p(0), None) == -1


def test_cpu_device_and_bad_density_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.TiesPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.ties_merge({}, cfg, central_weight={}, device="cpu")
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            merge.ties_merge({}, cfg, central_weight={}, density=bad)
        with pytest.raises(ValueError):
            merge.ties_keep_count(bad, 10)
    assert merge.ties_keep_count(0.2, 12289) == keep_count(0.2, 12289) == 2458
    assert merge.ties_keep_count(0.05, 12289) == 615 and merge.ties_keep_count(1, 12289) == 12289
    assert merge.ties_keep_count(1e-9, 3) == 1 and merge.ties_keep_count(0.5, 1) == 1
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.ties_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


def test_default_config_has_no_ties_key(pkg):
    cfg = importlib.import_module("vl_merging_amd.vilt.config").default_config()
    assert not [k for k in cfg if k.startswith("ties") or "ties_" in k or "density" in k]


# ------------------------------------------------------------------------------------- the restatement, by hand
def test_worked_case_of_the_issue():
    """c = 1; t_v = [2, .5, 0, -1], t_l = [-2, .5, 2, 1]; K = 2: thr_v = 1 keeps {2, -1}, thr_l = 2 keeps {-2, 2}.
    i0: 2 + -2 = 0 -> dropped -> 1.  i1: nothing kept -> 1.  i2: only l's 2 -> 1 + 2 = 3.  i3: only v's -1 -> 0."""
    out, info = ties(f32(1, 1, 1, 1), [f32(3, 1.5, 1, 0), f32(-1, 1.5, 3, 2)], 0.5, 1)
    assert out.tolist() == [1, 1, 3, 0]
    assert info["threshold"] == [1.0, 2.0] and info["kept"] == [2, 2]
    assert info["conflict"] == 1 and info["empty"] == 2


def test_tie_at_the_threshold_keeps_both():
    """t = [3, -2, 2, 1], K = 2: the 2nd largest magnitude is 2 and both +-2 are kept (3 entries kept, not 2)."""
    c = f32(0, 0, 0, 0)
    out, info = ties(c, [f32(3, -2, 2, 1), f32(3, -2, 2, 1)], 0.5, 1)
    assert info["kept"] == [3, 3] and info["threshold"] == [2.0, 2.0]
    assert out.tolist() == [3, -2, 2, 0] and info["empty"] == 1 and info["conflict"] == 0


def test_exact_cancellation_gives_the_central_value():
    c = f32(5, 7)
    out, info = ties(c, [f32(6.5, 8), f32(3.5, 6)], 1.0, 0.75)  # t = [1.5, 1], [-1.5, -1]: s = 0 everywhere
    assert out.tobytes() == c.tobytes()
    assert info["conflict"] == 2 and info["empty"] == 2 and info["kept"] == [2, 2]


def test_element_kept_by_one_source_only():
    """K = 1 of 2: v keeps index 0 (t = 4), l keeps index 1 (t = -8): out = c + lam * t of the only keeper."""
    c = f32(1, 1)
    out, info = ties(c, [f32(5, 1.5), f32(1.25, -7)], 0.5, 0.75)
    assert out.tolist() == [1 + 0.75 * 4, 1 + 0.75 * -8]
    assert info["kept"] == [1, 1] and info["empty"] == 0 and info["conflict"] == 0


def test_negative_zero_task_vector_entries():
    """W - c = -0.0 cannot come from a subtraction of equal finite numbers (x - x = +0.0), but (-0.0) - (+0.0) = -0.0 can: key(-0.0)
    = 0 like +0.0, it is kept at density 1, counts as zero in the election (neither > 0 nor < 0) and the element is empty."""
    c = f32(0.0, 0.0, 2.0)
    out, info = ties(c, [f32(-0.0, 1.0, 2.0), f32(-0.0, -0.0, 3.0)], 1.0, 1)
    assert info["kept"] == [3, 3] and info["threshold_bits"] == [0, 0]
    assert out.tolist() == [0.0, 1.0, 3.0] and not np.signbit(out[0])
    assert info["empty"] == 1 and info["conflict"] == 0
    # the elected sum of a lone -0.0: (+0.0) + (-0.0) = +0.0, and -0.0 central values survive only through c + lam * 0
    out, _ = ties(f32(-0.0), [f32(-0.0), f32(-0.0)], 1.0, 1)
    assert out.tolist() == [0.0] and not np.signbit(out[0])  # (-0.0) + (+0.0) = +0.0


def test_density_one_same_sign_is_the_plain_mean():
    rng = np.random.default_rng(5)
    c = rng.standard_normal(257).astype(F)
    ts = [np.abs(rng.standard_normal(257)).astype(F) + F(0.5) for _ in range(3)]
    srcs = [c + t for t in ts]
    lam = 0.75
    out, info = ties(c, srcs, 1.0, lam)
    t = [s - c for s in srcs]  # the task vectors as fp32 sees them
    assert all((x > 0).all() for x in t)
    naive = c + F(lam) * ((((F(0) + t[0]) + t[1]) + t[2]) / F(3))
    assert out.tobytes() == naive.tobytes()
    assert info["kept"] == [257] * 3 and info["empty"] == 0 and info["conflict"] == 0


def test_restatement_counts_on_random_data():
    """n = 12 289, three sources: without ties in the data the kept count IS K (615 / 2 458 / 12 289 at density 0.05 / 0.2 / 1);
    everything is finite; density 1 leaves no element empty."""
    rng = np.random.default_rng(0)
    n = 12289
    c = rng.standard_normal(n).astype(F)
    srcs = [c + rng.standard_normal(n).astype(F) * F(0.1) for _ in range(3)]
    for density, K in ((0.05, 615), (0.2, 2458), (1.0, 12289)):
        out, info = ties(c, srcs, density, 1)
        assert info["kept"] == [K] * 3 and np.isfinite(out).all()
        if density == 1.0:
            assert info["empty"] == 0
        else:
            assert info["empty"] > 0 and (out == c).sum() >= info["empty"]


# ----------------------------------------------------------------------------------------------- merge_ckpt.py
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_help_runs_without_a_device():
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for word in ("--method", "interp", "taskvec", "ties", "--density", "--lambda", "--ratio", "--central", "--report"):
        assert word in r.stdout


def test_merge_ckpt_argument_and_config_parsing(pkg):
    mc = tool()
    args, cfg = mc.parse_args(["--method", "ties", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--density", "0.1", "--lambda", "0.75",
                               "--report", "r.json", "with", "task_finetune_irtr_f30k_square_randaug_base", "only_activate_used_experts=True",
                               "vlffn_start_layer_index=10"])
    assert (args.method, args.ckpt, args.out, args.density, args.report) == ("ties", "a.ckpt", "b.ckpt", 0.1, "r.json")
    assert cfg["sum_lambda"] == 0.75 and cfg["only_activate_used_experts"] is True and cfg["vlffn_start_layer_index"] == 10
    assert cfg["loss_names"]["irtr"] == 1  # the named config was applied
    args, cfg = mc.parse_args(["--method", "interp", "--ckpt", "a", "--out", "b", "--ratio", "0.3", "merge_ratio=0.9"])
    assert cfg["merge_ratio"] == 0.3  # the option wins over the config word
    args, cfg = mc.parse_args(["--method", "taskvec", "--ckpt", "a", "--out", "b", "sum_lambda=0.4", "central_weight=c.ckpt"])
    assert cfg["sum_lambda"] == 0.4 and cfg["central_weight"] == "c.ckpt" and args.central is None
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "ties", "--ckpt", "a", "--out", "b", "--density", "0"])
    with pytest.raises(KeyError):
        mc.parse_args(["--method", "ties", "--ckpt", "a", "--out", "b", "no_such_config"])
    with pytest.raises(SystemExit):
        mc.parse_args(["--method", "median", "--ckpt", "a", "--out", "b"])
