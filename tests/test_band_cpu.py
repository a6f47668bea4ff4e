"""Model Breadcrumbs merge, host side (no GPU): the numpy restatement of the rule against a sort-based brute force and against the
TIES restatement, the ranks, merge_ckpt.py's command line, the ABI additions and the build's verdict on the new kernels.  The
reference has no such merge: nothing here is pinned to it."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from band_restatement import LINEAR, NO_OUTLIER, TIES, band, ranks, thresholds
from test_build_cpu import resources  # noqa: F401  (the fixture: brings the build and its resource record up to date)
from ties_restatement import keep_count, ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
SIZES = [1, 2, 3, 5, 1023, 4097, 70001]
PAIRS = [(0.9, 0.01), (0.85, 0.007), (0.5, 0.5), (1, 0), (1, 0.3), (0.001, 0.999)]


def inputs(n, S, seed):
    """Ordinary floats with a quarter of the entries on a dyadic grid (equal magnitudes: ties at the thresholds) and zeros."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(n).astype(F)
    srcs = [(c + rng.standard_normal(n).astype(F) * F(0.1)).astype(F) for _ in range(S)]
    grid = np.arange(n) % 4 == 0
    cg = (rng.integers(-16, 17, n) / 8).astype(F)
    c[grid] = cg[grid]
    for m in range(S):
        srcs[m][grid] = (cg + (rng.integers(-4, 5, n) / 8).astype(F))[grid]
    return c, srcs


# ------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", SIZES)
def test_restatement_against_sorted_keys(n):
    """The k-th entry of the descending sorted keys is each threshold; the masks follow from the two compares of the rule."""
    c, srcs = inputs(n, 2, seed=n)
    for density, gamma in PAIRS:
        k_hi, k_lo = ranks(n, density, gamma)
        rk = [(k_hi, k_lo), (0, k_lo)]
        out, info = band(c, srcs, rk, 0.75, LINEAR)
        d = np.zeros(n, F)
        for m, w in enumerate(srcs):
            t = w - c
            key = t.view(np.uint32) & np.uint32(0x7FFFFFFF)
            desc = np.sort(key)[::-1]
            lo = int(desc[rk[m][1] - 1])
            hi = int(desc[rk[m][0] - 1]) if rk[m][0] >= 1 else NO_OUTLIER
            assert (info["threshold_lo_bits"][m], info["threshold_hi_bits"][m]) == (lo, hi) == thresholds(key, *rk[m])[:2]
            kept = np.array([lo <= int(k) < hi for k in key]) if n <= 5000 else (key >= lo) & (key.astype(np.int64) < hi)
            assert np.array_equal(info["kept_mask"][m], kept)
            assert info["kept"][m] == int(kept.sum()) and info["outlier"][m] == int((key.astype(np.int64) >= hi).sum())
            assert info["outlier"][m] >= rk[m][0] and info["kept"][m] + info["outlier"][m] >= rk[m][1]
            d = d + np.where(kept, t, F(0))
        assert out.tobytes() == (c + F(0.75) * d).tobytes()
        assert info["threshold_hi"][1] is None and info["outlier"][1] == 0


@pytest.mark.parametrize("density", [0.05, 0.2, 1.0])
def test_restatement_without_outliers_in_ties_mode_is_ties(density):
    for n, S in ((12289, 3), (4097, 2), (5, 2), (1, 2)):
        c, srcs = inputs(n, S, seed=3 * n + S)
        K = keep_count(density, n)
        want, winfo = ties(c, srcs, density, 0.75)
        got, info = band(c, srcs, [(0, K)] * S, 0.75, TIES)
        assert got.tobytes() == want.tobytes()
        assert info["threshold_lo_bits"] == winfo["threshold_bits"] and info["threshold_hi_bits"] == [NO_OUTLIER] * S
        assert (info["kept"], info["conflict"], info["empty"]) == (winfo["kept"], winfo["conflict"], winfo["empty"])
        assert info["outlier"] == [0] * S


def test_worked_case():
    """c = 0; t = [8, -4, 2, 1, -1, 0.5], ranks (1, 4): thr_hi = 8 drops {8}, thr_lo = 1 keeps {-4, 2, 1, -1} (both ones: ties
    at the lower threshold are kept).  Ranks (2, 3) on t2 = [4, -4, 2, 1, 1, 0]: thr_hi = 4 drops both fours."""
    c = np.zeros(6, F)
    t = np.array([8, -4, 2, 1, -1, 0.5], F)
    t2 = np.array([4, -4, 2, 1, 1, 0], F)
    out, info = band(c, [t, t2], [(1, 4), (2, 3)], 1, LINEAR)
    assert info["threshold_lo"] == [1.0, 2.0] and info["threshold_hi"] == [8.0, 4.0]
    assert info["kept"] == [4, 1] and info["outlier"] == [1, 2]
    assert out.tolist() == [0, -4, 4, 1, -1, 0] and info["empty"] == 2 and info["conflict"] == 0
    out, info = band(c, [t, t2], [(1, 4), (2, 3)], 1, TIES)
    assert out.tolist() == [0, -4, 2, 1, -1, 0] and info["empty"] == 2
    # both thresholds the same key: the source contributes nothing
    out, info = band(c, [np.full(6, 0.5, F)], [(2, 5)], 1, LINEAR)
    assert info["kept"] == [0] and info["outlier"] == [6] and out.tobytes() == c.tobytes() and info["empty"] == 6


# ------------------------------------------------------------------------------------- band_ranks
def test_band_ranks(pkg):
    merge = importlib.import_module("vl_merging_amd.merge")
    for n in SIZES:
        for density, gamma in PAIRS:
            k_hi, k_lo = merge.band_ranks(n, density, gamma)
            assert 0 <= k_hi < k_lo <= n, (n, density, gamma)
            assert (k_hi, k_lo) == ranks(n, density, gamma)
    assert merge.band_ranks(1023, 0.9, 0.01) == (10, 931)
    assert merge.band_ranks(70001, 0.9, 0.01) == (700, 63701)
    assert all(merge.band_ranks(1, d, g) == (0, 1) for d, g in PAIRS)
    for density, gamma in ((0, 0.01), (1.5, 0.01), (0.9, 1), (0.9, -0.1), (float("nan"), 0.01), (0.9, float("nan"))):
        with pytest.raises(ValueError):
            merge.band_ranks(100, density, gamma)


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.BandPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.band_merge({}, cfg, central_weight={}, device="cpu")
    with pytest.raises(L.VlmError):
        merge.band_merge({}, cfg, central_weight={}, mode="median")
    for kw in (dict(density=0.0), dict(density=1.5), dict(gamma=1.0), dict(gamma=-0.1), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            merge.band_merge({}, cfg, central_weight={}, **kw)
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.band_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ------------------------------------------------------------------------------------- merge_ckpt.py
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_parses_breadcrumbs_before_any_device(pkg):
    mc = tool()
    io = ["--ckpt", "a.ckpt", "--out", "b.ckpt"]
    args, cfg = mc.parse_args(["--method", "breadcrumbs"] + io + ["--density", "0.9", "--gamma", "0.05", "--band-mode", "ties",
                                                                 "--lambda", "0.75", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.density, args.gamma, args.band_mode) == ("breadcrumbs", 0.9, 0.05, "ties")
    assert cfg["sum_lambda"] == 0.75 and cfg["vlffn_start_layer_index"] == 10
    args, _ = mc.parse_args(["--method", "breadcrumbs"] + io)
    assert (args.density, args.gamma, args.band_mode) == (0.2, 0.01, "linear")  # --density keeps its default
    for bad in (["--gamma", "1"], ["--gamma", "-0.1"], ["--gamma", "nan"], ["--density", "0"], ["--density", "1.5"]):
        with pytest.raises(ValueError):
            mc.parse_args(["--method", "breadcrumbs"] + io + bad)
    with pytest.raises(SystemExit):
        mc.parse_args(["--method", "breadcrumbs"] + io + ["--band-mode", "median"])
    # the other methods parse as before (a gamma they do not use is not looked at)
    args, _ = mc.parse_args(["--method", "ties"] + io + ["--density", "0.1"])
    assert (args.method, args.density) == ("ties", 0.1)
    args, _ = mc.parse_args(["--method", "dare"] + io + ["--drop", "0.5", "--gamma", "7"])
    assert (args.method, args.drop, args.dare_mode) == ("dare", 0.5, "linear")
    args, cfg = mc.parse_args(["--method", "interp"] + io + ["--ratio", "0.3"])
    assert cfg["merge_ratio"] == 0.3
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "ties"] + io + ["--density", "0"])
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for word in ("breadcrumbs", "--gamma", "--band-mode"):
        assert word in r.stdout


# ------------------------------------------------------------------------------------- ABI
def test_band_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_band_job_t": L.BandJob, "vlm_band_header_t": L.BandHeader, "vlm_band_state_t": L.BandState}
    lines = ['printf("VLM_BAND_COUNTERS %d\\n", VLM_BAND_COUNTERS);', 'printf("VLM_BAND_TIES %d\\n", VLM_BAND_TIES);',
             'printf("VLM_BAND_LINEAR %d\\n", VLM_BAND_LINEAR);']
    for cname, ty in types.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in ty._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vlm_hip.h"\nint main() {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    got = dict(ln.split() for ln in r.stdout.splitlines())
    want = {"VLM_BAND_COUNTERS": str(L.BAND_COUNTERS), "VLM_BAND_TIES": str(L.BAND_TIES), "VLM_BAND_LINEAR": str(L.BAND_LINEAR)}
    for cname, ty in types.items():
        want[cname] = str(ctypes.sizeof(ty))
        for field, _ in ty._fields_:
            want[cname + "." + field] = str(getattr(ty, field).offset)
    assert got == want
    assert (ctypes.sizeof(L.BandJob), ctypes.sizeof(L.BandHeader), ctypes.sizeof(L.BandState)) == (136, 80, 24)
    assert L.BAND_COUNTERS == 2 * L.MERGE_MAX_SRC + 2 == 10
    assert ctypes.sizeof(L.DareJob) == 96 and ctypes.sizeof(L.TiesJob) == 96 and ctypes.sizeof(L.MergeJob) == 80  # untouched


def test_band_entry_points_and_host_side_argument_checks(pkg):
    """vlm_band_plan_upload rejects bad jobs before it touches the device (the checks come first, as in its TIES namesake)."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    for s in ("vlm_band_plan_bytes", "vlm_band_plan_upload", "vlm_band_run"):
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_band_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_band_plan_bytes(1, 4096), lib.vlm_band_plan_bytes(2, 8192)
    assert 4 * 2048 * 8 < small < big  # holds at least one job's four histograms
    # the second rank costs no histogram: what a band plan needs beyond a TIES plan is the wider jobs, states and counters
    assert small - lib.vlm_ties_plan_bytes(1, 4096) < 1024
    job = L.BandJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam, job.mode = 0x1000, 0x2000, 2, 16, 1.0, L.BAND_LINEAR
    job.src[0], job.src[1] = 0x3000, 0x4000
    job.k_hi[0], job.k_hi[1], job.k_lo[0], job.k_lo[1] = 1, 0, 4, 16
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_band_plan_upload((L.BandJob * 1)(j), n, w, nbytes, None)

    assert upload(job) == -3                                 # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(job, w=ctypes.c_void_p(0)) == -1           # no workspace
    assert upload(job, n=0) == -1                            # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("dst", 0), ("base", 0), ("dst", 0x1004), ("base", 0x2008), ("n_elem", 0),
                         ("mode", 2), ("mode", -1),
                         ("dst", 0x2000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0)):  # dst equal to / overlapping an input
        bad = L.BandJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for idx, k_hi, k_lo in ((0, 4, 4), (0, 5, 4), (1, 0, 17), (1, 0, 0), (0, 16, 17)):
        bad = L.BandJob.from_buffer_copy(bytes(job))
        bad.k_hi[idx], bad.k_lo[idx] = k_hi, k_lo
        assert upload(bad) == -1, (idx, k_hi, k_lo)
    assert lib.vlm_band_run(ctypes.c_void_p(0), None) == -1


# ------------------------------------------------------------------------------------- the build's verdict
def test_band_kernels_keep_the_occupancy_the_ties_grids_count_on(resources):  # noqa: F811
    """The band kernels take the TIES grids over (csrc/ties_select.h): four histogram workgroups per CU with 32 KiB of LDS each
    -- the second rank lives in the other half of a source's bins, not in bins of its own -- and the apply pass three to a CU.
    None may spill: the kernels are HBM-bound streams."""
    hist = {k: v for k, v in resources.items() if "vlm_select_hist_kernel" in k and "band_sel" in k}
    assert len(hist) == 3, sorted(hist)  # PASS 0 / 1 / 2
    for name, r in hist.items():
        assert r["Occupancy"] == 4 and r["LDS Size"] == 32768, (name, r)
    apply_band = [v for k, v in resources.items() if "vlm_band_apply_kernel" in k]
    assert len(apply_band) == 1 and apply_band[0]["Occupancy"] >= 3, apply_band
    scan = [v for k, v in resources.items() if "vlm_select_scan_kernel" in k and "band_sel" in k]
    assert len(scan) == 3
    for r in list(hist.values()) + apply_band + scan:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
