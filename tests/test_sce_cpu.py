"""SCE, host side (no GPU): the restatement of the rule (sce_restatement.py) against cases worked out by hand and against the
published form written in float64, the ABI additions, the host surface, merge_ckpt.py's command line and the build's record of the
kernels.  The reference has no SCE: nothing here is pinned to it."""
import ctypes
import importlib
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sce_restatement as R
from test_ties_cpu import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32


def f32(*v):
    return np.array(v, dtype=F)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_identical_sources_are_taken_whole():
    """W_0 = W_1 = c + x: mean = x, e = 0, var = +0.0 at every element, so thr = 0 whatever K is and all five are selected (kept = 5
    > K = 1).  sq_0 = sq_1, w = (0.5, 0.5); s = 2 x, both agree wherever x != 0: num = 0.5 x + 0.5 x = x, den = 1, d = x.  Where
    x = 0 nothing agrees (one empty element) and d = +0.0 = x.  dst = c + lam x, exact on these dyadic values."""
    c = f32(0.5, -1.25, 3.0, 0.0, 7.0)
    x = f32(1.0, 1.0, -1.0, 0.125, 0.0)
    for S in (2, 3, 4):
        out, row = R.sce(c, [c + x] * S, density=0.2, lam=0.5)
        assert (row["K"], row["threshold_bits"], row["kept"], row["conflict"], row["empty"]) == (1, 0, 5, 0, 1)
        if S != 3:  # 1 / 3 is not a float: the three weights are f32(1 / 3) each and d is x only up to rounding
            assert row["weight"] == [1.0 / S] * S and out.tolist() == (c + F(0.5) * x).tolist()
        assert row["sq"] == [3.015625] * S and row["tot"] == S * 3.015625


def test_one_source_is_the_task_vector_job():
    """S = 1: mean = x, var = +0.0, everything selected, sq = sum x^2 = 0.25 + 36 + 0, w = f32(sq / sq) = 1; s = x, d = 1 x / 1 = x:
    dst = c + lam x.  The zero entry of x is the one empty element."""
    c, w = f32(1, 2, 3), f32(1.5, -4, 3)
    out, row = R.sce(c, [w], density=0.5, lam=1.0)
    assert out.tolist() == w.tolist()
    assert (row["K"], row["kept"], row["sq"], row["tot"], row["weight"], row["empty"], row["conflict"]) == (2, 3, [36.25], 36.25, [1.0], 1, 0)
    out, _ = R.sce(c, [w], density=1.0, lam=0.5)
    assert out.tolist() == (c + F(0.5) * (w - c)).tolist()


def test_opposite_entries_elect_nothing():
    """x_0 = (2, 1, 4), x_1 = (-2, 3, 4): var = (4, 1, 0), K = 2 selects elements 0 and 1 (thr = bits(1.0)).  Element 0: tt = (2, -2),
    s = 0: no sign is elected, the element is empty AND a conflict, d = +0.0, dst = c (mergekit would elect +).  Element 1:
    sq = (4 + 1, 4 + 9) = (5, 13), tot = 18, w = f32(5/18), f32(13/18); both agree: d = (w_0 1 + w_1 3) / (w_0 + w_1).  Element 2 is
    not selected: empty."""
    c = f32(1, 1, 1)
    out, row = R.sce(c, [c + f32(2, 1, 4), c + f32(-2, 3, 4)], density=0.5, lam=1.0)
    assert (row["K"], row["kept"], row["threshold"], row["conflict"], row["empty"]) == (2, 2, 1.0, 1, 2)
    assert (row["sq"], row["tot"]) == ([5.0, 13.0], 18.0) and row["weight"] == [float(F(5 / 18)), float(F(13 / 18))]
    w0, w1 = F(5 / 18), F(13 / 18)
    assert out.tolist() == [1.0, float(F(1) + (w0 * F(1) + w1 * F(3)) / (w0 + w1)), 1.0]


def test_a_source_that_is_zero_on_the_selected_set_has_weight_zero():
    """x_0 = (0, 0, 1, 1), x_1 = (4, -2, 1, 1): var = (4, 1, 0, 0), K = 2 selects elements 0 and 1, where x_0 is zero: sq = (0, 20),
    w = (+0.0, 1.0).  Source 0 never agrees (its tt is zero); d = 1.0 x_1 / 1.0 on the selected elements, +0.0 elsewhere."""
    c = f32(0.5, 0.5, 0.5, 0.5)
    out, row = R.sce(c, [c + f32(0, 0, 1, 1), c + f32(4, -2, 1, 1)], density=0.5, lam=1.0)
    assert (row["sq"], row["tot"], row["weight"], row["weight_bits"]) == ([0.0, 20.0], 20.0, [0.0, 1.0], [0, 0x3F800000])
    assert math.copysign(1.0, row["weight"][0]) == 1.0
    assert out.tolist() == [4.5, -1.5, 0.5, 0.5] and (row["kept"], row["conflict"], row["empty"]) == (2, 0, 2)


def test_sources_equal_to_the_central_tensor_give_it_back():
    """Every x is +0.0: var = 0, all selected, sq = 0, tot = 0 is not > 0: the uniform weights f32(1 / S); nothing agrees anywhere:
    every element is empty, d = +0.0 and dst = c bit for bit (c holds no -0.0)."""
    c = f32(0.5, -1.25, 3.0, 0.0, 7.0, 1e-3)
    for S in (1, 2, 3, 4):
        out, row = R.sce(c, [c.copy() for _ in range(S)], density=0.3, lam=0.75)
        assert out.tobytes() == c.tobytes()
        assert (row["tot"], row["sq"], row["kept"], row["empty"], row["conflict"]) == (0.0, [0.0] * S, 6, 6, 0)
        assert row["weight"] == [float(F(1.0 / S))] * S and row["weight_bits"] == [int(F(1.0 / S).view(np.uint32))] * S


def test_a_duplicate_of_the_threshold_key_is_selected_too():
    """Eight elements with x_1 = -x_0 = -a: mean = 0, var = a^2.  a = (5, 4, 3, 3, 3, 2, 1, 0): K = 3 puts the threshold on the first
    3; its two duplicates are selected as well: kept = 5 > K.  With keep = 5 the same set is selected."""
    a = f32(5, 4, 3, 3, 3, 2, 1, 0)
    c = np.zeros(8, F)
    out, row = R.sce(c, [a, -a], density=0.3, lam=1.0)
    assert (row["K"], row["kept"], row["threshold"], row["threshold_bits"]) == (3, 5, 9.0, int(F(9).view(np.uint32)))
    assert row["sq"] == [25.0 + 16 + 27] * 2 and (row["conflict"], row["empty"]) == (5, 8) and out.tobytes() == c.tobytes()
    out5, row5 = R.sce(c, [a, -a], density=None, lam=1.0, keep=5)
    assert {**row5, "K": 3} == row and out5.tobytes() == out.tobytes()


# ------------------------------------------------------------------------------------------------ the published form
def published(c, srcs, k, lam):
    """SCE as mergekit's `sce` states it, in float64, but for its K (here k elements are selected, where mergekit takes
    int(density * count_nonzero(var))): variance across the sources (population), the top k by a true top-k, weights = the mean
    square of the selected deltas normalised to sum 1, majority sign = sign of the sum with zero counted as +, the mean of the
    agreeing entries weighted by them, the denominator clamped at 1e-6.  Returns (d, selection mask)."""
    tv = np.stack([w.astype(np.float64) - c.astype(np.float64) for w in srcs])
    var = tv.var(axis=0)
    mask = np.zeros(var.size, bool)
    mask[np.argsort(-np.abs(var), kind="stable")[:k]] = True
    tv = tv * mask
    wgt = (tv ** 2).mean(axis=1)
    wgt = wgt / wgt.sum() if abs(wgt.sum()) >= 1e-6 else np.full(len(srcs), 1.0 / len(srcs))
    majority = np.where(tv.sum(axis=0) >= 0, 1.0, -1.0)
    agree = np.sign(tv) == majority
    num = (tv * wgt[:, None] * agree).sum(axis=0)
    den = (wgt[:, None] * agree).sum(axis=0)
    return num / np.maximum(den, 1e-6), mask


@pytest.mark.parametrize("S", [2, 4])
def test_agreement_with_the_published_form(S):
    """Dyadic inputs: c and every task vector are integers over 8 with |x| <= 4, so with S a power of two the sum, the mean, every
    e_m, its square, q and var are exact in fp32 and in float64 alike: the two forms rank the same variances.  K is moved to the
    nearest place where the K-th and the (K + 1)-th largest variance differ, so the published top-k and the rule's `>= thr`
    select the same set (asserted).  x_0 is odd over 8 and the others even over 8: no selected element sums to zero, where the two
    forms differ on purpose.
    Tolerance of d, relative: (4 S + 4) 2^-24 is the bound this method was accepted with; the count made here is smaller.  The A <= S agreeing entries
    share a sign and the weights are positive, so nothing cancels and a sum's relative error is at most that of its worst term.
    A term of num carries the rounding of its weight f32(sq / tot), of its product, and of the A - 1 additions it passes through
    (the first addition, to +0.0, is exact): A + 1.  A term of den carries its weight's rounding and A - 1 additions: A.  One
    division.  To first order that is (A + 1) + A + 1 = 2 A + 2 <= 2 S + 2 roundings of at most 2^-24 each -- half the bound, which
    also covers the second-order terms; the float64 form's own error (2^-53 per operation) is far below one unit of it."""
    n = 4097
    rng = np.random.default_rng(100 + S)
    c = (rng.integers(-16, 17, n) / 8).astype(F)
    xs = [((2 * rng.integers(-16, 16, n) + 1) / 8).astype(F)] + [((2 * rng.integers(-16, 17, n)) / 8).astype(F) for _ in range(S - 1)]
    srcs = [(c + x).astype(F) for x in xs]
    assert all(np.array_equal(w - c, x) for w, x in zip(srcs, xs))  # W - c gives the task vectors back exactly
    var32 = R.variance(xs)
    var64 = np.stack([x.astype(np.float64) for x in xs]).var(axis=0)
    assert np.array_equal(var32.astype(np.float64), var64)
    order = np.sort(var64)[::-1]
    K = next(k for k in range(n // 10, n) if order[k - 1] > order[k])
    lam = 0.75
    out, row = R.sce(c, srcs, density=None, lam=lam, keep=K)
    want_d, mask = published(c, srcs, K, lam)
    key = R.keys(var32)
    sel = key >= np.uint32(row["threshold_bits"])
    assert row["kept"] == K == int(mask.sum()) and np.array_equal(sel, mask)
    d, tts, cnt = R.erase(xs, sel, row["weight"])
    assert not np.any(sel & (np.sum(np.stack(xs).astype(np.float64), axis=0) == 0))
    assert row["empty"] == n - K and np.all(want_d[~mask] == 0) and np.all(d[~sel] == 0)
    err = np.abs(d.astype(np.float64) - want_d)
    assert np.all(err <= (4 * S + 4) * 2.0 ** -24 * np.abs(want_d)), float((err / np.maximum(np.abs(want_d), 1e-300)).max())
    assert np.any(d != 0) and row["conflict"] > 0
    assert out.tobytes() == (c + F(lam) * d).astype(F).tobytes()


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_sce_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_sce_plan_bytes", "vlm_sce_plan_upload", "vlm_sce_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert L.SIGNATURES["vlm_sce_plan_bytes"] == L.SIGNATURES["vlm_ties_plan_bytes"]
    assert L.SIGNATURES["vlm_sce_run"] == L.SIGNATURES["vlm_ties_run"]
    assert L.SIGNATURES["vlm_sce_plan_upload"][1][1:] == L.SIGNATURES["vlm_ties_plan_upload"][1][1:]
    assert lib.vlm_abi_version() == 11  # entry points are added, nothing moves


def test_sce_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_sce_job_t": L.SceJob, "vlm_sce_header_t": L.SceHeader, "vlm_sce_result_t": L.SceResult}
    consts = {"VLM_SCE_COUNTERS": L.SCE_COUNTERS}
    lines = ['printf("%s %%d\\n", %s);' % (c, c) for c in consts]
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
    want = {c: str(v) for c, v in consts.items()}
    for cname, ty in types.items():
        want[cname] = str(ctypes.sizeof(ty))
        for field, _ in ty._fields_:
            want[cname + "." + field] = str(getattr(ty, field).offset)
    assert got == want
    assert (ctypes.sizeof(L.SceJob), ctypes.sizeof(L.SceHeader), ctypes.sizeof(L.SceResult)) == (72, 96, 72)
    assert [f for f, _ in L.SceHeader._fields_][:10] == [f for f, _ in L.TiesHeader._fields_]  # the select's header comes first
    assert (ctypes.sizeof(L.TiesJob), ctypes.sizeof(L.TiesHeader), ctypes.sizeof(L.TiesState), ctypes.sizeof(L.BandJob),
            ctypes.sizeof(L.StockJob)) == (96, 80, 16, 136, 64)  # untouched


def test_sce_host_side_argument_checks(pkg):
    """vlm_sce_plan_upload rejects bad jobs before it touches the device: every pointer here is fake."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_sce_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_sce_plan_bytes(1, 4096), lib.vlm_sce_plan_bytes(100, 1 << 24)
    # jobs, results, one 16-KiB histogram per JOB (a TIES plan reserves four); 2^12 chunk entries and 32-byte records
    assert 0 < small < big and big >= 100 * (72 + 72 + 2048 * 8) + (8 + 32) * (1 << 12)
    assert big < lib.vlm_ties_plan_bytes(100, 1 << 24)
    job = L.SceJob()
    job.dst, job.base, job.n_src, job.n_elem, job.k, job.lam = 0x1000, 0x2000, 2, 16, 4, 1.0
    job.src[0], job.src[1] = 0x3000, 0x4000
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_sce_plan_upload((L.SceJob * 1)(j), n, w, nbytes, None)

    assert upload(job) == -3                                 # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(job, w=ctypes.c_void_p(0)) == -1           # no workspace
    assert upload(job, w=ctypes.c_void_p(0x10008)) == -1     # misaligned workspace
    assert upload(job, n=0) == -1                            # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("n_src", -1), ("n_elem", 0), ("dst", 0), ("base", 0), ("dst", 0x1004),
                         ("base", 0x2008), ("k", 0), ("k", 17),
                         ("dst", 0x2000),                    # dst exactly equal to base: five passes read it
                         ("dst", 0x3000), ("dst", 0x4000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0)):  # dst meets an input
        bad = L.SceJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for idx, src in ((1, 0), (1, 0x4004), (0, 0x3008), (0, 0x1010)):
        bad = L.SceJob.from_buffer_copy(bytes(job))
        bad.src[idx] = src
        assert upload(bad) == -1, (idx, src)
    bad = L.SceJob.from_buffer_copy(bytes(job))
    bad.n_elem, bad.dst = 1 << 34, 1 << 60
    assert upload(bad) == -4                                 # VLM_ERR_UNSUPPORTED: the length limit of the family
    # every source count; K = 1 and K = n; inputs that are one another (they are only read); a neighbour that ends where dst begins
    for fields in (dict(n_src=1), dict(n_src=3), dict(n_src=4), dict(k=1), dict(k=16), dict(base=0x3000), dict(dst=0x2040),
                   dict(dst=0x1FC0), dict(n_elem=(1 << 34) - 1, dst=1 << 60)):
        ok = L.SceJob.from_buffer_copy(bytes(job))
        for field, value in fields.items():
            setattr(ok, field, value)
        ok.src[2], ok.src[3] = 0x3000, 0x6000
        assert upload(ok) == -3, fields
    assert lib.vlm_sce_run(ctypes.c_void_p(0), None) == -1


# ------------------------------------------------------------------------------------------------------- the host surface
def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import inspect
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.ScePlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, loss_names={}, sum_lambda=1.0)
    with pytest.raises(L.VlmError):
        merge.sce_merge({}, cfg, central_weight={}, device="cpu")
    for bad in (0.0, -0.1, 1.5, float("nan")):  # before any device work: the device named here does not exist
        with pytest.raises(ValueError):
            merge.sce_merge({}, cfg, central_weight={}, density=bad, device="cuda:99")
    assert merge.ScePlan.PASSES == 5 and merge.ScePlan.HAS_DST
    sig = inspect.signature(merge.sce_merge)
    assert list(sig.parameters) == ["state_dict", "config", "central_weight", "density", "lam", "device", "plan_out", "report_out"]
    assert (sig.parameters["density"].default, sig.parameters["lam"].default) == (0.1, None)
    assert list(inspect.signature(merge.ScePlan.add).parameters) == ["self", "srcs", "base", "density", "lam", "keep", "name"]
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.sce_merge) and vm.ViLTransformerSS.sce_merge.__defaults__ == (0.1, None)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_parses_sce_before_any_device(pkg):
    mc = tool()
    assert "sce" in mc.METHODS
    io = ["--ckpt", "a.ckpt", "--out", "b.ckpt"]
    args, cfg = mc.parse_args(["--method", "sce"] + io + ["--central", "c.ckpt", "--density", "0.05", "--lambda", "0.3", "--report", "r.json",
                                                        "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.central, args.density, args.report) == ("sce", "c.ckpt", 0.05, "r.json")
    assert cfg["sum_lambda"] == 0.3 and cfg["vlffn_start_layer_index"] == 10
    for bad in ("0", "7", "-0.5", "nan"):
        with pytest.raises(ValueError):
            mc.parse_args(["--method", "sce"] + io + ["--density", bad])
    # what the method does not use is not looked at
    args, _ = mc.parse_args(["--method", "sce"] + io + ["--drop", "2", "--epsilon", "9", "--gamma", "3", "--seed", "-1"])
    assert args.method == "sce"
    args, _ = mc.parse_args(["--method", "della"] + io)  # the other methods parse as before
    assert (args.density, args.epsilon) == (0.2, 0.1)
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "sce" in r.stdout and "sce_merge" in r.stdout


# ------------------------------------------------------------------------------------------------------ the build record
def test_sce_kernels_keep_the_occupancy_their_grids_count_on():
    """None of the kernels may spill or use scratch.  SCE_HIST_BLOCKS_PER_CU = 4 counts on four resident histogram workgroups per CU
    (110 to 120 VGPRs; the ONE histogram of an element-keyed pass is 8 KiB of LDS where a per-source pass holds 32 KiB, but the
    registers bound the residency), SCE_REDUCE_BLOCKS_PER_CU = 12 on three rounds of four (114 VGPRs, two buffers of four waves' four
    sums), SCE_APPLY_BLOCKS_PER_CU = 12 on four rounds of three (140 VGPRs), as the TIES apply pass."""
    import test_build_cpu as tb
    if tb._stale():
        import __graft_entry__ as ge
        ge.build()
    with open(tb.RES) as f:
        resources = json.load(f)
    hist = {k: v for k, v in resources.items() if "vlm_select_hist_kernel" in k and "sce_sel" in k}
    scan = {k: v for k, v in resources.items() if "vlm_select_scan_kernel" in k and "sce_sel" in k}
    assert len(hist) == 3 and len(scan) == 3, sorted(k for k in resources if "sce" in k)
    for name, r in hist.items():
        assert r["Occupancy"] == 4 and r["LDS Size"] == 2048 * 4, (name, r)
    found = {}
    for name in ("vlm_sce_reduce_kernel", "vlm_sce_fold_kernel", "vlm_sce_apply_kernel"):
        hit = [v for k, v in resources.items() if name in k]
        assert len(hit) == 1, sorted(k for k in resources if "sce" in k)
        found[name] = hit[0]
    for name, r in list(hist.items()) + list(scan.items()) + list(found.items()):
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    assert found["vlm_sce_reduce_kernel"]["Occupancy"] == 4, found["vlm_sce_reduce_kernel"]
    assert found["vlm_sce_reduce_kernel"]["LDS Size"] == 2 * 4 * 4 * 8
    assert found["vlm_sce_apply_kernel"]["Occupancy"] >= 3, found["vlm_sce_apply_kernel"]
    for sel in ("ties_sel", "band_sel"):  # the per-source instantiations are still there, three passes each
        assert len([k for k in resources if "vlm_select_hist_kernel" in k and sel in k]) == 3, sel
