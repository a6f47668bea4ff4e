"""Model Stock, host side (no GPU): the restatement of the rule (stock_restatement.py) against cases worked out by hand and
against the identity t * mean(W) + (1 - t) * c, the ABI additions, the host surface, merge_ckpt.py's command line and the build's
record of the three kernels.  The reference has no Model Stock: nothing here is pinned to it."""
import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import stock_restatement as R
from test_ties_cpu import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32


def f32(*v):
    return np.array(v, dtype=F)


def aligned(n, S, seed):
    """Experts that share a component: W_m = c + 0.5 g + noise_m with g ~ 0.1 N(0, 1) shared and noise_m ~ 0.05 N(0, 1): the mean
    pairwise cosine of the task vectors is about 0.5 (between 0.49 and 0.52 for every n >= 1023 and S in 2 .. 4)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(n).astype(F)
    g = (rng.standard_normal(n) * 0.1).astype(F)
    srcs = [(c + F(0.5) * g + (rng.standard_normal(n) * 0.05).astype(F)).astype(F) for _ in range(S)]
    return c, srcs


# ------------------------------------------------------------------------------------------------------- the restatement
def test_identical_sources_keep_their_average():
    c = f32(0.5, -1.25, 3.0, 0.0, 7.0)
    w = f32(1.5, -0.25, 2.0, 0.125, 7.0)
    out, row = R.stock(c, [w, w.copy()])
    assert (row["cos"], row["t"], row["scale"]) == (1.0, 1.0, 0.5)
    assert row["pairs"] == [{"a": 0, "b": 1, "dot": row["sq"][0], "cosine": 1.0}] and row["sq"][0] == row["sq"][1]
    assert out.tolist() == w.tolist()  # c + 0.5 * (2 x): exact on these dyadic values
    out, row = R.stock(c, [w, w.copy(), w.copy()])
    assert (row["cos"], row["t"]) == (1.0, 1.0) and [p["cosine"] for p in row["pairs"]] == [1.0] * 3
    assert row["scale"] == float(F(1 / 3)) and row["scale_bits"] == int(F(1 / 3).view(np.uint32))


def test_disjoint_supports_give_the_central_tensor_back():
    c = f32(0.5, -1.25, 3.0, 0.0, 7.0, 1e-3)
    w0, w1 = c.copy(), c.copy()
    w0[:3] += f32(1, -2, 0.5)
    w1[3:] += f32(4, 0.25, 1)
    out, row = R.stock(c, [w0, w1])
    assert (row["cos"], row["t"], row["scale"], row["scale_bits"]) == (0.0, 0.0, 0.0, 0)
    assert row["pairs"][0]["dot"] == 0.0 and row["sq"][0] > 0 and row["sq"][1] > 0
    assert out.tobytes() == c.tobytes()  # c holds no -0.0: c + (+-0.0) is c


def test_opposite_task_vectors_hit_the_clamp():
    c = f32(1, 2, 3, 4)
    x = f32(0.5, -0.25, 2, 0.125)
    out, row = R.stock(c, [c + x, c - x])
    assert (row["pairs"][0]["cosine"], row["cos"], row["t"], row["scale"]) == (-1.0, -1.0, 0.0, 0.0)
    assert out.tobytes() == c.tobytes()
    # three sources, two of them opposite and the third across both: a negative mean is clamped too
    out, row = R.stock(c, [c + x, c - x, c - x])
    assert [p["cosine"] for p in row["pairs"]] == [-1.0, -1.0, 1.0] and row["cos"] == (-1.0 + -1.0 + 1.0) / 3 and row["t"] == 0.0


def test_a_zero_task_vector_has_cosine_plus_zero():
    import math
    c = f32(1, 2, 3, 4)
    x = f32(0.5, -0.25, 2, 0.125)
    out, row = R.stock(c, [c.copy(), c + x])
    p = row["pairs"][0]
    assert row["sq"][0] == 0.0 and (p["dot"], p["cosine"], row["cos"], row["t"]) == (0.0, 0.0, 0.0, 0.0)
    assert math.copysign(1.0, p["cosine"]) == 1.0 and math.copysign(1.0, row["cos"]) == 1.0
    out, row = R.stock(c, [c + x, c.copy(), c + x])  # pairs (0,1) and (1,2) have den == 0, pair (0,2) is 1
    assert [q["cosine"] for q in row["pairs"]] == [0.0, 1.0, 0.0] and row["cos"] == 1.0 / 3
    cc = 1.0 / 3
    assert row["t"] == (3 * cc) / (1 + 2 * cc)


def test_one_source_is_taken_whole():
    c = f32(1, 2, 3)
    w = f32(1.5, -4, 3)
    out, row = R.stock(c, [w])
    assert row["pairs"] == [] and (row["cos"], row["t"], row["scale"], row["n"]) == (0.0, 1.0, 1.0, 3)
    assert row["sq"] == [0.25 + 36.0 + 0.0] and out.tolist() == w.tolist()


def test_cosine_three_fifths_by_hand():
    """x_0 = (1, 0), x_1 = (3, 4): sq = 1, 25; dot = 3; den = sqrt(25) = 5; cos = 3 / 5; t = 2 cos / (1 + cos)."""
    c = f32(2, -1)
    out, row = R.stock(c, [c + f32(1, 0), c + f32(3, 4)])
    assert row["sq"] == [1.0, 25.0] and row["pairs"] == [{"a": 0, "b": 1, "dot": 3.0, "cosine": 0.6}]
    assert row["cos"] == 0.6 == 3.0 / 5.0
    assert row["t"] == 1.2 / 1.6 == (2 * 0.6) / (1 + 0.6)
    assert row["t"] == 0.7499999999999999  # python's 1.2 / 1.6: one ulp under 3 / 4, and so must the device's be
    assert row["scale"] == float(F((1.2 / 1.6) / 2)) == 0.375
    d = f32(4, 4)  # (1, 0) + (3, 4)
    assert out.tobytes() == (c + F(row["scale"]) * d).astype(F).tobytes()


@pytest.mark.parametrize("n,S", [(1023, 2), (4097, 3), (12289, 4)])
def test_identity_with_the_papers_form(n, S):
    """dst is t * mean(W) + (1 - t) * c: the float64 evaluation of that form against the restatement's fp32 output.  With M the
    largest operand magnitude at an element: the S subtractions err by at most 2^-24 2M each and reach dst scaled by 1 / S (2M
    together), the S - 1 additions of d by 2^-24 2SM each (at most 6M after the scale), the rounding of scale, the product and the
    last addition by 2M, 2M and 3M: under 15 M 2^-24, so 8 M 2^-23 bounds it.  A sanity check of the identity, not of a kernel."""
    c, srcs = aligned(n, S, seed=n + S)
    out, row = R.stock(c, srcs)
    assert 0.05 < row["cos"] < 0.95 and 0.49 <= row["cos"] <= 0.52
    t = row["t"]
    mean = sum(w.astype(np.float64) for w in srcs) / S
    want = t * mean + (1 - t) * c.astype(np.float64)
    M = np.max(np.abs(np.stack([c] + srcs)), axis=0).astype(np.float64)
    assert np.all(np.abs(out.astype(np.float64) - want) <= 8 * M * 2.0 ** -23)
    assert 0.0 < t < 1.0 and np.any(out != c)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_stock_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_stock_plan_bytes", "vlm_stock_plan_upload", "vlm_stock_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert L.SIGNATURES["vlm_stock_plan_bytes"] == L.SIGNATURES["vlm_dare_plan_bytes"]
    assert L.SIGNATURES["vlm_stock_run"] == L.SIGNATURES["vlm_dare_run"]
    assert L.SIGNATURES["vlm_stock_plan_upload"][1][1:] == L.SIGNATURES["vlm_dare_plan_upload"][1][1:]
    assert lib.vlm_abi_version() == 11  # entry points are added, nothing moves


def test_stock_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_stock_job_t": L.StockJob, "vlm_stock_header_t": L.StockHeader, "vlm_stock_result_t": L.StockResult}
    consts = {"VLM_STOCK_SUMS": L.STOCK_SUMS}
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
    assert (ctypes.sizeof(L.StockJob), ctypes.sizeof(L.StockHeader), ctypes.sizeof(L.StockResult)) == (64, 56, 152)
    assert L.STOCK_SUMS == 10 and L.StockResult.cos_pair.offset == 8 * L.STOCK_SUMS  # a result begins as a record does
    assert ctypes.sizeof(L.PairStatsJob) == 72 and ctypes.sizeof(L.PairStatsResult) == 448 and ctypes.sizeof(L.DareJob) == 96  # untouched


def test_stock_host_side_argument_checks(pkg):
    """vlm_stock_plan_upload rejects bad jobs before it touches the device: every pointer here is fake."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_stock_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_stock_plan_bytes(1, 4096), lib.vlm_stock_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (64 + 152) + (8 + 80) * (1 << 12)  # jobs, results; 2^12 chunk entries and records
    job = L.StockJob()
    job.dst, job.base, job.n_src, job.n_elem = 0x1000, 0x2000, 2, 16
    job.src[0], job.src[1] = 0x3000, 0x4000
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_stock_plan_upload((L.StockJob * 1)(j), n, w, nbytes, None)

    assert upload(job) == -3                                 # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(job, w=ctypes.c_void_p(0)) == -1           # no workspace
    assert upload(job, w=ctypes.c_void_p(0x10008)) == -1     # misaligned workspace
    assert upload(job, n=0) == -1                            # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("n_src", -1), ("n_elem", 0), ("dst", 0), ("base", 0), ("dst", 0x1004),
                         ("base", 0x2008),
                         ("dst", 0x2000),                    # dst exactly equal to base: two passes read it
                         ("dst", 0x3000), ("dst", 0x4000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0)):  # dst meets an input
        bad = L.StockJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for idx, src in ((1, 0), (1, 0x4004), (0, 0x3008), (0, 0x1010)):
        bad = L.StockJob.from_buffer_copy(bytes(job))
        bad.src[idx] = src
        assert upload(bad) == -1, (idx, src)
    bad = L.StockJob.from_buffer_copy(bytes(job))
    bad.n_elem, bad.dst = 1 << 34, 1 << 60
    assert upload(bad) == -4                                 # VLM_ERR_UNSUPPORTED: the length limit of the family
    # every source count; inputs that are one another (they are only read); a neighbour that ends where dst begins
    for fields in (dict(n_src=1), dict(n_src=3), dict(n_src=4), dict(base=0x3000), dict(dst=0x2040), dict(dst=0x1FC0),
                   dict(n_elem=(1 << 34) - 1, dst=1 << 60)):
        ok = L.StockJob.from_buffer_copy(bytes(job))
        for field, value in fields.items():
            setattr(ok, field, value)
        ok.src[2], ok.src[3] = 0x3000, 0x6000
        assert upload(ok) == -3, fields
    assert lib.vlm_stock_run(ctypes.c_void_p(0), None) == -1


# ------------------------------------------------------------------------------------------------------- the host surface
def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.StockPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, loss_names={})  # no sum_lambda: it is not read
    with pytest.raises(L.VlmError):
        merge.stock_merge({}, cfg, central_weight={}, device="cpu")
    assert merge.StockPlan.PASSES == 2 and merge.StockPlan.HAS_DST
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.stock_merge) and vm.ViLTransformerSS.stock_merge.__defaults__ is None
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_parses_stock_before_any_device(pkg):
    mc = tool()
    assert "stock" in mc.METHODS
    io = ["--ckpt", "a.ckpt", "--out", "b.ckpt"]
    args, cfg = mc.parse_args(["--method", "stock"] + io + ["--central", "c.ckpt", "--report", "r.json", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.central, args.report) == ("stock", "c.ckpt", "r.json") and cfg["vlffn_start_layer_index"] == 10
    # what the method does not use is not looked at, as for interp: values another method refuses parse here
    args, _ = mc.parse_args(["--method", "stock"] + io + ["--density", "7", "--drop", "2", "--epsilon", "9", "--gamma", "3", "--seed", "-1"])
    assert args.method == "stock"
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "ties"] + io + ["--density", "7"])  # the other methods parse as before
    args, _ = mc.parse_args(["--method", "della"] + io)
    assert (args.density, args.epsilon) == (0.2, 0.1)
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "stock" in r.stdout and "stock_merge" in r.stdout


# ------------------------------------------------------------------------------------------------------ the build record
def test_stock_kernels_keep_the_occupancy_their_grids_count_on():
    """None of the three may spill or use scratch.  The reducer's grid (12 workgroups per CU) counts on three resident workgroups
    per CU, four rounds of them -- the build gives 132 VGPRs, occupancy 3 --, the apply pass's (96 per CU, a chunk or a few per
    workgroup) on at least the four that the family's apply kernels have: 90 VGPRs, occupancy 5.  The fold is a 64-thread workgroup
    per job: 45 VGPRs."""
    import test_build_cpu as tb
    if tb._stale():
        import __graft_entry__ as ge
        ge.build()
    with open(tb.RES) as f:
        resources = json.load(f)
    found = {}
    for name in ("vlm_stock_reduce_kernel", "vlm_stock_fold_kernel", "vlm_stock_apply_kernel"):
        hit = [v for k, v in resources.items() if name in k]
        assert len(hit) == 1, sorted(k for k in resources if "stock" in k)
        found[name] = hit[0]
        assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0, (name, hit[0])
    assert found["vlm_stock_reduce_kernel"]["Occupancy"] >= 3, found["vlm_stock_reduce_kernel"]
    assert found["vlm_stock_apply_kernel"]["Occupancy"] >= 4, found["vlm_stock_apply_kernel"]
    assert found["vlm_stock_reduce_kernel"]["LDS Size"] == 2 * 4 * 10 * 8  # two buffers of four waves' ten sums
    for name in ("vlm_merge_kernel", "vlm_ties_apply_kernel", "vlm_dare_apply_kernel", "vlm_band_apply_kernel", "vlm_della_apply_kernel",
                 "vlm_pairstats_stream_kernel"):  # the family's lookups still find one each
        assert len([k for k in resources if name in k]) == 1, name
