"""Expert-pair statistics, host side (no GPU): the numpy restatement of the rule (pairstats_restatement.py) against cases small
enough to check by hand and against math.fsum, the ABI additions, expert_stats.py's command line and the build's record of the
kernels.  The reference has no such measure: nothing here is pinned to it."""
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

import pairstats_restatement as R
from test_ties_cpu import header_text
from test_ties_gpu import planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "expert_stats.py")
F = np.float32


def f32(*v):
    return np.array(v, dtype=F)


def key_of(x):
    return int(f32(x).view(np.uint32)[0] & 0x7FFFFFFF)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_by_hand():
    (p,) = R.pair_stats([f32(1, -1), f32(1, 1)])["pairs"]
    assert (p["ssd"], p["conflict"], p["cosine"], p["live"]) == (0.5, 1, 0.0, 2)
    assert (p["dot"], p["dist2"], p["l2"], p["ssd_sum"], p["conflict_rate"]) == (0.0, 4.0, 2.0, 1.0, 0.5)
    assert (p["tssd_sum"], p["tlive"], p["tconflict"], p["tssd"]) == (1.0, 2, 1, 0.5)  # tkey = 0: everything is in
    # relative to a central tensor: x = [1, -1], y = [1, 1] again
    row = R.pair_stats([f32(3, 1), f32(3, 3)], f32(2, 2))
    assert row["sq"] == [2.0, 2.0] and row["nnz"] == [2, 2] and row["pairs"][0]["ssd"] == 0.5
    # one source: sq and nnz only
    row = R.pair_stats([f32(3, 0, -4)])
    assert row["pairs"] == [] and row["sq"] == [25.0] and row["nnz"] == [2] and row["n"] == 3


def test_signed_zeros_are_neither_live_nor_nonzero():
    row = R.pair_stats([f32(0.0, -0.0, 0.0, 2), f32(-0.0, 0.0, 0.0, -2)])
    (p,) = row["pairs"]
    assert row["nnz"] == [1, 1] and (p["live"], p["conflict"], p["tlive"]) == (1, 1, 1)
    assert p["ssd_sum"] == 0.0 and p["ssd"] == 1.0 and p["cosine"] == -1.0
    # nothing alive: every derived value with a count below it is None, the cosine's zero norm as well
    (p,) = R.pair_stats([f32(0, -0.0), f32(-0.0, 0)])["pairs"]
    assert (p["live"], p["ssd"], p["tssd"], p["conflict_rate"], p["cosine"], p["l2"]) == (0, None, None, None, None, 0.0)
    assert math.copysign(1.0, p["dot"]) == 1.0  # sums start at +0.0: the -0.0 addends here cannot make them -0.0


def test_threshold_at_a_values_own_key_keeps_it():
    x, y = f32(0.5, -0.25, 0.125), f32(0.0625, 0.0625, 0.0625)
    at, above = key_of(0.25), key_of(0.25) + 1
    big = key_of(4.0)
    (p,) = R.pair_stats([x, y], tkeys=[at, big])["pairs"]
    assert p["tlive"] == 2 and p["live"] == 3            # |x| >= 0.25: elements 0 and 1; y is never in
    (p,) = R.pair_stats([x, y], tkeys=[above, big])["pairs"]
    assert p["tlive"] == 1
    (p,) = R.pair_stats([x, y], tkeys=[big, key_of(0.0625)])["pairs"]
    assert p["tlive"] == 3 and p["tssd_sum"] == p["ssd_sum"]  # in_a OR in_b
    (p,) = R.pair_stats([x, y], tkeys=[big, big])["pairs"]
    assert (p["tlive"], p["tssd_sum"], p["tssd"], p["tconflict"]) == (0, 0.0, None, 0)
    assert R.rms_keys({"n": 4, "sq": [4.0, 1.0]}, 0.5) == [key_of(0.5), key_of(0.25)]


def test_the_tree_is_the_stated_one():
    """chunk_records (vectorised) against the tree written out lane by lane for a full chunk, a partial one and a tail, on addends
    spread over 40 binades, where another order of the additions rounds differently."""
    rng = np.random.default_rng(5)
    n = 4096 + 4 * 300 + 3
    term = rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))
    n4 = n // 4
    recs = []
    for ck in range(2):
        lanes = []
        for t in range(256):
            acc = 0.0
            for u in range(4):
                i4 = 1024 * ck + 256 * u + t
                if i4 < n4:
                    for c in range(4):
                        acc = acc + term[4 * i4 + c]
            if ck == 1 and t < (n & 3):
                acc = acc + term[4 * n4 + t]
            lanes.append(acc)
        waves = []
        for w in range(4):
            v = lanes[64 * w: 64 * w + 64]
            for half in (32, 16, 8, 4, 2, 1):
                v = [v[i] + v[i + half] for i in range(half)]
            waves.append(v[0])
        recs.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert R.chunk_records(term[None, :])[0].tolist() == recs
    assert R.ordered_sum(term) == (0.0 + recs[0]) + recs[1]


@pytest.mark.parametrize("n", [4097, 12289, 70001])
def test_every_sum_is_within_the_bound_of_any_summation_order(n):
    """|sum in the rule's order - exact sum| <= n 2^-53 sum |term| (the first-order bound of ANY order of n additions)."""
    S = 3
    c, srcs = planted(n, S, seed=n + S)
    tkeys = R.density_keys(srcs, c, 0.2)
    per_src, per_pair = R.terms(srcs, c, tkeys)
    row = R.pair_stats(srcs, c, tkeys)
    checked = 0
    for got, t in [(row["sq"][m], per_src["sq"][m]) for m in range(S)] + \
                  [(p[k], per_pair[(p["a"], p["b"])][k]) for p in row["pairs"] for k in R.SUMS]:
        assert abs(got - math.fsum(t)) <= n * 2.0 ** -53 * math.fsum(np.abs(t))
        checked += 1
    assert checked == S + 4 * 3
    for p in row["pairs"]:
        for k in R.COUNTS:
            assert p[k] == int(per_pair[(p["a"], p["b"])][k].sum())
        assert 0 < p["tlive"] < p["live"] <= n and 0 < p["tconflict"] < p["conflict"] and p["tssd_sum"] < p["ssd_sum"]
    if n == 4097:
        p = row["pairs"][0]
        assert (p["live"], p["conflict"], p["tlive"]) == (4075, 2346, 1173)


def test_slot_map(pkg):
    L = importlib.import_module("vl_merging_amd._lib")
    seen = []
    for b in range(1, 4):
        for a in range(b):
            assert L.pair_slot(a, b) == R.pair_slot(a, b) == b * (b - 1) // 2 + a
            seen.append(L.pair_slot(a, b))
    assert seen == list(range(6)) == list(range(L.PAIRSTATS_PAIRS))  # the pairs of S sources fill the first S (S - 1) / 2 slots
    for bad in ((1, 1), (2, 1), (0, 4), (-1, 2)):
        with pytest.raises(ValueError):
            L.pair_slot(*bad)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_pairstats_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_pairstats_plan_bytes", "vlm_pairstats_plan_upload", "vlm_pairstats_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert L.SIGNATURES["vlm_pairstats_plan_bytes"] == L.SIGNATURES["vlm_dare_plan_bytes"]
    assert L.SIGNATURES["vlm_pairstats_run"] == L.SIGNATURES["vlm_dare_run"]
    assert L.SIGNATURES["vlm_pairstats_plan_upload"][1][1:] == L.SIGNATURES["vlm_dare_plan_upload"][1][1:]


def test_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_pairstats_job_t": L.PairStatsJob, "vlm_pairstats_header_t": L.PairStatsHeader,
             "vlm_pairstats_result_t": L.PairStatsResult}
    lines = []
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
    want = {}
    for cname, ty in types.items():
        want[cname] = str(ctypes.sizeof(ty))
        for field, _ in ty._fields_:
            want[cname + "." + field] = str(getattr(ty, field).offset)
    assert got == want
    assert (ctypes.sizeof(L.PairStatsJob), ctypes.sizeof(L.PairStatsHeader), ctypes.sizeof(L.PairStatsResult)) == (72, 56, 448)
    assert ctypes.sizeof(L.DareJob) == 96 and ctypes.sizeof(L.TiesJob) == 96 and ctypes.sizeof(L.MergeJob) == 80  # untouched


def test_pairstats_host_side_argument_checks(pkg):
    """vlm_pairstats_plan_upload rejects bad jobs before it touches the device."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_pairstats_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_pairstats_plan_bytes(1, 4096), lib.vlm_pairstats_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (72 + 448) + (8 + 448) * (1 << 12)  # jobs, results; 2^12 chunk entries and records
    job = L.PairStatsJob()
    job.base, job.n_src, job.n_elem = 0x2000, 2, 16
    job.src[0], job.src[1] = 0x3000, 0x4000
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_pairstats_plan_upload((L.PairStatsJob * 1)(j), n, w, nbytes, None)

    assert upload(job) == -3                                 # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(job, w=ctypes.c_void_p(0)) == -1           # no workspace
    assert upload(job, w=ctypes.c_void_p(0x10008)) == -1     # misaligned workspace
    assert upload(job, n=0) == -1                            # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("n_src", -1), ("base", 0x2008), ("n_elem", 0)):
        bad = L.PairStatsJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for idx, src in ((1, 0), (1, 0x4004), (0, 0x3008)):
        bad = L.PairStatsJob.from_buffer_copy(bytes(job))
        bad.src[idx] = src
        assert upload(bad) == -1, (idx, src)
    bad = L.PairStatsJob.from_buffer_copy(bytes(job))
    bad.n_elem = 1 << 34
    assert upload(bad) == -4                                 # VLM_ERR_UNSUPPORTED: the length limit of the family
    # no base, inputs that are one another (nothing is written, so nothing can overlap), every source count, any keys
    for field, value in (("base", 0), ("base", 0x3000), ("n_src", 1), ("n_src", 3), ("n_src", 4), ("n_elem", (1 << 34) - 1)):
        ok = L.PairStatsJob.from_buffer_copy(bytes(job))
        setattr(ok, field, value)
        ok.src[2], ok.src[3] = 0x3000, 0x6000
        ok.tkey[0], ok.tkey[3] = 0xFFFFFFFF, 0x7F800000
        assert upload(ok) == -3, (field, value)
    assert lib.vlm_pairstats_run(ctypes.c_void_p(0), None) == -1


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.PairStatsPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.expert_stats({}, cfg, central_weight={}, device="cpu")
    with pytest.raises(L.VlmError):
        merge.expert_stats({}, cfg, raw=True, device="cpu")
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            merge.expert_stats({}, cfg, central_weight={}, trunc_rms=bad)
    p = dict(sq_a=4.0, sq_b=9.0, dot=3.0, dist2=16.0, ssd_sum=1.5, tssd_sum=0.5, live=6, tlive=0, conflict=3, tconflict=0)
    assert merge.pair_derived(p) == R.derived(p) == {"l2": 4.0, "cosine": 0.5, "ssd": 0.75, "tssd": None, "conflict_rate": 0.5}
    assert merge.rms_tkeys({"n": 4, "sq": [4.0, 1.0]}, 0.5) == R.rms_keys({"n": 4, "sq": [4.0, 1.0]}, 0.5)
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.expert_stats)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ------------------------------------------------------------------------------------------------------ expert_stats.py
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("expert_stats")
    finally:
        sys.path.pop(0)


def test_expert_stats_command_line(pkg):
    es = tool()
    args, cfg = es.parse_args(["--ckpt", "a.ckpt", "--central", "c.ckpt", "--trunc-rms", "1.5", "--report", "r.json", "with",
                               "vlffn_start_layer_index=10"])
    assert (args.ckpt, args.central, args.raw, args.trunc_rms, args.report) == ("a.ckpt", "c.ckpt", False, 1.5, "r.json")
    assert cfg["vlffn_start_layer_index"] == 10
    args, _ = es.parse_args(["--ckpt", "a", "--raw", "--report", "r"])
    assert (args.central, args.raw, args.trunc_rms) == (None, True, None)
    for bad in (["--trunc-rms", "0"], ["--trunc-rms", "-1"], ["--trunc-rms", "nan"], ["--trunc-rms", "inf"]):
        with pytest.raises(ValueError):
            es.parse_args(["--ckpt", "a", "--report", "r"] + bad)
    for bad in (["--ckpt", "a"], ["--report", "r"], ["--ckpt", "a", "--report", "r", "--raw", "--central", "c"],
                ["--ckpt", "a", "--report", "r", "--out", "b"]):  # it writes no checkpoint
        with pytest.raises(SystemExit):
            es.parse_args(bad)
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for word in ("--ckpt", "--central", "--raw", "--trunc-rms", "--report"):
        assert word in r.stdout


# ------------------------------------------------------------------------------------------------------ the build record
def test_pairstats_kernels_keep_the_occupancy_their_grid_counts_on():
    """The streaming kernel's grid is sized from two resident workgroups per CU; it is an HBM stream and may not spill."""
    import test_build_cpu as tb
    if tb._stale():
        import __graft_entry__ as ge
        ge.build()
    with open(tb.RES) as f:
        resources = json.load(f)
    stream = [v for k, v in resources.items() if "vlm_pairstats_stream_kernel" in k]
    fold = [v for k, v in resources.items() if "vlm_pairstats_fold_kernel" in k]
    assert len(stream) == 1 and len(fold) == 1, sorted(k for k in resources if "pairstats" in k)
    for r in stream + fold:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Occupancy"] >= 2, r
    for name in ("vlm_merge_kernel", "vlm_ties_apply_kernel", "vlm_dare_apply_kernel"):  # the family's lookups still find one each
        assert len([k for k in resources if name in k]) == 1, name
