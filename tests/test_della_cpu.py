"""DELLA merge, host side (no GPU): the numpy restatement of the rule (della_restatement.py) against the definition of the rank
and against the rule's three consequences (epsilon = 0 is DARE, the full window is the task-vector sum, the kept share per rank
decile), della_window, the driver's refusals, merge_ckpt.py's command line, the ABI additions, the tile table and the build's
verdict on the kernel.  The reference has no DELLA: nothing here is pinned to it."""
import ctypes
import importlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dare_restatement as dr
from della_restatement import LINEAR, TIES, della, keep_thresholds, keys, ranks, window
from test_build_cpu import resources  # noqa: F401  (the fixture: brings the build and its resource record up to date)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
SEED, STREAM = 20240617, 5


def rows_with_ties(rows, L, seed):
    """Task vectors with duplicates, zeros (+0.0 and -0.0) and +-x pairs in every row."""
    rng = np.random.default_rng(seed)
    t = (rng.integers(-3, 4, rows * L) / 4).astype(F)  # seven values: duplicates, zeros and +-x pairs for every L > 1
    t[rng.integers(0, 4, rows * L) == 0] = F(-0.0)
    some = rng.integers(0, 3, rows * L) == 0
    t[some] = rng.standard_normal(rows * L).astype(F)[some]
    return t


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("L", [1, 2, 3, 5, 64, 257])
def test_ranks_against_the_definition(L):
    rows = 4
    t = rows_with_ties(rows, L, seed=L)
    got = ranks(t, L).reshape(rows, L)
    k = keys(t).reshape(rows, L).astype(np.int64)
    for r in range(rows):
        for i in range(L):  # O(L^2), straight from the rule
            want = sum(1 for j in range(L) if k[r, j] < k[r, i] or (k[r, j] == k[r, i] and j < i))
            assert int(got[r, i]) == want, (r, i)
        assert sorted(got[r].tolist()) == list(range(L))
    if L >= 5:
        assert len(np.unique(k)) < k.size  # the data does hold equal keys


def test_keep_thresholds_by_hand():
    r = np.arange(5, dtype=np.uint64)
    assert keep_thresholds(r, 5, 10, 30).tolist() == [10, 15, 20, 25, 30]
    assert keep_thresholds(r[:4], 4, 10, 30).tolist() == [10, 16, 23, 30]  # floor(20 r / 3)
    assert keep_thresholds(r[:1], 1, 10, 31).tolist() == [20]
    assert keep_thresholds(np.array([0, 4095], np.uint64), 4096, 1, 2 ** 32).tolist() == [1, 2 ** 32]
    assert keep_thresholds(np.array([2047], np.uint64), 4096, 1, 2 ** 32).tolist() == [1 + (2 ** 32 - 1) * 2047 // 4095]


def inputs(rows, L, S, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(rows * L).astype(F)
    return c, [(c + rows_with_ties(rows, L, seed + 1 + m)).astype(F) for m in range(S)]


@pytest.mark.parametrize("mode", [LINEAR, TIES])
@pytest.mark.parametrize("drop,rescale", [(0.5, True), (0.75, True), (0.9, False)])
def test_epsilon_zero_is_dare(mode, drop, rescale):
    """keep_lo == keep_hi: the ranks drop out.  DARE's bytes and counters wherever float32(1 / (1 - drop)) == 2^32 / float(keep_lo)."""
    kb = dr.keep_below(drop)
    if rescale:
        assert dr.rescale_of(drop) == F(4294967296.0) / F(kb)
    for (rows, L), S in zip(((3, 5), (7, 64), (2, 257), (1, 1)), (2, 3, 4, 1)):
        c, srcs = inputs(rows, L, S, seed=L)
        got, gi = della(c, srcs, L, kb, kb, 0.75, SEED, STREAM, mode, rescale)
        want, wi = dr.dare(c, srcs, drop, 0.75, SEED, STREAM, mode, rescale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (gi["kept"], gi["conflict"], gi["empty"]) == (wi["kept"], wi["conflict"], wi["empty"])


def test_full_window_is_the_plain_sum():
    for (rows, L), S in zip(((3, 5), (7, 64), (2, 257), (1, 1)), (2, 3, 4, 1)):
        c, srcs = inputs(rows, L, S, seed=L)
        got, info = della(c, srcs, L, 2 ** 32, 2 ** 32, 0.75, SEED, STREAM, LINEAR)
        d = np.zeros(c.size, F)
        for w in srcs:
            d = d + (w - c)
        assert np.array_equal(got.view(np.uint32), (c + F(0.75) * d).astype(F).view(np.uint32))
        assert info["kept"] == [c.size] * S and info["empty"] == 0


def test_kept_share_per_rank_decile():
    """Rows of 3 072, 64 rows, N(0, 1) against a zero base, window 0.3 +- 0.2, seed 1, stream 0: the kept share of each rank decile
    lies within 5 binomial standard deviations of the decile's mean keep probability (beyond 5 sigma: under 1e-6 per decile)."""
    rows, L = 64, 3072
    rng = np.random.default_rng(0)
    w = rng.standard_normal(rows * L).astype(F)
    lo, hi = window(0.3, 0.2)
    _, info = della(np.zeros(rows * L, F), [w], L, lo, hi, 1.0, 1, 0, LINEAR)
    r, kept, p = info["ranks"][0], info["masks"][0], info["kb"][0].astype(np.float64) / 2 ** 32
    assert abs(p.min() - 0.1) < 1e-6 and abs(p.max() - 0.5) < 1e-6
    worst = 0.0
    for d in range(10):
        sel = (r * np.uint64(10) // np.uint64(L)) == d
        n, mean = int(sel.sum()), float(p[sel].mean())
        sigma = math.sqrt(float((p[sel] * (1 - p[sel])).sum())) / n
        z = abs(float(kept[sel].mean()) - mean) / sigma
        worst = max(worst, z)
        assert z <= 5.0, (d, z)
    print("worst decile: %.2f sigma" % worst)


def test_restatement_by_hand():
    """One row of four, one source, window [2^30, 2^32]: kb = 2^30 + floor(3 * 2^30 * r / 3) = (r + 1) 2^30, scale = 4 / (r + 1)."""
    c = np.zeros(4, F)
    w = np.array([3.0, -1.0, 2.0, -4.0], F)  # ranks 2, 0, 1, 3
    out, info = della(c, [w], 4, 2 ** 30, 2 ** 32, 1.0, SEED, STREAM, LINEAR)
    assert info["ranks"][0].tolist() == [2, 0, 1, 3] and info["kb"][0].tolist() == [3 * 2 ** 30, 2 ** 30, 2 ** 31, 2 ** 32]
    u = dr.draws(4, 0, STREAM, SEED).astype(np.uint64)
    kept = u < info["kb"][0]
    assert kept[3] and info["masks"][0].tolist() == kept.tolist()
    scale = np.array([F(4) / F(3), 4, 2, 1], F)
    assert out.tolist() == np.where(kept, w * scale, F(0)).astype(F).tolist()
    out2, _ = della(c, [w], 4, 2 ** 30, 2 ** 32, 1.0, SEED, STREAM, LINEAR, rescale=False)
    assert out2.tolist() == np.where(kept, w, F(0)).tolist()


# ------------------------------------------------------------------------------------------------- host code
def test_della_window_values_edges_and_refusals(pkg):
    merge = importlib.import_module("vl_merging_amd.merge")
    assert merge.della_window(0.5, 0.0) == (2 ** 31, 2 ** 31)
    assert merge.della_window(0.5, 0.5 - 2.0 ** -32) == (1, 2 ** 32 - 1)
    assert merge.della_window(1, 0) == merge.della_window(1.0, 0.0) == (2 ** 32, 2 ** 32)
    assert merge.della_window(0.75, 0.25) == (2 ** 31, 2 ** 32)
    assert merge.della_window(0.2, 0.1) == window(0.2, 0.1) == (math.floor((0.2 - 0.1) * 2 ** 32), math.floor((0.2 + 0.1) * 2 ** 32))
    for density, epsilon in ((0.5, 0.5), (0.2, 0.2), (0.2, 0.3), (0.9, 0.2), (0.5, -0.1), (0.0, 0.0), (1.5, 0.0), (2.0 ** -33, 0.0),
                             (float("nan"), 0.1), (0.5, float("nan")), (float("inf"), 0.0), (-0.5, 0.0)):
        with pytest.raises(ValueError):
            merge.della_window(density, epsilon)


def test_della_row_len(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    assert merge.della_row_len(torch.zeros(3072, 768)) == 768 and merge.della_row_len(torch.zeros(768, 3072)) == 3072
    assert merge.della_row_len(torch.zeros(3072)) == 3072 and merge.della_row_len(torch.zeros(2, 3, 5)) == 5
    assert merge.della_row_len(torch.zeros(())) == 1


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.DellaPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.della_merge({}, cfg, central_weight={}, device="cpu")
    for kw in (dict(density=0.2, epsilon=0.2), dict(density=0.9, epsilon=0.2), dict(epsilon=-0.1), dict(density=float("nan")),
               dict(epsilon=float("nan")), dict(density=0.0, epsilon=0.0)):
        with pytest.raises(ValueError):
            merge.della_merge({}, cfg, central_weight={}, **kw)
    with pytest.raises(L.VlmError):
        merge.della_merge({}, cfg, central_weight={}, mode="median")
    with pytest.raises(L.VlmError):
        merge.della_merge({}, cfg, central_weight={}, mode=True)
    assert merge.della_merge.__defaults__[:7] == (None, 0.2, 0.1, "linear", None, 0, True)
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.della_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ------------------------------------------------------------------------------------------------- merge_ckpt.py
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_parses_della_before_any_device(pkg):
    mc = tool()
    io = ["--ckpt", "a.ckpt", "--out", "b.ckpt"]
    args, cfg = mc.parse_args(["--method", "della"] + io + ["--density", "0.4", "--epsilon", "0.3", "--seed", "20240617", "--della-mode",
                                                           "ties", "--no-rescale", "--lambda", "0.75", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.density, args.epsilon, args.seed, args.della_mode, args.rescale) == ("della", 0.4, 0.3, 20240617, "ties", False)
    assert cfg["sum_lambda"] == 0.75 and cfg["vlffn_start_layer_index"] == 10
    args, _ = mc.parse_args(["--method", "della"] + io)
    assert (args.density, args.epsilon, args.seed, args.della_mode, args.rescale) == (0.2, 0.1, 0, "linear", True)  # --density's default stays
    args, _ = mc.parse_args(["--method", "della"] + io + ["--density", "1", "--epsilon", "0"])
    assert (args.density, args.epsilon) == (1.0, 0.0)
    for bad in (["--epsilon", "0.2"], ["--epsilon", "-0.1"], ["--epsilon", "nan"], ["--density", "0.95"], ["--density", "nan"],
                ["--density", "0"], ["--seed", "-1"], ["--seed", str(2 ** 64)]):
        with pytest.raises(ValueError):
            mc.parse_args(["--method", "della"] + io + bad)
    with pytest.raises(SystemExit):
        mc.parse_args(["--method", "della"] + io + ["--della-mode", "median"])
    # the other methods parse as before (an epsilon they do not use is not looked at)
    args, _ = mc.parse_args(["--method", "ties"] + io + ["--density", "0.1", "--epsilon", "7"])
    assert (args.method, args.density) == ("ties", 0.1)
    args, _ = mc.parse_args(["--method", "dare"] + io + ["--drop", "0.5"])
    assert (args.method, args.drop, args.dare_mode, args.rescale) == ("dare", 0.5, "linear", True)
    args, _ = mc.parse_args(["--method", "breadcrumbs"] + io)
    assert (args.density, args.gamma, args.band_mode) == (0.2, 0.01, "linear")
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for word in ("della", "--epsilon", "--della-mode", "--density", "--seed", "--no-rescale"):
        assert word in r.stdout


# ------------------------------------------------------------------------------------------------- ABI
def test_della_struct_layouts_are_the_compilers(pkg, tmp_path):
    """sizeof and the offsets of the ctypes structures against what the host compiler makes of include/vlm_hip.h."""
    L = importlib.import_module("vl_merging_amd._lib")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    types = {"vlm_della_job_t": L.DellaJob, "vlm_della_header_t": L.DellaHeader}
    consts = {"VLM_DELLA_COUNTERS": L.DELLA_COUNTERS, "VLM_DELLA_TIES": L.DELLA_TIES, "VLM_DELLA_LINEAR": L.DELLA_LINEAR,
              "VLM_DELLA_MAX_ROW": L.DELLA_MAX_ROW}
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
    print(r.stdout)
    got = dict(ln.split() for ln in r.stdout.splitlines())
    want = {c: str(v) for c, v in consts.items()}
    for cname, ty in types.items():
        want[cname] = str(ctypes.sizeof(ty))
        for field, _ in ty._fields_:
            want[cname + "." + field] = str(getattr(ty, field).offset)
    assert got == want
    assert (ctypes.sizeof(L.DellaJob), ctypes.sizeof(L.DellaHeader)) == (104, 40)  # what the compiler printed when this was written
    assert (L.DELLA_COUNTERS, L.DELLA_MAX_ROW) == (L.MERGE_MAX_SRC + 2, 4096)
    assert ctypes.sizeof(L.DareJob) == 96 and ctypes.sizeof(L.TiesJob) == 96 and ctypes.sizeof(L.BandJob) == 136  # untouched


def test_della_entry_points_and_host_side_argument_checks(pkg):
    """vlm_della_plan_upload rejects bad jobs before it touches the device: every pointer here is fake."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    for s in ("vlm_della_plan_bytes", "vlm_della_plan_upload", "vlm_della_run"):
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_abi_version() == 11  # entry points are added, nothing moves
    assert lib.vlm_della_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_della_plan_bytes(1, 4096), lib.vlm_della_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (104 + 8 * L.DELLA_COUNTERS) + 8 * (1 << 12)  # jobs, counters, 2^12 tile records
    job = L.DellaJob()
    job.dst, job.base, job.n_src, job.n_elem, job.row_len, job.lam, job.rescale = 0x1000, 0x2000, 2, 16, 4, 1.0, 1
    job.src[0], job.src[1] = 0x3000, 0x4000
    job.keep_lo, job.keep_hi, job.seed, job.stream, job.mode = 2 ** 30, 2 ** 31, 1, 2, L.DELLA_TIES
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=64):
        return lib.vlm_della_plan_upload((L.DellaJob * 1)(j), n, w, nbytes, None)

    assert upload(job) == -3                                 # VLM_ERR_WORKSPACE: every argument check passed
    assert upload(job, w=ctypes.c_void_p(0)) == -1           # no workspace
    assert upload(job, n=0) == -1                            # no jobs
    for field, value in (("n_src", 0), ("n_src", 5), ("dst", 0), ("base", 0), ("dst", 0x1004), ("base", 0x2008), ("n_elem", 0),
                         ("n_elem", 18), ("row_len", 3), ("row_len", 5), ("keep_lo", 0), ("keep_lo", 2 ** 31 + 1), ("keep_hi", 2 ** 32 + 1),
                         ("keep_hi", 2 ** 63), ("mode", 2), ("mode", -1), ("rescale", 2), ("rescale", -1),
                         ("dst", 0x2000), ("dst", 0x3000), ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0)):  # dst meets an input
        bad = L.DellaJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for rl, n in ((0, 16), (4097, 4097), (8192, 8192), (2 ** 32 - 1, 2 ** 32 - 1)):
        bad = L.DellaJob.from_buffer_copy(bytes(job))
        bad.row_len, bad.n_elem = rl, n
        bad.dst = 1 << 40  # far from the inputs whatever the length
        assert upload(bad) == -4, (rl, n)                    # VLM_ERR_UNSUPPORTED
    bad = L.DellaJob.from_buffer_copy(bytes(job))
    bad.src[1] = 0x4004
    assert upload(bad) == -1
    # both ends of the window, both modes, the longest row, one row, one source and four
    for fields in (dict(keep_lo=1), dict(keep_hi=2 ** 32), dict(keep_lo=2 ** 31), dict(keep_lo=2 ** 32, keep_hi=2 ** 32), dict(mode=L.DELLA_LINEAR),
                   dict(rescale=0), dict(row_len=16), dict(row_len=1), dict(n_src=1), dict(n_src=4), dict(row_len=4096, n_elem=8192, dst=0x100000)):
        ok = L.DellaJob.from_buffer_copy(bytes(job))
        for field, value in fields.items():
            setattr(ok, field, value)
        ok.src[2], ok.src[3] = 0x5000, 0x6000
        assert upload(ok) == -3, fields
    assert lib.vlm_della_run(ctypes.c_void_p(0), None) == -1


def test_della_tile_table(tmp_path):
    """csrc/della_tiles.h without HIP, as a stand-alone program under AddressSanitizer + UBSan: the tiles of a job cover every row
    exactly once and in order, no tile exceeds 4 096 elements, and della_tiles_bound bounds the count."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "della_tiles_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "della_tiles_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "della tiles ok" in r.stdout


# ------------------------------------------------------------------------------------------------- the build's verdict
def test_della_kernel_resources(resources):  # noqa: F811
    """The ranks are made in LDS by a workgroup that holds its tile in registers: no scratch, no spilled VGPR, and at most 80 KiB
    of LDS, so that two workgroups share a CU and one tile's loads overlap another's sort."""
    apply_della = [v for k, v in resources.items() if "vlm_della_apply_kernel" in k]
    assert len(apply_della) == 1, sorted(resources)
    r = apply_della[0]
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] <= 81920 and r["Occupancy"] >= 2, r
