"""DARE merge, host side (no GPU): csrc/philox.h compiled with the host compiler against the numpy restatement of the rule
(dare_restatement.py) and the known answers, the statistics of the mask, dare_keep_below, the ABI additions and merge_ckpt.py's
command line.  The reference has no DARE: nothing here is pinned to it."""
import ctypes
import importlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from dare_restatement import LINEAR, TIES, dare, draws, keep_below, philox4x32_10, rescale_of
from test_ties_cpu import header_struct_size, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
SEED, STREAM = 20231106, 5

KNOWN = [  # (counter, key, output): Philox4x32-10
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_restatement_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join("%08x" % int(w) for w in philox4x32_10(counter, key)) == want


def test_philox_header_on_the_host_matches_the_restatement(tmp_path):
    """csrc/philox.h without HIP, as a stand-alone program under AddressSanitizer + UBSan: the three known answers, and the draw of
    (i, m, stream, seed) for coordinates that exercise every word of a block, every counter word and both key halves."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "philox_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "philox_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    coords = [(0, 0, 0, 0), (1, 0, STREAM, SEED), (2, 1, STREAM, SEED), (3, 2, STREAM, SEED), (4, 3, STREAM, SEED),
              (4097, 1, 155, 1), (12288, 2, 13 * 11 + 12, 2 ** 32), ((1 << 34) - 1, 3, 2 ** 32 - 1, 2 ** 64 - 1),
              (1 << 20, 0, 7, 0x0123456789ABCDEF), (6, 1, 7, 0x0123456789ABCDEF)]
    r = subprocess.run([exe] + ["%d:%d:%d:%d" % c for c in coords], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.split("\n")
    assert lines[:3] == ["kat " + want for _, _, want in KNOWN]
    got = [int(ln.split()[1]) for ln in lines[3:] if ln.startswith("draw ")]
    want = []
    for i, m, stream, seed in coords:
        w = philox4x32_10([i >> 2, 0, m, stream], (seed & 0xFFFFFFFF, seed >> 32))
        want.append(int(w[i & 3]))
        if i < (1 << 21):
            assert int(draws(i + 1, m, stream, seed)[i]) == want[-1]  # the array form the kernel is compared against
    assert got == want


def test_known_kept_counts():
    kb = math.floor(0.1 * 2 ** 32)
    for n, want in ((4096, [421, 415, 401]), (1 << 20, [105010, 105270, 105458])):
        assert [int((draws(n, m, STREAM, SEED).astype(np.uint64) < np.uint64(kb)).sum()) for m in range(3)] == want


@pytest.mark.parametrize("drop", [0.1, 0.5, 0.9])
def test_kept_count_is_binomial(drop):
    """A check on the generator's wiring (the counter layout, the key, the compare), not a tolerance on the kernel: the kept count
    of n = 2^20 draws lies within 5 sigma of n q, q = keep_below / 2^32."""
    n = 1 << 20
    q = keep_below(drop) / 2 ** 32
    for m in range(3):
        kept = int((draws(n, m, STREAM, SEED).astype(np.uint64) < np.uint64(keep_below(drop))).sum())
        assert abs(kept - n * q) <= 5 * math.sqrt(n * q * (1 - q)), (drop, m, kept)


def test_masks_of_different_coordinates_differ():
    n = 4096
    a = draws(n, 0, STREAM, SEED)
    assert not np.array_equal(a, draws(n, 1, STREAM, SEED))
    assert not np.array_equal(a, draws(n, 0, STREAM + 1, SEED))
    assert not np.array_equal(a, draws(n, 0, STREAM, SEED + 1))
    assert not np.array_equal(a, draws(n, 0, STREAM, SEED + 2 ** 32))  # the key's high word
    assert np.array_equal(a[:1023], draws(1023, 0, STREAM, SEED))     # a draw does not depend on the tensor's length


def test_restatement_by_hand():
    """drop = 0 keeps everything with rescale 1: LINEAR is c + lam * (t_0 + t_1); TIES elects the sign of the sum."""
    c = np.array([1, 1, 1, 1], F)
    srcs = [np.array([3, 1.5, 1, 0], F), np.array([-1, 1.5, 3, 3], F)]  # t_0 = [2, .5, 0, -1], t_1 = [-2, .5, 2, 2]
    out, info = dare(c, srcs, 0.0, 0.5, SEED, STREAM, LINEAR)
    assert out.tolist() == [1, 1.5, 2, 1.5] and info["kept"] == [4, 4] and info["empty"] == 0 and info["conflict"] == 2
    out, info = dare(c, srcs, 0.0, 0.5, SEED, STREAM, TIES)
    assert out.tolist() == [1, 1.25, 2, 2] and info["kept"] == [4, 4] and info["empty"] == 1 and info["conflict"] == 2
    # drop = 0.5 doubles the survivors; without rescaling they stay as they are
    out, info = dare(c, srcs, 0.5, 1, SEED, STREAM, LINEAR)
    m0, m1 = info["masks"]
    t0, t1 = srcs[0] - c, srcs[1] - c
    assert out.tolist() == (c + (np.where(m0, 2 * t0, 0) + np.where(m1, 2 * t1, 0))).tolist()
    assert info["empty"] == int((~m0 & ~m1).sum()) and info["keep_below"] == 2 ** 31
    out2, _ = dare(c, srcs, 0.5, 1, SEED, STREAM, LINEAR, rescale=False)
    assert out2.tolist() == (c + (np.where(m0, t0, 0) + np.where(m1, t1, 0))).tolist()
    assert rescale_of(0.9) == F(1.0 / (1.0 - 0.9)) and rescale_of(0.9, False) == 1.0


# ---------------------------------------------------------------------------------------------------------------- host code
def test_dare_keep_below_edges(pkg):
    merge = importlib.import_module("vl_merging_amd.merge")
    assert merge.dare_keep_below(0) == merge.dare_keep_below(0.0) == 2 ** 32
    assert merge.dare_keep_below(0.5) == 2 ** 31
    assert merge.dare_keep_below(0.9) == keep_below(0.9) == math.floor((1.0 - 0.9) * 2 ** 32)
    assert merge.dare_keep_below(1 - 2.0 ** -32) == 1
    for bad in (1, 1.0, -0.1, -1e-300, 1.5, float("nan"), float("inf"), 1 - 2.0 ** -33):
        with pytest.raises(ValueError):
            merge.dare_keep_below(bad)
    assert np.float32(merge.dare_rescale(0.9)).tobytes() == rescale_of(0.9).tobytes()
    assert merge.dare_rescale(0.9, False) == 1.0 and merge.dare_rescale(0.0) == 1.0
    # 13 names per layer; the stream of a name does not depend on a checkpoint
    assert merge.dare_stream("transformer.blocks.0.attn.qkv.weight") == 0
    assert merge.dare_stream("transformer.blocks.11.norm2.bias") == 13 * 11 + 12
    assert sorted(merge._DARE_STREAM.values()) == list(range(12 * 13))


def test_dare_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    import re
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_dare_plan_bytes", "vlm_dare_plan_upload", "vlm_dare_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_abi_version() == 11
    assert ctypes.sizeof(L.DareJob) == header_struct_size("vlm_dare_job_t") == 96
    assert ctypes.sizeof(L.DareHeader) == header_struct_size("vlm_dare_header_t") == 40
    assert L.DARE_COUNTERS == L.MERGE_MAX_SRC + 2 and "VLM_DARE_COUNTERS (VLM_MERGE_MAX_SRC + 2)" in txt
    assert (L.DARE_LINEAR, L.DARE_TIES) == (0, 1) and "VLM_DARE_LINEAR 0" in txt and "VLM_DARE_TIES 1" in txt
    assert ctypes.sizeof(L.TiesJob) == 96 and ctypes.sizeof(L.MergeJob) == 80  # the existing job structs are untouched


def test_dare_host_side_argument_checks(pkg):
    """vlm_dare_plan_upload rejects bad jobs before it touches the device."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_dare_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_dare_plan_bytes(1, 4096), lib.vlm_dare_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (96 + 8 * L.DARE_COUNTERS) + 8 * (1 << 12)  # jobs, counters, 2^12 chunk records
    job = L.DareJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam, job.rescale = 0x1000, 0x2000, 2, 16, 1.0, 2.0
    job.src[0], job.src[1] = 0x3000, 0x4000
    job.keep_below, job.seed, job.stream, job.mode = 2 ** 31, 1, 2, L.DARE_TIES
    ws = ctypes.c_void_p(0x10000)

    def upload(j, n=1, w=ws, nbytes=small):
        return lib.vlm_dare_plan_upload((L.DareJob * 1)(j), n, w, nbytes, None)

    assert upload(job, w=ctypes.c_void_p(0)) == -1          # no workspace
    assert upload(job, n=0) == -1                            # no jobs
    assert upload(job, nbytes=64) == -3                      # VLM_ERR_WORKSPACE: every argument check passed
    for field, value in (("n_src", 0), ("n_src", 5), ("dst", 0), ("base", 0), ("dst", 0x1004), ("base", 0x2008), ("n_elem", 0),
                         ("dst", 0x2010), ("dst", 0x1FF0), ("dst", 0x3FF0), ("dst", 0x4010),  # partial overlap with an input
                         ("mode", 2), ("mode", -1), ("keep_below", 0), ("keep_below", 2 ** 32 + 1), ("keep_below", 2 ** 63)):
        bad = L.DareJob.from_buffer_copy(bytes(job))
        setattr(bad, field, value)
        assert upload(bad) == -1, (field, value)
    for idx, src in ((1, 0), (1, 0x4004)):
        bad = L.DareJob.from_buffer_copy(bytes(job))
        bad.src[idx] = src
        assert upload(bad) == -1, (idx, src)
    # dst exactly base or exactly a source is allowed; so are both ends of keep_below and both modes
    for field, value in (("dst", 0x2000), ("dst", 0x3000), ("dst", 0x4000), ("keep_below", 1), ("keep_below", 2 ** 32),
                         ("mode", L.DARE_LINEAR), ("n_src", 1), ("n_src", 4)):
        ok = L.DareJob.from_buffer_copy(bytes(job))
        setattr(ok, field, value)
        ok.src[2], ok.src[3] = 0x5000, 0x6000
        assert upload(ok, nbytes=64) == -3, (field, value)
    assert lib.vlm_dare_run(ctypes.c_void_p(0), None) == -1


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.DarePlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.dare_merge({}, cfg, central_weight={}, device="cpu")
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            merge.dare_merge({}, cfg, central_weight={}, drop=bad)
    with pytest.raises(L.VlmError):
        merge.dare_merge({}, cfg, central_weight={}, mode="median")
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.dare_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ----------------------------------------------------------------------------------------------- merge_ckpt.py
def tool():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_merge_ckpt_accepts_the_dare_options(pkg):
    mc = tool()
    args, cfg = mc.parse_args(["--method", "dare", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--drop", "0.7", "--seed", "20231106",
                               "--dare-mode", "ties", "--no-rescale", "--lambda", "0.75", "--report", "r.json", "with",
                               "vlffn_start_layer_index=10"])
    assert (args.method, args.drop, args.seed, args.dare_mode, args.rescale) == ("dare", 0.7, 20231106, "ties", False)
    assert cfg["sum_lambda"] == 0.75 and cfg["vlffn_start_layer_index"] == 10
    args, _ = mc.parse_args(["--method", "dare", "--ckpt", "a", "--out", "b"])
    assert (args.drop, args.seed, args.dare_mode, args.rescale) == (0.9, 0, "linear", True)
    args, _ = mc.parse_args(["--method", "dare", "--ckpt", "a", "--out", "b", "--drop", "0"])
    assert args.drop == 0.0
    for bad in (["--drop", "1"], ["--drop", "-0.5"], ["--drop", "nan"], ["--seed", "-1"]):
        with pytest.raises(ValueError):
            mc.parse_args(["--method", "dare", "--ckpt", "a", "--out", "b"] + bad)
    with pytest.raises(SystemExit):
        mc.parse_args(["--method", "dare", "--ckpt", "a", "--out", "b", "--dare-mode", "median"])
    # the other methods are as they were
    args, _ = mc.parse_args(["--method", "ties", "--ckpt", "a", "--out", "b", "--density", "0.1"])
    assert args.method == "ties" and args.density == 0.1
    r = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for word in ("dare", "--drop", "--seed", "--dare-mode", "--no-rescale"):
        assert word in r.stdout
