"""Consensus merge with TALL masks, host side (no GPU): the numpy restatement of the rule (tall_restatement.py) by hand,
tall_threshold / consensus_k, the ABI additions, the upload checks that need no device, csrc/tall_mask.h compiled with the host
compiler under AddressSanitizer + UBSan, and the command lines.  The reference has no such merge: nothing here is pinned to it."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tall_restatement import consensus, pack, restore, unpack
from test_ties_cpu import header_struct_size, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
RESTORE_TOOL = os.path.join(ROOT, "vl-merging_amd", "tall_restore.py")
F = np.float32


def test_restatement_by_hand():
    """c = 0; x_0 = [4, 1, 0, 1], x_1 = [1, 1, 0, -3]; d = [5, 2, 0, -2].  With tall_lambda = 0.5: expert 0 keeps where
    |x_0| >= 0.5 |x_1|: [4 >= .5, 1 >= .5, 0 >= 0, 1 >= 1.5] = [1, 1, 1, 0]; expert 1 where |x_1| >= 0.5 |x_0|:
    [1 >= 2, 1 >= .5, 0 >= 0, 3 >= .5] = [0, 1, 1, 1].  Votes [1, 2, 2, 1]."""
    c = np.zeros(4, F)
    srcs = [np.array([4, 1, 0, 1], F), np.array([1, 1, 0, -3], F)]
    out, info = consensus(c, srcs, 0.5, 2, 0.5)
    assert [k.tolist() for k in info["keep"]] == [[True, True, True, False], [False, True, True, True]]
    assert out.tolist() == [0, 1, 0, 0] and info["kept"] == [3, 3] and info["selected"] == 2 and info["empty"] == 0
    assert [int(w[0]) for w in info["words"]] == [0b0111, 0b1110] and all(w.size == 1 and w.dtype == np.dtype("<u4") for w in info["words"])
    out, info = consensus(c, srcs, 0.5, 1, 1)
    assert out.tolist() == [5, 2, 0, -2] and info["selected"] == 4
    out0, info0 = consensus(c + 1, [s + 1 for s in srcs], 0.5, 0, 0.25)   # k = 0: c + lam * d whatever the masks say
    assert out0.tolist() == [2.25, 1.5, 1, 0.5] and info0["kept"] == [3, 3]
    # the exact tie |x| == tall_lambda |r| is kept (>=); a larger lambda empties elements; a NaN keeps nothing
    out, info = consensus(c[:2], [np.array([1, 1], F), np.array([2, 4], F)], 0.5, 2, 1)
    assert [k.tolist() for k in info["keep"]] == [[True, False], [True, True]] and out.tolist() == [3, 0]
    out, info = consensus(c[:2], [np.array([1, 2], F), np.array([1, 2], F), np.array([1, 2], F)], 4.0, 1, 1)
    assert info["empty"] == 2 and info["kept"] == [0, 0, 0] and out.tolist() == [0, 0]
    out, info = consensus(c[:1], [np.array([np.nan], F), np.array([1], F)], 0.5, 1, 1)
    assert info["kept"] == [0, 0] and info["empty"] == 1 and out.tolist() == [0]
    # S = 1 keeps everything: r = 0
    out, info = consensus(c, [srcs[1]], 7.0, 1, 1)
    assert info["kept"] == [4] and out.tolist() == srcs[1].tolist()
    # the restore rule, and float32(c + keep * d) for the k = 0, lam = 1 output
    cc = np.array([1, 2, 3, 4], F)
    u, info = consensus(cc, [cc + s for s in srcs], 0.5, 0, 1)
    for m in range(2):
        got, rinfo = restore(u, cc, info["words"][m])
        assert got.tobytes() == (cc + np.where(info["keep"][m], info["d"], F(0))).astype(F).tobytes()
        assert rinfo == {"kept": [3], "selected": 0, "empty": 0}


def test_pack_layout():
    keep = np.zeros(70, bool)
    keep[[0, 31, 32, 69]] = True
    w = pack(keep)
    assert w.tolist() == [0x80000001, 1, 1 << 5] and w.dtype == np.dtype("<u4")
    assert unpack(w, 70).tolist() == keep.tolist()
    assert pack(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1]  # padding bits are zero
    assert pack(np.ones(1, bool)).tolist() == [1]


def test_tall_threshold_and_consensus_k_edges(pkg):
    merge = importlib.import_module("vl_merging_amd.merge")
    assert merge.tall_threshold(0) == 0.0 and merge.tall_threshold(0.4) == 0.4 and merge.tall_threshold(float("inf")) == float("inf")
    for bad in (-0.1, -1e-300, float("nan"), True, False, "0.4", None):
        with pytest.raises(ValueError):
            merge.tall_threshold(bad)
    assert [merge.consensus_k(k, 3) for k in (0, 1, 2, 3)] == [0, 1, 2, 3] and merge.consensus_k(1, 1) == 1
    assert merge.consensus_k(7) == 7  # no source count: the caller clamps per layer
    for bad, S in ((4, 3), (2, 1), (-1, 3), (True, 3), (False, 3), (1.0, 3), ("2", 3), (None, 3), (-1, None), (True, None)):
        with pytest.raises(ValueError):
            merge.consensus_k(bad, S)
    assert merge.tall_mask_words(1) == 1 and merge.tall_mask_words(32) == 1 and merge.tall_mask_words(33) == 2


def test_tall_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_tall_plan_bytes", "vlm_tall_plan_upload", "vlm_tall_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_abi_version() == 11
    assert ctypes.sizeof(L.TallJob) == header_struct_size("vlm_tall_job_t") == 112
    assert ctypes.sizeof(L.TallHeader) == header_struct_size("vlm_tall_header_t") == 40
    assert L.TALL_COUNTERS == L.MERGE_MAX_SRC + 2 and "VLM_TALL_COUNTERS (VLM_MERGE_MAX_SRC + 2)" in txt
    assert (L.TALL_CONSENSUS, L.TALL_RESTORE) == (0, 1) and "VLM_TALL_CONSENSUS 0" in txt and "VLM_TALL_RESTORE 1" in txt
    assert ctypes.sizeof(L.DareJob) == 96 and ctypes.sizeof(L.TiesJob) == 96 and ctypes.sizeof(L.MergeJob) == 80  # untouched
    # the fields sit where the header puts them
    m = re.search(r"typedef struct \{([^}]*)\}\s*vlm_tall_job_t\s*;", txt)
    names = [re.sub(r"\[.*", "", d.split()[-1]) for d in m.group(1).split(";") if d.strip()]
    assert names == [f[0] for f in L.TallJob._fields_]


def good_job(L):
    job = L.TallJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam = 0x10000, 0x20000, 2, 100, 1.0
    job.src[0], job.src[1] = 0x30000, 0x40000
    job.mask[0], job.mask[1] = 0x50000, 0x50010
    job.op, job.k, job.tall_lambda = L.TALL_CONSENSUS, 2, 0.4
    return job


def test_tall_host_side_argument_checks(pkg):
    """vlm_tall_plan_upload rejects bad jobs before it touches the device; a job that passes every check fails at the size of the
    workspace (-3)."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_tall_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_tall_plan_bytes(1, 4096), lib.vlm_tall_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (112 + 8 * L.TALL_COUNTERS) + 8 * (1 << 12)  # jobs, counters, 2^12 chunk records
    ws = ctypes.c_void_p(0x100000)

    def upload(j, n=1, w=ws, nbytes=small):
        return lib.vlm_tall_plan_upload((L.TallJob * 1)(j), n, w, nbytes, None)

    def changed(**fields):
        j = L.TallJob.from_buffer_copy(bytes(good_job(L)))
        for f, v in fields.items():
            if "_" in f and f.split("_")[0] in ("mask", "src") and f.split("_")[1].isdigit():
                getattr(j, f.split("_")[0])[int(f.split("_")[1])] = v
            else:
                setattr(j, f, v)
        return j

    job = good_job(L)
    assert upload(job, w=ctypes.c_void_p(0)) == -1          # no workspace
    assert upload(job, n=0) == -1                            # no jobs
    assert upload(job, nbytes=64) == -3                      # VLM_ERR_WORKSPACE: every argument check passed
    bad = [dict(n_src=0), dict(n_src=5), dict(dst=0), dict(base=0), dict(dst=0x10004), dict(n_elem=0), dict(src_1=0),
           dict(dst=0x20010), dict(dst=0x2fff0),                                  # dst partly over an input
           dict(k=3), dict(k=-1), dict(tall_lambda=-0.5), dict(tall_lambda=float("nan")), dict(op=2), dict(op=-1),
           dict(mask_1=0), dict(mask_0=0),                                        # some but not all masks
           dict(mask_1=0x50008), dict(mask_0=0x50004),                            # misaligned
           dict(mask_1=0x50000),                                                  # two masks, one range
           dict(n_elem=129),                                                      # five words each: the masks now meet
           dict(mask_0=0x10000), dict(mask_1=0x10180), dict(mask_0=0x20000), dict(mask_1=0x30010), dict(mask_0=0x40180),
           dict(mask_0=0xfff0, n_elem=129),                                       # runs into dst from below
           dict(op=L.TALL_RESTORE), dict(op=L.TALL_RESTORE, n_src=1, k=0, mask_0=0), dict(op=L.TALL_RESTORE, n_src=1, k=2)]
    for fields in bad:
        assert upload(changed(**fields)) == -1, fields
    ok = [dict(), dict(mask_0=0, mask_1=0), dict(k=0), dict(k=1), dict(tall_lambda=0.0), dict(dst=0x20000), dict(dst=0x30000),
          dict(dst=0x40000), dict(mask_1=0x10190), dict(mask_0=0xfff0), dict(n_src=1, k=1),
          dict(op=L.TALL_RESTORE, n_src=1, k=0), dict(op=L.TALL_RESTORE, n_src=1, k=1, dst=0x30000)]
    for fields in ok:
        assert upload(changed(**fields), nbytes=64) == -3, fields
    four = changed(n_src=4, k=4, src_2=0x60000, src_3=0x70000, mask_2=0x50020, mask_3=0x50030)
    assert upload(four, nbytes=64) == -3
    four.mask[3] = 0
    assert upload(four, nbytes=64) == -1
    long = changed(n_elem=1 << 34, mask_0=0, mask_1=0, dst=0x1000000000, base=0x2000000000, src_0=0x3000000000, src_1=0x4000000000)
    assert upload(long) == -4                                # VLM_ERR_UNSUPPORTED: the family's length limit
    assert lib.vlm_tall_run(ctypes.c_void_p(0), None) == -1


def test_tall_mask_header_on_the_host(tmp_path):
    """csrc/tall_mask.h without HIP, as a stand-alone program under AddressSanitizer + UBSan: the kernel's walk (slots, lane groups,
    the tail's lane, the fifth slot) packs a known pattern into a buffer of exactly ceil(n / 32) words for every length the GPU
    tests use and the edges around 32, 4096 and 8192 elements; and tall_job_check's verdicts on a fixed list of jobs."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "tall_pack_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "tall_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    sizes = [1, 2, 3, 4, 5, 23, 28, 29, 31, 32, 33, 35, 63, 64, 65, 1023, 4092, 4095, 4096, 4097, 4098, 4099, 4100, 4110, 4127,
             4128, 4129, 8191, 8192, 8193, 8195, 12289, 70001, 1 << 20, (1 << 20) + 3]
    r = subprocess.run([exe, "pack"] + [str(n) for n in sizes], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = [ln.split() for ln in r.stdout.split("\n") if ln.startswith("pack ")]
    assert [(int(a), int(b)) for _, a, b, _ in rows] == [(n, (n + 31) // 32) for n in sizes]
    assert all(0 < int(p) <= n for (_, _, _, p), n in zip(rows, sizes))
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = dict((ln.split()[1], int(ln.split()[2])) for ln in r.stdout.split("\n") if ln.startswith("check "))
    passing = {"good", "no_masks", "mask_behind_dst", "mask_before_base", "k_zero", "lambda_zero", "restore"}
    assert len(got) == 22 and passing <= set(got)
    assert got == {name: (0 if name in passing else -1) for name in got}


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.TallPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.consensus_merge({}, cfg, central_weight={}, device="cpu")
    with pytest.raises(L.VlmError):
        merge.tall_restore({}, {}, cfg, central_weight={}, device="cpu")
    for bad in (-0.1, float("nan"), True):
        with pytest.raises(ValueError):
            merge.consensus_merge({}, cfg, central_weight={}, tall_lambda=bad)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            merge.consensus_merge({}, cfg, central_weight={}, k=bad)
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.consensus_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ----------------------------------------------------------------------------------------------- the command lines
def run_tool(tool, *argv):
    return subprocess.run([sys.executable, tool] + list(argv), capture_output=True, text=True, timeout=300)


def test_merge_ckpt_consensus_argument_errors_as_a_child_process():
    base = ["--method", "consensus", "--ckpt", "missing.ckpt", "--out", "out.ckpt"]
    for bad, word in ((["--tall-lambda", "-0.5"], "tall_lambda"), (["--tall-lambda", "nan"], "tall_lambda"),
                      (["--consensus-k", "-1"], "consensus k")):
        r = run_tool(TOOL, *(base + bad))
        assert r.returncode != 0 and "ValueError" in r.stderr and word in r.stderr, (bad, r.stderr[-500:])
    r = run_tool(TOOL, *(base + ["--consensus-k", "1.5"]))       # argparse's own error
    assert r.returncode == 2 and "--consensus-k" in r.stderr
    r = run_tool(TOOL, "--method", "dare", "--ckpt", "missing.ckpt", "--out", "out.ckpt", "--masks-out", "m.pt")
    assert r.returncode != 0 and "--masks-out belongs to --method consensus" in r.stderr
    r = run_tool(TOOL, "--help")
    assert r.returncode == 0, r.stderr
    for word in ("consensus", "--tall-lambda", "--consensus-k", "--masks-out", "dare", "--drop"):
        assert word in r.stdout
    r = run_tool(RESTORE_TOOL, "--help")
    assert r.returncode == 0, r.stderr
    for word in ("--unified", "--central", "--masks", "--out", "tall-masks-1"):
        assert word in r.stdout
    r = run_tool(RESTORE_TOOL, "--unified", "u.ckpt", "--out", "o.ckpt")
    assert r.returncode == 2 and "--masks" in r.stderr


def test_merge_ckpt_accepts_the_consensus_options(pkg):
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        mc = importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)
    args, cfg = mc.parse_args(["--method", "consensus", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--tall-lambda", "0.5", "--consensus-k",
                               "1", "--masks-out", "m.pt", "--lambda", "0.75", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.tall_lambda, args.consensus_k, args.masks_out) == ("consensus", 0.5, 1, "m.pt")
    assert cfg["sum_lambda"] == 0.75
    args, _ = mc.parse_args(["--method", "consensus", "--ckpt", "a", "--out", "b"])
    assert (args.tall_lambda, args.consensus_k, args.masks_out) == (0.4, 2, None)
    args, _ = mc.parse_args(["--method", "ties", "--ckpt", "a", "--out", "b", "--density", "0.1"])  # the others are as they were
    assert args.method == "ties" and args.density == 0.1
