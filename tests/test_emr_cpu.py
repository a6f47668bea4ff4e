"""EMR-Merging, host side (no GPU): the numpy restatement of the rule (emr_restatement.py) by hand, its edge cases and the L1
property the method exists for, what the planted inputs reach, the ABI additions, the upload checks that need no device, and the
command lines.  The reference has no such merge: nothing here is pinned to it."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from emr_restatement import chunk_records, emr, ordered_sums, pack, restore, unpack
from pairstats_restatement import ordered_sums as pairstats_ordered_sums
from test_ties_cpu import header_struct_size, header_text
from test_ties_gpu import planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
RESTORE_TOOL = os.path.join(ROOT, "vl-merging_amd", "tall_restore.py")
F, D = np.float32, np.float64


def inputs(n, S, seed):
    """planted(n, S, seed); planted needs two sources, so S = 1 is the first source of planted(n, 2, seed)."""
    c, srcs = planted(n, max(S, 2), seed)
    return c, srcs[:S]


def test_restatement_by_hand():
    """c = 0; x_0 = [4, 1, 0, 1, -2], x_1 = [1, 1, 0, -3, 2].  s = [5, 2, 0, -2, 0].  Expert 0 agrees where s and x_0 share a sign:
    [1, 1, 0, 0, 0]; expert 1: [1, 1, 0, 1, 0].  e = [max(4, 1), max(1, 1), 0, 3, 0], u = [4, 1, 0, -3, 0].  a = [4+1+0+1+2,
    1+1+0+3+2] = [8, 7]; b_0 = 4 + 1 = 5, b_1 = 4 + 1 + 3 = 8; rescale = [8 / 5, 7 / 8] = [1.6, 0.875].  zero: elements 2 and 4;
    conflict: elements 3 and 4."""
    c = np.zeros(5, F)
    srcs = [np.array([4, 1, 0, 1, -2], F), np.array([1, 1, 0, -3, 2], F)]
    out, info = emr(c, srcs, 1)
    assert info["s"].tolist() == [5, 2, 0, -2, 0] and info["u"].tolist() == [4, 1, 0, -3, 0] and out.tolist() == [4, 1, 0, -3, 0]
    assert [a.astype(int).tolist() for a in info["agree"]] == [[1, 1, 0, 0, 0], [1, 1, 0, 1, 0]]
    assert [int(w[0]) for w in info["words"]] == [0b00011, 0b01011] and all(w.size == 1 and w.dtype == np.dtype("<u4") for w in info["words"])
    assert info["abs_sum"] == [8.0, 7.0] and info["uni_sum"] == [5.0, 8.0]
    assert [r.tobytes() for r in info["rescale"]] == [F(1.6).tobytes(), F(0.875).tobytes()]
    assert (info["kept"], info["zero"], info["conflict"]) == ([2, 3], 2, 2)
    out, _ = emr(c + 1, [s + 1 for s in srcs], 0.25)
    assert out.tolist() == [2, 1.25, 1, 0.25, 1]
    # -0.0 and NaN sums count as zero
    _, info = emr(np.zeros(2, F), [np.array([-0.0, np.nan], F), np.array([-0.0, 1], F)], 1)
    assert info["zero"] == 2 and info["kept"] == [0, 0] and info["u"].tobytes() == np.zeros(2, F).tobytes()
    # the restore rule: three roundings
    cc = np.array([1, 2, 3, 4, 5], F)
    u, info = emr(cc, [cc + s for s in srcs], 1)
    for m in range(2):
        got, rinfo = restore(u, cc, info["words"][m], info["rescale"][m])
        t = np.where(info["agree"][m], u - cc, F(0)).astype(F)
        assert got.tobytes() == (cc + info["rescale"][m] * t).astype(F).tobytes() and rinfo == {"kept": [info["kept"][m]]}
    assert restore(u, cc, info["words"][0], 1.6)[0].tolist() == [F(1) + F(1.6) * F(4), F(2) + F(1.6) * F(1), 3, 4, 5]


def test_one_source_is_its_own_unified_vector():
    for n in (1, 3, 23, 4097, 12289):
        c, (w,) = inputs(n, 1, 7)
        out, info = emr(c, [w], 1)
        x = w - c
        assert info["u"].tobytes() == np.where(x != 0, x, F(0)).astype(F).tobytes()   # u = x_0 (a -0.0 entry gives +0.0)
        assert info["agree"][0].tolist() == (x != 0).tolist() and info["conflict"] == 0 and info["zero"] == int((x == 0).sum())
        assert info["abs_sum"] == info["uni_sum"]
        assert info["rescale"][0].tobytes() == F(1.0 if info["abs_sum"][0] > 0 else 0.0).tobytes()
    assert emr(*inputs(12289, 1, 7), 1)[1]["rescale"][0] == F(1.0)


def test_a_source_that_never_agrees():
    """x_0 >= 1 and -2^-6 - 0.25 |g| <= x_1 < 0: the sum is positive everywhere, source 1 never agrees: an all-zero mask, rescale
    +0.0, and a restore that equals c."""
    rng = np.random.default_rng(3)
    n = 4110
    c = np.zeros(n, F)
    x0 = (1 + np.abs(rng.standard_normal(n))).astype(F)
    x1 = (-(2.0 ** -6) - 0.25 * np.abs(np.clip(rng.standard_normal(n), -3, 3))).astype(F)
    assert (x0 >= 1).all() and (x1 < 0).all() and (x1 >= -1).all()
    cc = rng.standard_normal(n).astype(F)
    for base in (c, cc):
        srcs = [(base + x0).astype(F), (base + x1).astype(F)]
        out, info = emr(base, srcs, 1)
        assert info["kept"] == [n, 0] and info["zero"] == 0 and info["conflict"] == n
        assert [r.tobytes() for r in info["rescale"]] == [F(1.0).tobytes(), F(0.0).tobytes()]
        assert not info["words"][1].any() and info["uni_sum"][1] == 0.0
        got, rinfo = restore(out, base, info["words"][1], info["rescale"][1])
        assert got.tobytes() == base.tobytes() and rinfo["kept"] == [0]


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [23, 4097, 12289])
def test_restore_gives_every_expert_its_l1_mass(n, S):
    """What the rescaler is for.  With c = 0, uni - c is u exactly, so restore_m = rescale_m * (agree_m ? u : 0) elementwise and
    sum |restore_m| = rescale_m * b[m] up to one fp32 rounding per product (2^-24 relative each, so 2^-24 of the sum), while
    rescale_m = a[m] / b[m] up to its own fp32 rounding (2^-24); the f64 sums of at most 12289 addends add below 2^-38.  Together
    under 2^-23 + 2^-38 < 2^-22."""
    c, srcs = inputs(n, S, 7)
    xs = [(w - c).astype(F) for w in srcs]
    zero = np.zeros(n, F)
    out, info = emr(zero, xs, 1)
    assert out.tobytes() == info["u"].tobytes()   # the unified tensor is the unified task vector
    for m in range(S):
        got, _ = restore(out, zero, info["words"][m], info["rescale"][m])
        l1 = float(np.abs(got).astype(D).sum())
        a = info["abs_sum"][m]
        assert a > 0 and abs(l1 - a) <= a * 2.0 ** -22, (n, S, m, l1, a)
        assert (np.sign(got) * np.sign(xs[m]) >= 0)[info["agree"][m]].all()   # never an entry of the wrong sign


def test_planted_inputs_reach_every_case():
    """What the GPU cases rely on (numpy only): on planted(12289, S, 7) zero sums, sign conflicts and every vote level 0 .. S
    occur, and where the sum is not zero a source agrees and u != 0."""
    for S in (2, 3, 4):
        c, srcs = planted(12289, S, 7)
        _, info = emr(c, srcs, 1)
        assert info["zero"] >= 100 and info["conflict"] >= 1000, (S, info["zero"], info["conflict"])
        assert set(np.unique(info["votes"]).tolist()) == set(range(S + 1)), S
        nz = info["s"] != 0
        assert (info["votes"][nz] >= 1).all() and (info["u"][nz] != 0).all() and not info["u"][~nz].any()


def test_the_tail_rule_differs_from_the_pair_statistics():
    """Step 6: the tail's addends enter ONE thread's sums, behind its float4s, in element order.  Addends chosen so that the order
    shows: the tail [1, 2^53, -2^53] in one thread is ((0 + 1) + 2^53) - 2^53 = 0 (the 1 is lost to the tie), where the pair
    statistics' lanes 0, 1, 2 fold as (1 - 2^53) + 2^53 = 1."""
    for n, thread, chunk in ((3, 0, 0), (23, 5, 0), (4099, 0, 0), (4110, 3, 1), (4 * 300 + 2, 44, 0), (8192 + 3, 0, 1)):
        term = np.zeros((1, n), D)
        term[0, n - (n & 3):] = 1.0
        rec = chunk_records(term)
        assert rec.shape == (1, max(1, -(-(n // 4) // 1024))) and rec[0, chunk] == (n & 3) and rec.sum() == (n & 3), n
        assert (n // 4) & 255 == thread
    t = np.zeros(7, D)
    t[4:] = [1, 2.0 ** 53, -2.0 ** 53]
    assert ordered_sums([t]) == [0.0] and pairstats_ordered_sums([t]) == [1.0]
    # the float4s of the tail's thread come first
    t = np.zeros(4 * 257 + 2, D)          # n4 = 257: thread 1, whose float4 is 1 (u = 0); the tail stands at its u = 1
    t[4] = 2.0 ** 53
    t[-2:] = 1
    assert ordered_sums([t]) == [2.0 ** 53]
    t[4], t[8] = 0, 2.0 ** 53             # thread 2's: the tail's 1 + 1 = 2 meets it only in the wave fold
    assert ordered_sums([t]) == [2.0 ** 53 + 2]


def test_pack_is_the_consensus_layout():
    keep = np.zeros(70, bool)
    keep[[0, 31, 32, 69]] = True
    assert pack(keep).tolist() == [0x80000001, 1, 1 << 5] and unpack(pack(keep), 70).tolist() == keep.tolist()
    import tall_restatement
    assert pack is tall_restatement.pack and unpack is tall_restatement.unpack


def test_emr_entry_points_declared_exported_bound(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    txt = header_text()
    for s in ("vlm_emr_plan_bytes", "vlm_emr_plan_upload", "vlm_emr_run"):
        assert re.search(r"\b" + s + r"\s*\(", txt), "header does not declare " + s
        assert hasattr(lib, s), "library does not export " + s
        assert s in L.SIGNATURES, "ctypes binding lacks " + s
    assert lib.vlm_abi_version() == 11
    assert ctypes.sizeof(L.EmrJob) == header_struct_size("vlm_emr_job_t") == 104
    assert ctypes.sizeof(L.EmrHeader) == header_struct_size("vlm_emr_header_t") == 56 == ctypes.sizeof(L.StockHeader)
    assert ctypes.sizeof(L.EmrResult) == 128 and L.EmrResult.rescale.offset == 112   # emr.hip's static_assert holds the C side to it
    assert L.EMR_SUMS == 3 * L.MERGE_MAX_SRC + 2 and "VLM_EMR_SUMS (3 * VLM_MERGE_MAX_SRC + 2)" in txt
    assert (L.EMR_MERGE, L.EMR_RESTORE) == (0, 1) and "VLM_EMR_MERGE 0" in txt and "VLM_EMR_RESTORE 1" in txt
    assert ctypes.sizeof(L.TallJob) == 112 and ctypes.sizeof(L.StockJob) == 64   # untouched
    for ctype, name in ((L.EmrJob, "vlm_emr_job_t"), (L.EmrResult, "vlm_emr_result_t"), (L.EmrHeader, "vlm_emr_header_t")):
        m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt)
        names = []
        for d in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):   # "uint64_t n_jobs, n_chunks" declares two
            parts = [p.strip() for p in d.split(",")] if d.strip() else []
            names += [re.sub(r"\[.*", "", p.split()[-1]) for p in parts]
        assert names == [f[0] for f in ctype._fields_], name


def good_job(L):
    job = L.EmrJob()
    job.dst, job.base, job.n_src, job.n_elem, job.lam = 0x10000, 0x20000, 2, 100, 1.0
    job.src[0], job.src[1] = 0x30000, 0x40000
    job.mask[0], job.mask[1] = 0x50000, 0x50010
    job.op, job.rescale = L.EMR_MERGE, 0.0
    return job


def test_emr_host_side_argument_checks(pkg):
    """vlm_emr_plan_upload rejects bad jobs before it touches the device; a job that passes every check fails at the size of the
    workspace (-3)."""
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    assert lib.vlm_emr_plan_bytes(-1, 0) == 0
    small, big = lib.vlm_emr_plan_bytes(1, 4096), lib.vlm_emr_plan_bytes(100, 1 << 24)
    assert 0 < small < big and big >= 100 * (104 + 128) + (8 + 8 * L.EMR_SUMS) * (1 << 12)  # jobs, results, 2^12 chunks and records
    ws = ctypes.c_void_p(0x100000)

    def upload(j, n=1, w=ws, nbytes=small):
        return lib.vlm_emr_plan_upload((L.EmrJob * 1)(j), n, w, nbytes, None)

    def changed(**fields):
        j = L.EmrJob.from_buffer_copy(bytes(good_job(L)))
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
    restore_ok = dict(op=L.EMR_RESTORE, n_src=1, rescale=1.7)
    bad = [dict(n_src=0), dict(n_src=5), dict(dst=0), dict(base=0), dict(dst=0x10004), dict(n_elem=0), dict(src_1=0),
           dict(dst=0x20010), dict(dst=0x2fff0),                                  # dst partly over an input
           dict(op=2), dict(op=-1),
           dict(mask_1=0), dict(mask_0=0),                                        # a partial mask set
           dict(mask_1=0x50008), dict(mask_0=0x50004),                            # misaligned
           dict(mask_1=0x50000),                                                  # the other mask
           dict(n_elem=129),                                                      # five words each: the masks now meet
           dict(mask_0=0x10000), dict(mask_1=0x10180),                            # on dst
           dict(mask_0=0x20000), dict(mask_1=0x30010), dict(mask_0=0x40180),      # on the base, on a source
           dict(mask_0=0xfff0, n_elem=129),                                       # runs into dst from below
           dict(op=L.EMR_RESTORE, rescale=1.0),                                   # restore with two sources
           dict(restore_ok, mask_0=0),                                            # restore without its mask
           dict(restore_ok, rescale=float("nan")), dict(restore_ok, rescale=-0.5), dict(restore_ok, rescale=float("inf")),
           dict(restore_ok, rescale=-float("inf"))]
    for fields in bad:
        assert upload(changed(**fields)) == -1, fields
    ok = [dict(), dict(mask_0=0, mask_1=0), dict(lam=-2.0), dict(rescale=float("nan")),   # MERGE does not read rescale
          dict(dst=0x20000), dict(dst=0x30000), dict(dst=0x40000), dict(mask_1=0x10190), dict(mask_0=0xfff0), dict(n_src=1),
          restore_ok, dict(restore_ok, rescale=0.0), dict(restore_ok, rescale=-0.0), dict(restore_ok, dst=0x30000),
          dict(restore_ok, dst=0x20000)]
    for fields in ok:
        assert upload(changed(**fields), nbytes=64) == -3, fields
    four = changed(n_src=4, src_2=0x60000, src_3=0x70000, mask_2=0x50020, mask_3=0x50030)
    assert upload(four, nbytes=64) == -3
    four.mask[3] = 0
    assert upload(four, nbytes=64) == -1
    long = changed(n_elem=1 << 34, mask_0=0, mask_1=0, dst=0x1000000000, base=0x2000000000, src_0=0x3000000000, src_1=0x4000000000)
    assert upload(long) == -4                                # VLM_ERR_UNSUPPORTED: the family's length limit
    assert lib.vlm_emr_run(ctypes.c_void_p(0), None) == -1


def test_emr_host_code_on_the_host(tmp_path):
    """What emr.hip takes from csrc/tall_mask.h and csrc/chunk_plan.h without HIP, as a stand-alone program under AddressSanitizer +
    UBSan: for every length the GPU tests use (the long job at 256 CUs) exactly one place of the kernel's walk stands at the ragged
    tail -- the job's last chunk, thread n4 & 255, with no float4 of that thread behind it -- and the verdicts of the upload's
    per-job check on a fixed list of jobs."""
    import shutil
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "emr_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "emr_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    sizes = [1, 2, 3, 4, 5, 23, 31, 32, 33, 63, 1023, 4096, 4097, 4098, 4099, 4100, 4110, 8191, 8193, 8195, 12289, 70000, 70001,
             1 << 18, 4096 * (2 * 12 * 256 + 3) + 5]
    r = subprocess.run([exe, "tail"] + [str(n) for n in sizes], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = [ln.split()[1:] for ln in r.stdout.split("\n") if ln.startswith("tail ")]
    want = [[str(n), "none"] if n % 4 == 0 else [str(n), str(max(1, -(-(n // 4) // 1024)) - 1), str((n // 4) & 255)] for n in sizes]
    assert [row[:3] for row in rows] == want
    slot = {row[0]: int(row[3]) for row in rows if row[1] != "none"}
    assert slot["4097"] == 4 and slot["8195"] == 4 and slot["4099"] == 4      # the fifth slot: n4 a positive multiple of 1024
    assert slot["3"] == 0 and slot["4110"] == 0 and slot["1023"] == 0 and slot["70001"] == 0
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = dict((ln.split()[1], int(ln.split()[2])) for ln in r.stdout.split("\n") if ln.startswith("check "))
    passing = {"good", "no_masks", "mask_behind_dst", "dst_is_base", "dst_is_src1", "merge_ignores_rescale", "restore", "restore_zero",
               "restore_in_place"}
    assert len(got) == 24 and passing <= set(got)
    assert got == {name: (0 if name in passing else -1) for name in got}


def test_emr_kernels_keep_the_budget_their_head_comment_states():
    """Neither kernel may spill vector registers or use scratch -- the pass kernel holds every instantiation up to S = 4 with masks
    on.  The pass's grid (12 workgroups per CU, tall.hip's value) counts on the three resident workgroups per CU that
    vlm_tall_apply_kernel has; its LDS is the two record buffers of four waves' fourteen doubles."""
    import json
    import test_build_cpu as tb
    if tb._stale():
        import __graft_entry__ as ge
        ge.build()
    with open(tb.RES) as f:
        resources = json.load(f)
    found = {}
    for name in ("vlm_emr_pass_kernel", "vlm_emr_fold_kernel"):
        hit = [v for k, v in resources.items() if name in k]
        assert len(hit) == 1, sorted(k for k in resources if "emr" in k)
        found[name] = hit[0]
        assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["AGPRs"] == 0, (name, hit[0])
    assert found["vlm_emr_pass_kernel"]["Occupancy"] >= 3, found["vlm_emr_pass_kernel"]
    assert found["vlm_emr_pass_kernel"]["LDS Size"] == 2 * 4 * 14 * 8
    assert len([k for k in resources if "vlm_tall_apply_kernel" in k]) == 1   # the consensus kernels are still there, one each


def test_cpu_device_and_bad_arguments_are_rejected(pkg):
    import torch
    merge = importlib.import_module("vl_merging_amd.merge")
    L = importlib.import_module("vl_merging_amd._lib")
    with pytest.raises(L.VlmError):
        merge.EmrPlan("cpu")
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, sum_lambda=1, loss_names={})
    with pytest.raises(L.VlmError):
        merge.emr_merge({}, cfg, central_weight={}, device="cpu")
    with pytest.raises(L.VlmError):
        merge.emr_restore({}, {}, {}, cfg, central_weight={}, device="cpu")
    assert merge.emr_rescale(0) == 0.0 and merge.emr_rescale(1.7) == 1.7
    for bad in (-0.1, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError):
            merge.emr_rescale(bad)
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")
    assert callable(vm.ViLTransformerSS.emr_merge)
    assert torch.zeros(1).device.type == "cpu"  # nothing above needed a device


# ----------------------------------------------------------------------------------------------- the command lines
def run_tool(tool, *argv):
    return subprocess.run([sys.executable, tool] + list(argv), capture_output=True, text=True, timeout=300)


def test_merge_ckpt_emr_argument_errors_as_a_child_process():
    r = run_tool(TOOL, "--method", "emr", "--ckpt", "missing.ckpt", "--out", "out.ckpt", "--lambda", "x")   # argparse's own error
    assert r.returncode == 2 and "--lambda" in r.stderr
    r = run_tool(TOOL, "--method", "emr", "--ckpt", "missing.ckpt", "--out", "out.ckpt", "--masks-out", "m.pt")
    assert r.returncode != 0 and "missing.ckpt" in r.stderr and "--masks-out" not in r.stderr   # the options pass; the file is missing
    r = run_tool(TOOL, "--method", "stock", "--ckpt", "missing.ckpt", "--out", "out.ckpt", "--masks-out", "m.pt")   # the wording stays
    assert r.returncode != 0 and "ValueError" in r.stderr and "--masks-out belongs to --method consensus or emr (got stock)" in r.stderr
    r = run_tool(TOOL, "--help")
    assert r.returncode == 0, r.stderr
    for word in ("emr", "emr_merge", "--masks-out", "emr-masks-1", "consensus", "tall-masks-1"):
        assert word in r.stdout, word
    r = run_tool(RESTORE_TOOL, "--help")
    assert r.returncode == 0, r.stderr
    for word in ("--unified", "--central", "--masks", "--out", "tall-masks-1", "emr-masks-1"):
        assert word in r.stdout, word


def test_merge_ckpt_accepts_the_emr_options(pkg):
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        mc = importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)
    args, cfg = mc.parse_args(["--method", "emr", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--masks-out", "m.pt", "--lambda", "0.75",
                               "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.masks_out) == ("emr", "m.pt") and cfg["sum_lambda"] == 0.75
    args, _ = mc.parse_args(["--method", "emr", "--ckpt", "a", "--out", "b"])
    assert args.masks_out is None
    args, _ = mc.parse_args(["--method", "consensus", "--ckpt", "a", "--out", "b", "--masks-out", "m.pt"])  # as it was
    assert (args.method, args.masks_out) == ("consensus", "m.pt")
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "sce", "--ckpt", "a", "--out", "b", "--masks-out", "m.pt"])


def test_tall_restore_refuses_an_unknown_format(tmp_path):
    import torch
    sys.path.insert(0, os.path.dirname(RESTORE_TOOL))
    try:
        tr = importlib.import_module("tall_restore")
    finally:
        sys.path.pop(0)
    words = torch.zeros(1, dtype=torch.int32)
    torch.save({"format": "tall-masks-1", "tall_lambda": 0.4, "k": 0, "masks": {"a": words}}, tmp_path / "tall.pt")
    torch.save({"format": "emr-masks-1", "masks": {"a": words}, "rescalers": {"a": 1.5}}, tmp_path / "emr.pt")
    torch.save({"format": "emr-masks-2", "masks": {"a": words}, "rescalers": {"a": 1.5}}, tmp_path / "new.pt")
    torch.save({"format": "emr-masks-1", "masks": {"a": words}}, tmp_path / "half.pt")
    fmt, masks, rescalers = tr.read_masks_file(str(tmp_path / "tall.pt"))
    assert fmt == "tall-masks-1" and list(masks) == ["a"] and rescalers is None
    assert list(tr.read_masks(str(tmp_path / "tall.pt"))) == ["a"]   # the earlier entry point reads what it read
    fmt, masks, rescalers = tr.read_masks_file(str(tmp_path / "emr.pt"))
    assert fmt == "emr-masks-1" and list(masks) == ["a"] and rescalers == {"a": 1.5}
    for name in ("new.pt", "half.pt"):
        with pytest.raises(ValueError) as e:
            tr.read_masks_file(str(tmp_path / name))
        assert "tall-masks-1" in str(e.value) and "emr-masks-1" in str(e.value)
    r = run_tool(RESTORE_TOOL, "--unified", "u.ckpt", "--central", "c.ckpt", "--masks", str(tmp_path / "new.pt"), "--out", "o.ckpt")
    assert r.returncode != 0 and "ValueError" in r.stderr and "tall-masks-1" in r.stderr and "emr-masks-1" in r.stderr
