"""TSV-M without a GPU: properties of the numpy restatement of the rule (tsvm_restatement.py), the restated Jacobi sweep against
LAPACK, the tournament schedule through a stand-alone host program, the C ABI and the command line."""
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import tsvm_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
SVD_SYMBOLS = ("vlm_svd_work_doubles", "vlm_svd_steps", "vlm_svd_reset", "vlm_svd_sweep", "vlm_svd_finish")
TSV_SYMBOLS = ("vlm_tsv_delta", "vlm_tsv_gather", "vlm_tsv_apply")


def merge_ckpt():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


# ------------------------------------------------------------------------------------------------- the restatement's properties
def test_identical_experts_give_the_rank_k_truncation():
    """S copies of one expert: Ucat = [U_k .. U_k] has k singular values sqrt(S) and k (S - 1) zeros, which the polar threshold
    drops and counts; Uo = Ucat / sqrt(S), and the merged task vector is the rank-k truncation of the common task vector -- the mean
    of the S truncations, not their sum."""
    for (m, n, S) in ((12, 20, 2), (21, 9, 3)):
        c, srcs = R.planted(m, n, S)
        ref = R.tsvm(c, [srcs[0]] * S, 1.0)
        k = min(m, n) // S
        want = R.rank_k(R.taus(c, srcs[:1])[0], k)
        assert ref["k"] == k and ref["dropped"] == (k * (S - 1), k * (S - 1))
        assert np.abs(ref["T"] - want).max() <= 64 * 2.0 ** -52 * np.abs(want).max()


def test_an_expert_at_the_central_tensor_changes_nothing():
    """Its triplets are exact zeros: zero columns in Ucat and Vcat, nothing added to the polar factors' span."""
    m, n = 16, 24
    c, srcs = R.planted(m, n, 3)
    with_c = R.tsvm(c, [srcs[0], c.copy(), srcs[1]], 0.75)
    k = with_c["k"]
    # the same k from the two live experts alone: their truncations side by side
    parts = [R.truncation(t, k) for t in R.taus(c, [srcs[0], srcs[1]])]
    Uo, du = R.polar(np.concatenate([p[0] for p in parts], axis=1))
    Vo, dv = R.polar(np.concatenate([p[2] for p in parts], axis=1))
    want = (Uo * np.concatenate([p[1][:k] for p in parts])) @ Vo.T
    assert (du, dv) == (0, 0) and with_c["dropped"] == (k, k)
    assert np.abs(with_c["T"] - want).max() <= 64 * 2.0 ** -52 * np.abs(want).max()
    assert not np.any(with_c["scat"][k:2 * k])


def test_no_rank_to_share_gives_the_central_tensor():
    c, srcs = R.planted(2, 9, 3)
    ref = R.tsvm(c, srcs, 0.75)
    assert ref["k"] == 0 and ref["out"].tobytes() == c.tobytes() and not ref["T"].any()


def test_orthogonal_experts_merge_to_the_sum_of_their_truncations():
    """Task vectors whose row spaces and column spaces are mutually orthogonal: Ucat and Vcat have orthonormal columns, the polar
    factors are Ucat and Vcat themselves, and the merge is sum_i trunc_k(tau_i)."""
    rng = np.random.default_rng(3)
    m, n, S = 24, 36, 3
    k = min(m, n) // S
    u, _ = np.linalg.qr(rng.standard_normal((m, m)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    c = np.zeros((m, n), R.F)
    ts = [(u[:, 8 * i: 8 * i + 8] * np.geomspace(1.0, 0.1, 8)) @ v[:, 12 * i: 12 * i + 8].T for i in range(S)]   # rank 8 = k each
    srcs = [t.astype(R.F) for t in ts]
    ref = R.tsvm(c, srcs, 1.0)
    want = sum(R.rank_k(t, k) for t in R.taus(c, srcs))
    assert ref["dropped"] == (0, 0)
    assert np.abs(ref["T"] - want).max() <= 1e-6 * np.abs(want).max()   # fp32 inputs: orthogonal to 6e-8, not exactly
    c2, srcs2, total = R.exact_case(16, 24, 2)                          # exactly orthogonal: the closed form, bit for bit
    ref2 = R.tsvm(c2, srcs2, 1.0)
    assert ref2["T"].tobytes() == total.tobytes() and ref2["out"].tobytes() == total.astype(R.F).tobytes()


def test_the_two_orders_agree():
    c, srcs = R.planted(33, 70, 2)
    a, b = R.tsvm(c, srcs, 0.75), R.tsvm(c, srcs, 0.75, flip=True)
    spread = np.abs(a["T"] - b["T"]).max()
    assert spread <= 1e-12 * np.abs(a["T"]).max()
    u = R.ulp_diff(a["out"], b["out"])
    assert u.max() <= 1 and (u > 0).sum() <= max(2, 1e-4 * c.size)


@pytest.mark.parametrize("m,n,S", R.MERGE_CASES)
def test_the_gpu_inputs_are_well_posed(m, n, S):
    """The condition of the GPU test's fp32 cap: on every input it uses, the restatement's own two orders agree to at most 1 ulp in
    at most max(2, 1e-4 n) elements, at both lam; and the planted gap at the cut is there."""
    c, srcs = R.planted(m, n, S)
    a, b = R.tsvm(c, srcs, 1.0), R.tsvm(c, srcs, 1.0, flip=True)
    for lam in (0.75, 1.0):
        u = R.ulp_diff(R.finish(c, a["T"], lam), R.finish(c, b["T"], lam))
        assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * c.size), (lam, int(u.max()), int((u > 0).sum()))
    k = a["k"]
    if 0 < k < min(m, n):
        assert all(s[k - 1] > 5 * s[k] for s in a["s"])
    assert a["dropped"] == b["dropped"] == (0, 0)


# ------------------------------------------------------------------------------------------------- the restated sweep
@pytest.mark.parametrize("p,q", R.SHAPES)
def test_restated_sweeps_reach_the_svd(p, q):
    A0 = R.gaussian(p, q)
    A, Rm, counts = R.jacobi(A0)
    s = np.sqrt((A * A).sum(1))
    ref = np.linalg.svd(A0, compute_uv=False)
    assert (p == 1 and counts == []) or counts[-1] == 0
    assert np.abs(np.sort(s)[::-1] - ref).max() <= 8 * p * 2.0 ** -52 * ref[0]
    assert np.abs(Rm @ Rm.T - np.eye(p)).max() <= 8 * p * 2.0 ** -52
    assert np.abs(Rm.T @ A - A0).max() <= 8 * p * 2.0 ** -52 * ref[0]


@pytest.mark.parametrize("q", R.PAIR_Q)
def test_restated_sweeps_on_duplicate_one_hot_pairs(q):
    """The exact case of the GPU suite (test_tsvm_gpu.py) through the restated sweep: the values it asserts on the device are
    what the device's formulas give in numpy doubles."""
    A0, C, v = R.duplicate_pairs(q)
    assert C[0] == 0 and C[-1] == q - 1 and len(C) == len(set(C)) and A0.shape == (2 * len(C), q)
    assert all(u * 256 in C and min(u * 256 + 255, q - 1) in C for u in range((q + 255) // 256))
    A, Rm, counts = R.jacobi(A0)
    s = np.sqrt((A * A).sum(1))
    Vt = np.divide(A, s[:, None], out=np.zeros_like(A), where=s[:, None] > 0)
    R.check_duplicate_pairs(C, v, s, Vt, Rm, counts)


@pytest.mark.parametrize("p,q", R.BOUNDARY_SKINNY)
def test_restated_sweeps_reach_the_svd_at_the_long_rows(p, q):
    """The skinny shapes of the GPU suite past q = 512, under the GPU suite's own constants (p 2^-52 units, test_tsvm_gpu.py):
    the algorithm alone is well inside them, so a device value above is the kernel's."""
    A0 = R.gaussian(p, q)
    A, Rm, counts = R.jacobi(A0)
    s = np.sqrt((A * A).sum(1))
    Vt = A / s[:, None]
    sl = np.linalg.svd(A0, compute_uv=False)
    unit = p * 2.0 ** -52
    assert counts[-1] == 0
    assert np.abs(Rm @ Rm.T - np.eye(p)).max() <= 16.0 * unit and np.abs(Vt @ Vt.T - np.eye(p)).max() <= 12.0 * unit
    assert np.sqrt(((A0 - Rm.T @ A) ** 2).sum()) <= 8.2 * unit * np.sqrt((A0 * A0).sum())
    assert np.abs(np.sort(s)[::-1] - sl).max() <= 4.4 * unit * sl[0]


@pytest.mark.parametrize("m,n,S", R.BOUNDARY_MERGE)
def test_the_boundary_merge_inputs_are_well_posed(m, n, S):
    """test_the_gpu_inputs_are_well_posed for the two merges past the kernels' grid caps, at the lam = 1 the GPU suite runs."""
    c, srcs = R.planted(m, n, S)
    a, b = R.tsvm(c, srcs, 1.0), R.tsvm(c, srcs, 1.0, flip=True)
    u = R.ulp_diff(a["out"], b["out"])
    assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * c.size), (int(u.max()), int((u > 0).sum()))
    k = a["k"]
    assert k * S in (512, 513) and all(s[k - 1] > 5 * s[k] for s in a["s"]) and a["dropped"] == b["dropped"] == (0, 0)


def test_restated_schedule_matches_the_header():
    """pairs() is csrc/jacobi_schedule.h in numpy: every pair once per sweep, disjoint within a step."""
    for p in list(range(1, 10)) + [64]:
        seen = set()
        for t in range(R.steps(p)):
            i, j = R.pairs(p, t)
            assert len(i) == p // 2 and (i < j).all() and (j < p).all() and (i >= 0).all()
            assert len(set(i.tolist()) | set(j.tolist())) == 2 * (p // 2)
            seen |= set(zip(i.tolist(), j.tolist()))
        assert len(seen) == p * (p - 1) // 2


def test_the_tournament_schedule_under_the_sanitizers(tmp_path):
    """helpers/jacobi_schedule_check.cpp over csrc/jacobi_schedule.h, which has no HIP in it: every pair exactly once per sweep and
    disjoint pairs within a step for p = 1 .. 9, 64 and more, built with -fsanitize=address,undefined."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "helpers", "jacobi_schedule_check.cpp")
    exe = str(tmp_path / "jacobi_schedule_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "jacobi_schedule_check: ok" in r.stdout


# ------------------------------------------------------------------------------------------------- the surface
def test_abi_exports_the_svd_and_tsv_entries(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    header = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    for s in SVD_SYMBOLS + TSV_SYMBOLS:
        assert hasattr(lib, s) and s in L.SIGNATURES and ("%s(" % s) in header, s
    assert sorted(s for s in L.SIGNATURES if s.startswith(("vlm_svd_", "vlm_tsv_"))) == sorted(SVD_SYMBOLS + TSV_SYMBOLS)
    assert lib.vlm_abi_version() == 11 and "#define VLM_ABI_VERSION 11" in header
    assert "#define VLM_SVD_HEAD %d\n" % L.SVD_HEAD in header and "#define VLM_SVD_MAX_SWEEPS %d\n" % L.SVD_MAX_SWEEPS in header
    # host-side functions of the shape alone (no device is touched)
    assert lib.vlm_svd_work_doubles(3, 5) == L.SVD_HEAD + 15 + 9 + 6 and lib.vlm_svd_work_doubles(5, 3) == 0
    assert [lib.vlm_svd_steps(p) for p in (0, 1, 2, 3, 8, 9)] == [0, 0, 1, 3, 7, 9]
    tsvm = importlib.import_module("vl_merging_amd.tsvm")
    with pytest.raises(L.VlmError):
        tsvm.TsvPlan("cpu")
    with pytest.raises(L.VlmError):
        tsvm.SvdPlan("cpu")
    assert 1 <= tsvm.SWEEPS <= L.SVD_MAX_SWEEPS and tsvm.POLAR_FLOOR == R.POLAR_FLOOR


def test_merge_ckpt_parses_tsvm(pkg):
    mc = merge_ckpt()
    assert "tsvm" in mc.METHODS
    args, cfg = mc.parse_args(["--method", "tsvm", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--central", "c.ckpt", "--lambda", "0.75",
                               "--report", "r.json", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.central, args.report) == ("tsvm", "c.ckpt", "r.json") and cfg["sum_lambda"] == 0.75
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "tsvm", "--ckpt", "a", "--out", "b", "--masks-out", "m.pt"])
    assert "--method tsvm" in mc.__doc__ and "tsvm_merge" in mc.__doc__ and ",tsvm," in mc.__doc__
