"""TSV-M on the GPU (csrc/jacobi.hip, csrc/tsvm.hip, tsvm.py): the batched Jacobi SVD alone against LAPACK, exact cases bit for
bit, the merge against the numpy restatement of the rule (tsvm_restatement.py), the dictionary walk and the command line.

The SVD's residuals are C p 2^-52 quantities.  The constants C below were taken after the first run on the MI355X, which printed the
device's residuals beside LAPACK's own on the same inputs: C is 8 times LAPACK's worst (docs/experiments.md, "TSV-M"; on the larger
shapes Jacobi's orthogonality residual is the larger one -- it accumulates a rotation's rounding per pair and sweep -- on the
small ones LAPACK's is).  The merge is held to a tolerance made per
input from the restatement's OWN noise: tol = max(16 spread, (p + q) 2^-52 s_max), spread = the difference between the
restatement's two orders, s_max = the largest singular value of any task vector."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, is_block, to_dev
import tsvm_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
U52 = 2.0 ** -52
# residual <= C * p * 2^-52 (singular values and the reconstruction: relative to s_max and ||A||_F).  C = 8 x LAPACK's own worst
# residual over these inputs in the same unit: 2.000 (U^T U - I), 1.500 (V V^T - I), 1.025 (reconstruction), 0.551 (its singular
# values of A against those of A^T).  The device's worst on the first run: 1.788, 0.250, 0.853, 0.607.  The constants were not
# retaken for the shapes past q = 512 and p = 256 (R.BOUNDARY_SKINNY, R.BOUNDARY_TALL), where the device's worst is 1.269, 0.667,
# 1.062, 1.306 and the restated sweep's 1.50, 1.50, 1.05, 1.15 (LAPACK's own: 1.333, 2.500, 2.212, 1.170).
C_ORTH_R, C_ORTH_V, C_RECON, C_SIGMA = 16.0, 12.0, 8.2, 4.4
ROW_KEYS = ["dst", "n", "shape", "transposed", "S", "k", "sweeps", "converged", "s_max", "s_kept_min", "s_dropped_max", "energy_kept",
            "dropped"]


@pytest.fixture(scope="module")
def tsvm(pkg):
    return importlib.import_module("vl_merging_amd.tsvm")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------ the primitive alone
def svd_run(tsvm, mats):
    plan = tsvm.SvdPlan("cuda")
    ids = [plan.add(dev(a)) for a in mats]
    plan.run()
    torch.cuda.synchronize()
    return [dict(R=plan.rt(j).cpu().numpy(), Vt=plan.vt(j).cpu().numpy(), s=plan.s(j).cpu().numpy(), rank=plan.rank(j).cpu().numpy(),
                 order=plan.order(j).cpu().numpy(), head=plan.head(j).cpu().numpy(), row=plan.rows[j]) for j in ids], plan


def figures(A0, got):
    """The residuals of one SVD in units of p 2^-52, the device's and LAPACK's own on the same input."""
    p = min(A0.shape)
    W = A0.T if A0.shape[0] > A0.shape[1] else A0
    Rm, Vt, s = got["R"], got["Vt"], got["s"]
    u, sl, vt = np.linalg.svd(W, full_matrices=False)
    live = s > 0
    fro = np.sqrt((W * W).sum())
    unit = p * U52
    dev_ = dict(orth_r=np.abs(Rm @ Rm.T - np.eye(p)).max() / unit,
                orth_v=(np.abs(Vt[live] @ Vt[live].T - np.eye(int(live.sum()))).max() if live.any() else 0.0) / unit,
                recon=(np.sqrt(((W - Rm.T @ (s[:, None] * Vt)) ** 2).sum()) / fro if fro else 0.0) / unit,
                sigma=(np.abs(np.sort(s)[::-1] - sl).max() / sl[0] if sl[0] else float(np.abs(s).max())) / unit)
    lap = dict(orth_r=np.abs(u.T @ u - np.eye(p)).max() / unit, orth_v=np.abs(vt @ vt.T - np.eye(p)).max() / unit,
               recon=(np.sqrt(((W - (u * sl) @ vt) ** 2).sum()) / fro if fro else 0.0) / unit,
               sigma=(np.abs(sl - np.linalg.svd(W.T, compute_uv=False)).max() / sl[0] if sl[0] else 0.0) / unit)
    return dev_, lap


def check_svd(A0, got, what):
    p, q = min(A0.shape), max(A0.shape)
    d, l = figures(A0, got)
    row = got["row"]
    print("svd %s %dx%d: sweeps %d; in p 2^-52: |RR^T-I| %.3f (lapack %.3f) |VV^T-I| %.3f (%.3f) recon %.3f (%.3f) sigma %.3f (%.3f)"
          % (what, p, q, row["sweeps"], d["orth_r"], l["orth_r"], d["orth_v"], l["orth_v"], d["recon"], l["recon"], d["sigma"], l["sigma"]))
    assert row["converged"] and (row["p"], row["q"], row["transposed"]) == (p, q, A0.shape[0] > A0.shape[1])
    assert row["sweeps"] == len(row["rotations"]) and (p == 1 or row["rotations"][-1] == 0)
    assert d["orth_r"] <= C_ORTH_R and d["orth_v"] <= C_ORTH_V and d["recon"] <= C_RECON and d["sigma"] <= C_SIGMA
    s, rank, order = got["s"], got["rank"], got["order"]
    assert sorted(rank.tolist()) == list(range(p)) and (order[rank] == np.arange(p)).all()
    ranked = s[order]
    assert (ranked[:-1] >= ranked[1:]).all() and got["head"][0] == ranked[0]
    for a in range(p - 1):   # ties in index order
        assert ranked[a] > ranked[a + 1] or order[a] < order[a + 1]
    assert (got["Vt"][s == 0] == 0).all() and got["head"][1] == int((s == 0).sum())
    return d, l


@pytest.mark.parametrize("p,q", R.SHAPES)
def test_svd_of_gaussian_matrices(p, q, tsvm):
    A0 = R.gaussian(p, q)
    (a, b), _ = svd_run(tsvm, [A0, A0.T.copy()])     # as given and tall: the same working set
    check_svd(A0, a, "gaussian")
    check_svd(A0.T, b, "tall")
    for key in ("R", "Vt", "s", "rank", "order"):        # (a square matrix is not transposed: its transpose is another input)
        assert p == q or a[key].tobytes() == b[key].tobytes(), key
    (again,), _ = svd_run(tsvm, [A0])                # two runs, identical bits
    assert all(a[key].tobytes() == again[key].tobytes() for key in ("R", "Vt", "s", "rank", "order", "head")) and a["row"] == again["row"]


@pytest.mark.parametrize("q", R.PAIR_Q)
def test_svd_of_duplicate_one_hot_pairs_in_every_instantiation(q, tsvm):
    """One q per instantiation of jacobi_step_kernel above PER = 1, entries at the first and last element of every register slot
    (tsvm_restatement.duplicate_pairs): exact, no tolerance.  A slot left out of the three sums leaves gamma = 0 and the pair
    unrotated (no zero row); a slot left out of the store leaves the row its old norm."""
    A0, C, v = R.duplicate_pairs(q)
    (got,), _ = svd_run(tsvm, [A0])
    row = got["row"]
    assert row["converged"] and row["sweeps"] == 2 and (row["p"], row["q"], row["transposed"]) == (2 * len(C), q, False)
    R.check_duplicate_pairs(C, v, got["s"], got["Vt"], got["R"], row["rotations"])
    assert got["head"][1] == len(C) and got["head"][0] == got["s"].max()


@pytest.mark.parametrize("p,q", R.BOUNDARY_SKINNY)
def test_svd_of_gaussian_matrices_at_the_long_rows(p, q, tsvm):
    """Every instantiation from PER = 4 up at its first and last q, against LAPACK under the constants above."""
    A0 = R.gaussian(p, q)
    (a, b), _ = svd_run(tsvm, [A0, A0.T.copy()])
    check_svd(A0, a, "long rows")
    check_svd(A0.T, b, "long rows, tall")
    for key in ("R", "Vt", "s", "rank", "order"):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("p,q", R.BOUNDARY_TALL)
def test_svd_of_gaussian_matrices_past_256_rows(p, q, tsvm):
    """p > 256: the rotation of R in a second register slot and the second trip of svd_rank_kernel's loops; 513 x 513 elements of
    R: svd_reset_kernel's grid at its cap."""
    ops = importlib.import_module("vl_merging_amd.ops")
    A0 = R.gaussian(p, q)
    # an adopted working set that holds NaN wherever the kernels do not write: a rank or an order entry that a loop skips is no
    # index then, whatever the allocator handed out
    work = torch.full((ops.svd_work_doubles(p, q),), float("nan"), dtype=torch.float64, device="cuda")
    ops.svd_views(work, p, q)[1].copy_(dev(A0))
    plan = tsvm.SvdPlan("cuda")
    j = plan.adopt(work, p, q)
    plan.run()
    torch.cuda.synchronize()
    a = dict(R=plan.rt(j).cpu().numpy(), Vt=plan.vt(j).cpu().numpy(), s=plan.s(j).cpu().numpy(), rank=plan.rank(j).cpu().numpy(),
             order=plan.order(j).cpu().numpy(), head=plan.head(j).cpu().numpy(), row=plan.rows[j])
    check_svd(A0, a, "tall rows")


@pytest.mark.parametrize("m,n", [(513, 513), (520, 513)])
def test_tsv_delta_bit_for_bit_past_the_grid_cap(m, n, tsvm):
    """m n > 256 workgroups x 1024 elements: the stride loop's second trip.  513 x 513 is odd (a tail of one element), 520 x 513
    is tall (stored transposed).  Two matrices a call; nothing but A is written."""
    L = importlib.import_module("vl_merging_amd._lib")
    ops = importlib.import_module("vl_merging_amd.ops")
    assert m * n > 256 * 1024 and (m * n) % 4 == (1 if m == n else 0)
    p, q = min(m, n), max(m, n)
    rng = np.random.default_rng(m + n)
    cs = [rng.standard_normal((m, n)).astype(F) for _ in range(2)]
    ss = [rng.standard_normal((m, n)).astype(F) for _ in range(2)]
    work = torch.full((2, ops.svd_work_doubles(p, q)), float("nan"), dtype=torch.float64, device="cuda")
    ops.tsv_delta([dev(c) for c in cs], [dev(s) for s in ss], [work[0], work[1]])
    torch.cuda.synchronize()
    got = work.cpu().numpy()
    for b in range(2):
        d = ss[b].astype(np.float64) - cs[b].astype(np.float64)
        d = np.ascontiguousarray(d.T) if m > n else d
        assert got[b, L.SVD_HEAD: L.SVD_HEAD + p * q].tobytes() == d.tobytes(), b
        assert np.isnan(got[b, :L.SVD_HEAD]).all() and np.isnan(got[b, L.SVD_HEAD + p * q:]).all(), b


def test_svd_rank_deficient_and_zero(tsvm):
    rng = np.random.default_rng(5)
    low = rng.standard_normal((33, 5)) @ rng.standard_normal((5, 70))        # rank 5 of 33
    dup = R.gaussian(8, 12)
    dup[5] = dup[2]                                                           # an exact copy: one rotation leaves an exact zero row
    zero = np.zeros((5, 7))
    (a, b, c), _ = svd_run(tsvm, [low, dup, zero])
    check_svd(low, a, "rank 5")
    assert (np.sort(a["s"])[::-1][5:] <= 33 * U52 * a["s"].max()).all()
    check_svd(dup, b, "duplicate row")
    assert int((b["s"] == 0).sum()) == 1
    check_svd(zero, c, "zero")
    assert c["row"]["sweeps"] == 1 and c["row"]["rotations"] == [0] and not c["s"].any() and not c["Vt"].any()
    assert c["rank"].tolist() == list(range(5)) and c["R"].tobytes() == np.eye(5).tobytes()


def test_svd_more_matrices_than_a_table_holds(tsvm):
    mats = [R.gaussian(4, 6, seed=i) for i in range(65)]
    outs, plan = svd_run(tsvm, mats)
    assert len(plan.groups) == 1 and len(plan.groups[0]["jobs"]) == 65
    for i in (0, 63, 64):                                                     # (64 in the first call of a step, 1 in the second)
        check_svd(mats[i], outs[i], "of 65")
        (one,), _ = svd_run(tsvm, [mats[i]])
        assert all(one[key].tobytes() == outs[i][key].tobytes() for key in ("R", "Vt", "s", "rank", "order")), i
    assert len({o["s"].tobytes() for o in outs}) == 65


def test_svd_argument_checks(tsvm):
    L = importlib.import_module("vl_merging_amd._lib")
    ops = importlib.import_module("vl_merging_amd.ops")
    plan = tsvm.SvdPlan("cuda")
    with pytest.raises(L.VlmError):
        plan.add(torch.zeros(4, 4, device="cuda"))                            # float32
    with pytest.raises(L.VlmError):
        plan.add(torch.zeros(1, L.SVD_MAX_Q + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(L.VlmError):
        plan.report()
    for bad in (dict(sweeps=0), dict(sweeps=L.SVD_MAX_SWEEPS + 1), dict(floor_rel=1.0)):
        with pytest.raises(ValueError):
            tsvm.SvdPlan("cuda", **bad)
    work = torch.zeros(ops.svd_work_doubles(4, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(L.VlmError):
        ops.svd_sweep([work[:-1]], 4, 6, 0)
    with pytest.raises(L.VlmError):
        ops.svd_sweep([work], 6, 4, 0)
    with pytest.raises(L.VlmError):
        ops.svd_sweep([work], 4, 6, L.SVD_MAX_SWEEPS)
    with pytest.raises(L.VlmError):
        ops.svd_sweep([work] * 65, 4, 6, 0)
    with pytest.raises(L.VlmError):
        ops.svd_finish([work], 4, 6, floor_rel=1.5)
    assert L.get_lib().vlm_svd_sweep(ops._ptr_list([work]), 1, L.SVD_MAX_Q + 1, 0, 1, None) == -4   # VLM_ERR_UNSUPPORTED
    assert tsvm.SvdPlan("cuda").run().report() == [] and tsvm.TsvPlan("cuda").run().report() == []


# ------------------------------------------------------------------------------------------------------ the merge
def run(tsvm, jobs):
    """jobs: (c, srcs, lam).  Returns (outputs, merged task vectors, report), the first two as numpy."""
    plan = tsvm.TsvPlan("cuda")
    outs = [plan.add([dev(s) for s in srcs], dev(c), lam=lam, name=str(i)) for i, (c, srcs, lam) in enumerate(jobs)]
    for o in outs:
        o.fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], [plan.task_vector(i).cpu().numpy() for i in range(len(jobs))], plan.report()


# ---- exact cases: bit for bit, no tolerance
@pytest.mark.parametrize("m,n,S", [(16, 24, 2), (24, 16, 2), (12, 12, 3), (30, 9, 3)])
@pytest.mark.parametrize("with_central", [False, True])
def test_exact_cases_bit_for_bit(m, n, S, with_central, tsvm):
    """Signed permutations times diagonals of distinct powers of two on disjoint supports: every row pair of every SVD is
    orthogonal with gamma = 0 exactly, nothing rotates, one sweep each, and the output is the closed-form sum as bytes."""
    c, srcs, total = R.exact_case(m, n, S, with_central=with_central)
    (got,), (T,), (row,) = run(tsvm, [(c, srcs, 1.0)])
    k = min(m, n) // S
    assert row["k"] == k and row["sweeps"] == {"tau": [1] * S, "U": 1, "V": 1}          # the minimum: one sweep that rotates nothing
    assert row["converged"] == {"tau": [True] * S, "U": True, "V": True}
    assert T.tobytes() == total.tobytes()
    assert got.tobytes() == total.astype(F).tobytes()
    assert row["dropped"] == ({"U": k, "V": k} if with_central else {"U": 0, "V": 0})
    live = S - 1 if with_central else S
    assert row["s_max"] == [1.0] * live + [0.0] * (S - live) and row["s_kept_min"][:live] == [2.0 ** -(k - 1)] * live
    assert row["s_dropped_max"] == [0.0] * S and row["energy_kept"] == [1.0] * S


def test_no_rank_to_share_gives_the_central_tensor(tsvm):
    c, srcs = R.planted(2, 9, 3)
    c2, srcs2 = R.planted(9, 2, 3)
    (a, b), (Ta, Tb), rows = run(tsvm, [(c, srcs, 0.75), (c2, srcs2, 1.0)])
    assert a.tobytes() == c.tobytes() and b.tobytes() == c2.tobytes() and not Ta.any() and not Tb.any()
    assert all(r["k"] == 0 and r["sweeps"] == {"tau": [], "U": None, "V": None} for r in rows) and sorted(rows[0]) == sorted(ROW_KEYS)


# ---- against the restatement
_REF = {}


def reference(m, n, S):
    """The restatement in both orders, computed once per input and left unchanged."""
    if (m, n, S) not in _REF:
        c, srcs = R.planted(m, n, S)
        a, b = R.tsvm(c, srcs, 1.0), R.tsvm(c, srcs, 1.0, flip=True)
        _REF[(m, n, S)] = dict(c=c, srcs=srcs, T=a["T"], k=a["k"], s=a["s"], dropped=a["dropped"],
                               spread=float(np.abs(a["T"] - b["T"]).max()), s_max=max(float(s[0]) for s in a["s"]))
    return _REF[(m, n, S)]


@pytest.mark.parametrize("lam", [0.75, 1.0])
@pytest.mark.parametrize("m,n,S", R.MERGE_CASES)
def test_against_the_restatement(m, n, S, lam, tsvm):
    against_the_restatement(m, n, S, lam, tsvm)


@pytest.mark.parametrize("m,n,S", R.BOUNDARY_MERGE)
def test_against_the_restatement_past_the_grid_caps(m, n, S, tsvm):
    """The same check at one size past the limits: tsv_delta's grid cap, several tiles of tsv_apply each way with a reduction
    kS = 512 and 513 (ragged by one against its 16-row stage), and the Jacobi kernels at p > 256, q > 512."""
    k = min(m, n) // S
    assert m * n > 256 * 1024 and k * S == (513 if S == 3 else 512) and min(m, n) > 256 and max(m, n) > 512
    against_the_restatement(m, n, S, 1.0, tsvm)


def against_the_restatement(m, n, S, lam, tsvm):
    ref = reference(m, n, S)
    c, srcs = ref["c"], ref["srcs"]
    p, q = min(m, n), max(m, n)
    (got,), (T,), (row,) = run(tsvm, [(c, srcs, lam)])
    tol = max(16 * ref["spread"], (p + q) * U52 * ref["s_max"])
    err = float(np.abs(T - ref["T"]).max())
    want = R.finish(c, ref["T"], lam)
    u = R.ulp_diff(got, want)
    print("tsvm %dx%d S=%d lam=%g k=%d: |T - T_ref| %.3e tol %.3e (err/tol %.3f; spread %.3e, s_max %.3e); fp32 differing %d max %d ulp; "
          "sweeps %s" % (m, n, S, lam, ref["k"], err, tol, err / tol, ref["spread"], ref["s_max"], int((u > 0).sum()), int(u.max()),
                         row["sweeps"]))
    assert sorted(row) == sorted(ROW_KEYS) and (row["dst"], row["n"], row["shape"], row["transposed"], row["S"], row["k"]) == \
        ("0", m * n, [m, n], m > n, S, ref["k"])
    assert T.dtype == np.float64 and T.shape == (m, n)
    assert err <= tol
    assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * c.size)
    assert got.tobytes() == R.finish(c, T, lam).tobytes()              # the output is fl32(c + lam * T), the device's own T
    if ref["k"]:
        k = ref["k"]
        assert all(row["converged"]["tau"]) and row["converged"]["U"] and row["converged"]["V"]
        assert row["dropped"] == {"U": ref["dropped"][0], "V": ref["dropped"][1]}
        for i, s in enumerate(ref["s"]):
            rel = (C_SIGMA + 1) * p * U52 * s[0]                        # the device's bound and one unit for LAPACK's own
            assert abs(row["s_max"][i] - s[0]) <= rel and abs(row["s_kept_min"][i] - s[k - 1]) <= rel
            assert abs(row["s_dropped_max"][i] - (s[k] if k < p else 0.0)) <= rel
            assert abs(row["energy_kept"][i] - (s[:k] ** 2).sum() / (s ** 2).sum()) <= 1e-12


def test_two_runs_same_bytes_same_report(tsvm):
    jobs = [(*R.planted(33, 70, 2), 0.75), (*R.planted(70, 33, 3), 1.0), (*R.planted(33, 70, 3, seed=1), 1.0), (*R.planted(8, 8, 2), 1.0)]
    seen = []
    for _ in range(2):
        outs, Ts, rows = run(tsvm, jobs)
        seen.append(([o.tobytes() for o in outs], [t.tobytes() for t in Ts], rows))
    assert seen[0] == seen[1]
    for i, job in enumerate(jobs):                                     # and a matrix in company is the matrix alone
        (one,), (T,), (row,) = run(tsvm, [job])
        assert one.tobytes() == seen[0][0][i] and T.tobytes() == seen[0][1][i] and {**row, "dst": str(i)} == seen[0][2][i]


# ---- aliasing
def test_dst_may_be_the_central_tensor_or_a_source(tsvm):
    for m, n in ((33, 70), (70, 33), (8, 8)):
        c, srcs = R.planted(m, n, 3)
        (want,), (T,), rows = run(tsvm, [(c, srcs, 0.75)])
        for which in ("base", 1):
            b, ds = dev(c), [dev(s) for s in srcs]
            out = b if which == "base" else ds[which]
            plan = tsvm.TsvPlan("cuda")
            got = plan.add(ds, b, lam=0.75, out=out, name="0")
            assert got.data_ptr() == out.data_ptr()
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want.tobytes(), (m, n, which)
            assert plan.report() == rows and plan.task_vector(0).cpu().numpy().tobytes() == T.tobytes()
            for k, s in enumerate(ds):
                if which != k:
                    assert s.cpu().numpy().tobytes() == srcs[k].tobytes()
            if which != "base":
                assert b.cpu().numpy().tobytes() == c.tobytes()


def test_plan_argument_checks(tsvm):
    L = importlib.import_module("vl_merging_amd._lib")
    plan = tsvm.TsvPlan("cuda")
    c = torch.zeros(4, 4, device="cuda")
    with pytest.raises(L.VlmError):
        plan.add([c] * 5, c)
    with pytest.raises(L.VlmError):
        plan.add([torch.zeros(4, 3, device="cuda")], c)
    with pytest.raises(L.VlmError):
        plan.add([torch.zeros(16, device="cuda")], torch.zeros(16, device="cuda"))
    with pytest.raises(L.VlmError):
        plan.add([c.double()], c)
    with pytest.raises(L.VlmError):
        plan.add([c], c, out=torch.zeros(4, 4))
    with pytest.raises(L.VlmError):
        plan.report()


# ------------------------------------------------------------------------------------------------------ the walk
def test_tsvm_merge_tiny_walks_as_isoc_does(tsvm):
    merge = importlib.import_module("vl_merging_amd.merge")
    isoc = importlib.import_module("vl_merging_amd.isoc")
    lam = 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES["all"])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {key: v.clone() for key, v in central.items()}
    rows, plans = [], []
    res = tsvm.tsvm_merge(sd, cfg, central_weight={"state_dict": central}, report_out=rows, plan_out=plans)
    ref = isoc.isoc_merge(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    for key, v in res.items():
        if is_block(key):
            assert v.data_ptr() != central[key].data_ptr()
        else:
            assert v is sd[key] and ref[key] is sd[key]
    by_dst = {r["dst"]: r for r in rows}
    n_mat, worst = 0, 0.0
    for i in range(12):
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            c, srcs = central_np[dst], [sd_np[src(m)] for m in mods]
            got = res[dst].cpu().numpy()
            if c.ndim != 2:                                            # bit-equal to the mean-task-vector job (and to Iso-C's)
                assert got.tobytes() == mo.taskvec(c, srcs, [lam / len(srcs)] * len(srcs)).tobytes(), dst
                assert got.tobytes() == ref[dst].cpu().numpy().tobytes() and dst not in by_dst
            else:
                n_mat += 1
                row = by_dst[dst]
                assert sorted(row) == sorted(ROW_KEYS) and row["shape"] == list(c.shape) and row["S"] == len(srcs)
                a, b = R.tsvm(c, srcs, lam), R.tsvm(c, srcs, lam, flip=True)
                T = plans[0].task_vector([j[0] for j in plans[0].jobs].index(dst)).cpu().numpy()
                tol = max(16 * float(np.abs(a["T"] - b["T"]).max()), sum(c.shape) * U52 * max(float(s[0]) for s in a["s"]))
                worst = max(worst, float(np.abs(T - a["T"]).max()) / tol)
                assert got.tobytes() == R.finish(c, T, lam).tobytes()
    # (printed, not asserted: the tiny state's Gaussian task vectors have no gap at the cut, so the truncation itself is ill-defined)
    print("tsvm tiny state: %d matrices, worst |T - T_ref| / tol %.3f" % (n_mat, worst))
    assert n_mat == len(rows) == 48
    assert all(torch.equal(central[key], central_before[key]) for key in central)   # the central tensors are inputs only
    assert isinstance(plans[0], tsvm.TsvPlan) and isinstance(plans[1], merge.MergePlan) and len(plans) == 2
    res2 = tsvm.tsvm_merge(sd, merge_cfg(sum_lambda=0.1), central_weight=central, lam=lam)   # an explicit lam wins
    torch.cuda.synchronize()
    assert all(res2[key].cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes() for key in res if is_block(key))
    cfg1 = merge_cfg(sum_lambda=lam, **CASES["used_vqa"])              # single-source layers take the ratio-1 job
    res3 = tsvm.tsvm_merge(sd, cfg1, central_weight=central)
    ref3 = isoc.isoc_merge(sd, cfg1, central_weight=central)
    torch.cuda.synchronize()
    for i in range(10, 12):
        for _, dst in mo._names(i):
            assert res3[dst].cpu().numpy().tobytes() == ref3[dst].cpu().numpy().tobytes(), dst
    with pytest.raises(KeyError):
        tsvm.tsvm_merge(sd, cfg, central_weight={k: v for k, v in central.items() if k != "transformer.blocks.3.mlp.fc1.weight"})


def test_merge_ckpt_tsvm_as_a_child_process(tsvm, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {key: torch.from_numpy(v) for key, v in tiny_state("all_moe").items()}
    central = {key: torch.from_numpy(v) for key, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "tsvm.ckpt", tmp_path / "tsvm.json"
    cmd = [sys.executable, TOOL, "--method", "tsvm", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.75", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = tsvm.tsvm_merge(to_dev(sd), merge_cfg(sum_lambda=0.75), central_weight=to_dev(central), report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for key in want:
        assert got[key].device.type == "cpu" and got[key].numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    assert rep["method"] == "tsvm" and rep["sum_lambda"] == 0.75 and rep["density"] is None
    mats = [t for t in rep["tensors"] if "shape" in t]
    assert len(mats) == 4 * 12 and mats == rows and len(rep["tensors"]) == 12 * 13
    assert all(sorted(t) == sorted(ROW_KEYS) for t in mats)
