"""Iso-C on the GPU (csrc/isoc.hip, the SYRK of csrc/f64ops.hip, isoc.py) against the numpy restatement of the rule
(isoc_restatement.py).  What is elementwise is held bit for bit: D, and the output given the device's own X and nuclear norm.  What
goes through the blocked factorisation and solve sums in another order than numpy and is held to a tolerance MEASURED per input:
8 times the error of the numpy iteration against the SVD, at least r * 2^-52, never above 1e-8 (RegMean's)."""
import importlib
import inspect
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, is_block, to_dev
import isoc_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
EPS = 2.0 ** -52
LAM = 0.75


@pytest.fixture(scope="module")
def isoc(pkg):
    return importlib.import_module("vl_merging_amd.isoc")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(isoc, jobs, **kw):
    """jobs: (c, srcs, lam).  Returns (outputs as numpy, report, plan)."""
    plan = isoc.IsoPlan("cuda", **kw)
    outs = [plan.add([dev(s) for s in srcs], dev(c), lam=lam, name=str(i)) for i, (c, srcs, lam) in enumerate(jobs)]
    for o in outs:
        o.fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], plan.report(), plan


def own(X, shape):
    """The device's X (working orientation) in the tensor's own orientation."""
    return X.T if shape[0] < shape[1] else X


_REF = {}


def reference(m, n, S):
    """Per row of SHAPES, computed once: inputs, the SVD definition, and the numpy iteration's error against it."""
    if (m, n, S) not in _REF:
        c, srcs = R.case(m, n, S)
        want, q, nuc = R.iso_svd(c, srcs, LAM)
        _, Xn, _, _ = R.iso_qdwh(c, srcs, LAM)
        _REF[(m, n, S)] = dict(c=c, srcs=srcs, want=want, q=q, nuc=nuc, cpu_err=float(np.abs(Xn - q).max()))
    return _REF[(m, n, S)]


def check_output(got, c, X_own, nuclear, lam, want):
    """Check 4: bit for bit finish() of the device's own X and nuclear; against the SVD at most 1 ulp in at most max(2, 1e-4 n)
    elements."""
    r = min(c.shape)
    assert got.tobytes() == R.finish(c, X_own, nuclear, lam, r).tobytes()
    u = R.ulp_diff(got, want)
    assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * c.size), (int(u.max()), int((u > 0).sum()))


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("m,n,S", R.SHAPES)
def test_delta_bit_for_bit_and_its_norm(m, n, S, ops):
    delta_bit_for_bit_and_its_norm(m, n, S, ops)


def crosses_the_limit(m, n):
    """A boundary shape is past the limit it is there for, by the library's own count of partials: more than the 64 a one-wave fold
    reads in one trip, or the cap of 256 workgroups with more than 2048 elements each."""
    parts = importlib.import_module("vl_merging_amd._lib").get_lib().vlm_iso_parts(m, n)
    if m * n > 256 * 2048:
        assert parts == 256 and (m * n) % 2 == 1
    else:
        assert parts == 65


@pytest.mark.parametrize("m,n,S", R.BOUNDARY_SHAPES)
def test_delta_bit_for_bit_and_its_norm_past_the_fold_and_the_cap(m, n, S, ops):
    crosses_the_limit(m, n)
    delta_bit_for_bit_and_its_norm(m, n, S, ops)


@pytest.mark.parametrize("m,n,S", R.BOUNDARY_SHAPES)
def test_polar_factor_nuclear_norm_and_output_past_the_fold_and_the_cap(m, n, S, isoc):
    crosses_the_limit(m, n)
    polar_factor_nuclear_norm_and_output(m, n, S, isoc)


def delta_bit_for_bit_and_its_norm(m, n, S, ops):
    L = importlib.import_module("vl_merging_amd._lib")
    ref = reference(m, n, S)
    c, srcs = ref["c"], ref["srcs"]
    N = m * n
    work = torch.full((2, L.ISO_HEAD + 3 * N), float("nan"), dtype=torch.float64, device="cuda")
    # two matrices in one launch: the second with the sources in reverse order
    base = [dev(c), dev(c)]
    lists = [[dev(srcs[k]), dev(srcs[S - 1 - k])] for k in range(S)]
    ops.iso_delta(base, lists, [work[0], work[1]], ops.iso_partials(m, n, 2, "cuda"))
    torch.cuda.synchronize()
    got = work.cpu().numpy()
    for b, order in enumerate((srcs, srcs[::-1])):
        d = R.working(R.delta(c, order))
        assert got[b, L.ISO_HEAD: L.ISO_HEAD + N].tobytes() == d.tobytes(), b          # D, transposed when m < n
        assert got[b, L.ISO_HEAD + 2 * N:].tobytes() == d.tobytes(), b                 # Y = D
        exact = math.fsum(float(v) * float(v) for v in d.ravel())
        assert abs(got[b, 0] - exact) <= (N + 2) * 2.0 ** -53 * exact, (got[b, 0], exact)
        assert np.isnan(got[b, 1: L.ISO_HEAD]).all() and np.isnan(got[b, L.ISO_HEAD + N: L.ISO_HEAD + 2 * N]).all()  # nothing else


@pytest.mark.parametrize("m,n,S", R.SHAPES)
def test_polar_factor_nuclear_norm_and_output(m, n, S, isoc):
    polar_factor_nuclear_norm_and_output(m, n, S, isoc)


def polar_factor_nuclear_norm_and_output(m, n, S, isoc):
    ref = reference(m, n, S)
    c, srcs = ref["c"], ref["srcs"]
    r = min(m, n)
    (got,), (row,), plan = run(isoc, [(c, srcs, LAM)])
    X = plan.factor(0).cpu().numpy()
    assert X.shape == (max(m, n), r) and plan.delta(0).cpu().numpy().tobytes() == R.working(R.delta(c, srcs)).tobytes()
    # check 2: the factor against U V^T, tolerance from the numpy iteration's own error
    tol = min(1e-8, max(8 * ref["cpu_err"], r * EPS))
    err = float(np.abs(own(X, (m, n)) - ref["q"]).max())
    live = np.abs(R.working(R.delta(c, srcs))).sum(axis=0) > 0
    orth = float(np.abs(X[:, live].T @ X[:, live] - np.eye(int(live.sum()))).max())
    fro = float(np.sqrt((R.delta(c, srcs) ** 2).sum()))
    nuc_tol = r * EPS * fro * math.sqrt(r)
    print("isoc %dx%d S=%d: |X - UV^T| gpu %.3e cpu %.3e tol %.3e; |X^T X - I| %.3e; nuclear err %.3e tol %.3e; steps %d last %.3e"
          % (m, n, S, err, ref["cpu_err"], tol, orth, abs(row["nuclear"] - ref["nuc"]), nuc_tol, row["steps"], row["last_step"]))
    assert err <= tol
    assert orth <= 1e-12
    # check 3
    assert abs(row["nuclear"] - ref["nuc"]) <= nuc_tol
    assert row == {"dst": "0", "n": m * n, "shape": [m, n], "transposed": m < n, "S": S, "fro": row["fro"], "nuclear": row["nuclear"],
                   "sigma_mean": row["nuclear"] / r, "steps": 8, "last_step": row["last_step"], "converged": True}
    assert abs(row["fro"] - fro) <= 1e-14 * fro and row["last_step"] <= 1e-10 * math.sqrt(r)
    # check 4
    check_output(got, c, own(X, (m, n)), row["nuclear"], LAM, ref["want"])
    if (m, n) == (130, 70):   # check 5: exact zero columns
        assert not live[5:9].any() and live.sum() == 66
        assert (X[:, 5:9] == 0.0).all() and got[:, 5:9].tobytes() == c[:, 5:9].tobytes()


def test_zero_task_vectors_give_the_central_tensor(isoc):
    c, srcs = R.inputs(48, 16, 3)
    c2, srcs2 = R.inputs(48, 16, 2, seed=1)
    outs, rows, plan = run(isoc, [(c, [c.copy() for _ in srcs], LAM), (c2, srcs2, LAM)])   # beside a live matrix of its group
    assert outs[0].tobytes() == c.tobytes() and not np.isnan(plan.factor(0).cpu().numpy()).any()
    assert (rows[0]["fro"], rows[0]["nuclear"], rows[0]["last_step"], rows[0]["converged"], rows[0]["steps"]) == (0.0, 0.0, 0.0, True, 8)
    assert not plan.factor(0).cpu().numpy().any()
    want, _, _ = R.iso_svd(c2, srcs2, LAM)
    check_output(outs[1], c2, plan.factor(1).cpu().numpy(), rows[1]["nuclear"], LAM, want)


def slow_inputs():
    """96 x 40 with singular values 1 .. 1e-9.  The central tensor is ZERO here: beside a Gaussian c of unit size the planted task
    vector would be rounded at c's ulp (6e-8) when the source c + D is formed in fp32, which lifts the smallest singular values to
    1e-7 of the largest -- and those the 8 scheduled steps do bring home (measured in numpy).  As fp32 holds it, the planted D keeps
    sigma_min / ||D||_F = 2.5e-9, far below l0 = 1e-6."""
    rng = np.random.default_rng(5)
    c = np.zeros((96, 40), F)
    return c, [R.planted_delta(96, 40, np.geomspace(1.0, 1e-9, 40), rng).astype(F), c.copy()]


def test_slow_spectrum_takes_the_extra_rounds(isoc):
    c, srcs = slow_inputs()
    d = R.delta(c, srcs)
    _, norms = R.qdwh(d)
    assert norms[-1] > 1e-10 * math.sqrt(40)               # the numpy iteration has not converged after the 8 steps either
    c2, srcs2 = R.inputs(96, 40, 2)                        # a well-conditioned matrix of the same group: it must not take them
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # converged inside the extra rounds: nothing is warned about
        outs, rows, plan = run(isoc, [(c, srcs, 1.0), (c2, srcs2, 1.0)])
    q, nuc = R.polar_svd(d)
    X = plan.factor(0).cpu().numpy()
    print("isoc slow 96x40: steps %d last %.3e |X - UV^T| %.3e" % (rows[0]["steps"], rows[0]["last_step"], np.abs(X - q).max()))
    assert rows[0]["converged"] is True and 8 < rows[0]["steps"] <= 40 and rows[0]["steps"] % 4 == 0
    assert rows[0]["last_step"] <= 1e-10 * math.sqrt(40)
    assert np.abs(X - q).max() <= 1e-6
    assert outs[0].tobytes() == R.finish(c, X, rows[0]["nuclear"], 1.0, 40).tobytes()
    assert rows[1]["steps"] == 8 and rows[1]["converged"] is True
    want2, _, _ = R.iso_svd(c2, srcs2, 1.0)
    check_output(outs[1], c2, plan.factor(1).cpu().numpy(), rows[1]["nuclear"], 1.0, want2)


@pytest.mark.parametrize("which", ["base", 0])
def test_slow_spectrum_with_dst_the_central_tensor_or_a_source(which, isoc):
    """The extra rounds and an output that IS an input: the central tensor is read by the apply pass, so a matrix is applied once,
    after its verdict.  Beside it a matrix of the same group that converges on schedule, aliased the same way.  Same bytes and
    report as the run without aliasing, which stands against the SVD in test_slow_spectrum_takes_the_extra_rounds."""
    jobs = [(*slow_inputs(), 1.0), (*R.inputs(96, 40, 2), 0.75)]
    want, rows, _ = run(isoc, jobs)
    assert rows[0]["steps"] > 8 and rows[1]["steps"] == 8
    plan = isoc.IsoPlan("cuda")
    held, outs = [], []
    for i, (c, srcs, lam) in enumerate(jobs):
        b, ds = dev(c), [dev(s) for s in srcs]
        out = b if which == "base" else ds[which]
        outs.append(plan.add(ds, b, lam=lam, out=out, name=str(i)))
        assert outs[-1].data_ptr() == out.data_ptr()
        held.append((b, ds))
    plan.run()
    torch.cuda.synchronize()
    assert plan.report() == rows
    for i, (c, srcs, _) in enumerate(jobs):
        assert outs[i].cpu().numpy().tobytes() == want[i].tobytes(), (which, i)
        b, ds = held[i]
        for k, s in enumerate(ds):
            if which != k:
                assert s.cpu().numpy().tobytes() == srcs[k].tobytes()
        if which != "base":
            assert b.cpu().numpy().tobytes() == c.tobytes()


def test_finish_phases(isoc, ops):
    """ISO_PHASE_NUCLEAR writes head[1] and no output; ISO_PHASE_APPLY writes the output from head[1] as it stands; both = one
    after the other."""
    L = importlib.import_module("vl_merging_amd._lib")
    c, srcs = R.inputs(48, 16, 2)
    (want,), (row,), plan = run(isoc, [(c, srcs, LAM)])
    work, part = [plan.groups[0]["work"][0].clone()], ops.iso_partials(48, 16, 1, "cuda")
    work[0][1] = float("nan")
    out = torch.full((48, 16), float("nan"), device="cuda")
    ops.iso_finish(work, [dev(c)], [out], LAM, part, L.ISO_PHASE_NUCLEAR)
    torch.cuda.synchronize()
    assert float(work[0][1]) == row["nuclear"] and bool(torch.isnan(out).all())
    work[0][1] = 2 * row["nuclear"]
    ops.iso_finish(work, [dev(c)], [out], LAM, part, L.ISO_PHASE_APPLY)
    torch.cuda.synchronize()
    assert float(work[0][1]) == 2 * row["nuclear"]
    assert out.cpu().numpy().tobytes() == R.finish(c, plan.factor(0).cpu().numpy(), 2 * row["nuclear"], LAM, 16).tobytes()
    ops.iso_finish(work, [dev(c)], [out], LAM, part)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    for bad in (0, 4, -1):
        with pytest.raises(L.VlmError):
            ops.iso_finish(work, [dev(c)], [out], LAM, part, bad)


def test_unconverged_matrix_is_written_and_reported(isoc, monkeypatch):
    """The loud path, reached through its own rule: with a tolerance no step norm meets, the matrix takes the 8 scheduled and all
    32 extra steps, is written as it stands -- here the converged factor --, reported with converged = False and warned about."""
    c, srcs = R.inputs(16, 16, 2)
    monkeypatch.setattr(isoc, "STEP_TOL", -1.0)
    with pytest.warns(UserWarning, match="Iso-C: the polar iteration of 0 has not converged after 40 steps"):
        (got,), (row,), plan = run(isoc, [(c, srcs, LAM)])
    assert row["converged"] is False and row["steps"] == 40
    want, _, _ = R.iso_svd(c, srcs, LAM)
    check_output(got, c, plan.factor(0).cpu().numpy(), row["nuclear"], LAM, want)


def dozen():
    jobs = []
    for i in range(6):
        c, srcs = R.inputs(48, 16, 2 + i % 3, seed=10 + i)
        jobs.append((c, srcs, [1.0, 0.75][i % 2]))
        c, srcs = R.inputs(16, 32, 2 + (i + 1) % 3, seed=20 + i)
        jobs.append((c, srcs, [0.75, 0.3][i % 2]))
    return jobs


def test_a_dozen_matrices_of_two_shapes_as_one_call_each(isoc):
    jobs = dozen()
    outs, rows, plan = run(isoc, jobs)
    assert len(plan.groups) == 2 and sorted(len(g["jobs"]) for g in plan.groups) == [6, 6]
    for i, job in enumerate(jobs):
        (one,), (row,), p1 = run(isoc, [job])
        assert one.tobytes() == outs[i].tobytes(), i
        assert p1.factor(0).cpu().numpy().tobytes() == plan.factor(i).cpu().numpy().tobytes(), i
        assert {**row, "dst": str(i)} == rows[i]
    c, srcs, lam = jobs[1]
    want, _, _ = R.iso_svd(c, srcs, lam)
    check_output(outs[1], c, plan.factor(1).cpu().numpy().T, rows[1]["nuclear"], lam, want)


def test_three_runs_same_bytes_same_report(isoc):
    jobs = dozen()[:4] + [(*R.case(130, 70, 2), LAM), (*slow_inputs(), 1.0)]
    seen = []
    for _ in range(3):
        outs, rows, plan = run(isoc, jobs)
        seen.append(([o.tobytes() for o in outs], [plan.factor(i).cpu().numpy().tobytes() for i in range(len(jobs))], rows))
    assert seen[0] == seen[1] == seen[2]


def test_dst_may_be_the_central_tensor_or_a_source(isoc):
    for m, n in ((48, 16), (16, 32), (5, 3)):
        c, srcs = R.inputs(m, n, 3)
        (want,), rows, _ = run(isoc, [(c, srcs, LAM)])
        for which in ("base", 1):
            b, ds = dev(c), [dev(s) for s in srcs]
            out = b if which == "base" else ds[which]
            plan = isoc.IsoPlan("cuda")
            got = plan.add(ds, b, lam=LAM, out=out, name="0")
            assert got.data_ptr() == out.data_ptr()
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want.tobytes(), (m, n, which)
            assert plan.report() == rows
            for k, s in enumerate(ds):
                if which != k:
                    assert s.cpu().numpy().tobytes() == srcs[k].tobytes()
            if which != "base":
                assert b.cpu().numpy().tobytes() == c.tobytes()


def test_argument_checks(isoc, ops):
    L = importlib.import_module("vl_merging_amd._lib")
    plan = isoc.IsoPlan("cuda")
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
    with pytest.raises(ValueError):
        isoc.IsoPlan("cuda", steps=9)
    work = torch.zeros(L.ISO_HEAD + 3 * 16, dtype=torch.float64, device="cuda")
    with pytest.raises(L.VlmError):
        ops.iso_delta([c], [[c]], [work[:-1]], ops.iso_partials(4, 4, 1, "cuda"))
    with pytest.raises(L.VlmError):
        ops.iso_delta([c], [[c]], [work], torch.zeros(0, dtype=torch.float64, device="cuda"))
    with pytest.raises(L.VlmError):
        ops.iso_step([work], 4, 4, 1.0, 1.0, L.ISO_MAX_STEPS, False, ops.iso_partials(4, 4, 1, "cuda"))
    with pytest.raises(L.VlmError):
        ops.iso_gram([work], 4, 4, [torch.zeros(3, 3, dtype=torch.float64, device="cuda")], 1.0, False)
    with pytest.raises(L.VlmError):
        ops.iso_finish([work], [c], [c[:, :2]], 1.0, ops.iso_partials(4, 4, 1, "cuda"))
    assert isoc.IsoPlan("cuda").run().report() == []


# ---------------------------------------------------------------------------------------------------------------- state dicts
def check_state(res, sd_np, central_np, cfg, lam, rows, factors):
    """Every block tensor of a merged tiny state against the rule."""
    by_dst = {r["dst"]: r for r in rows}
    n_mat = 0
    for i in range(12):
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            c, srcs = central_np[dst], [sd_np[src(m)] for m in mods]
            got = res[dst].cpu().numpy()
            assert got.shape == c.shape
            if len(mods) == 1:
                assert got.tobytes() == mo.taskvec(c, srcs, [1]).tobytes(), dst
                assert dst not in by_dst and dst not in factors
            elif c.ndim != 2:
                assert got.tobytes() == mo.taskvec(c, srcs, [lam / len(srcs)] * len(srcs)).tobytes(), dst
                assert dst not in by_dst and dst not in factors
            else:
                n_mat += 1
                row, X = by_dst[dst], factors[dst].cpu().numpy()
                assert X.dtype == np.float64 and X.shape == (max(c.shape), min(c.shape))
                assert (row["shape"], row["S"], row["transposed"], row["converged"]) == (list(c.shape), len(srcs), c.shape[0] < c.shape[1], True)
                want, _, nuc = R.iso_svd(c, srcs, lam)
                assert abs(row["nuclear"] - nuc) <= 1e-12 * nuc
                check_output(got, c, own(X, c.shape), row["nuclear"], lam, want)
    assert n_mat == len(rows) == len(factors)
    return n_mat


@pytest.mark.parametrize("case", sorted(CASES))
def test_isoc_merge_tiny_matches_the_rule(case, isoc):
    merge = importlib.import_module("vl_merging_amd.merge")
    cfg = merge_cfg(sum_lambda=LAM, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {key: v.clone() for key, v in central.items()}
    rows, plans, factors = [], [], {}
    res = isoc.isoc_merge(sd, cfg, central_weight={"state_dict": central}, report_out=rows, plan_out=plans, factors_out=factors)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    for key, v in res.items():
        if is_block(key):
            assert v.data_ptr() != central[key].data_ptr()
        else:
            assert v is sd[key]
    n_mat = check_state(res, sd_np, central_np, cfg, LAM, rows, factors)
    assert n_mat == {"all": 48, "used_irtr": 48, "used_vqa": 40}[case]
    assert all(torch.equal(central[key], central_before[key]) for key in central)   # the central tensors are inputs only
    assert isinstance(plans[0], isoc.IsoPlan) and isinstance(plans[1], merge.MergePlan) and len(plans) == 2
    if case == "all":   # fc1 and the transposed fc2 are one group; lam = None reads sum_lambda, an explicit lam wins
        assert sorted((g["shape"], len(g["jobs"])) for g in plans[0].groups) == [((16, 16), 12), ((32, 16), 24), ((48, 16), 12)]
        res2 = isoc.isoc_merge(sd, merge_cfg(sum_lambda=0.1), central_weight=central, lam=LAM)
        torch.cuda.synchronize()
        assert all(res2[key].cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes() for key in res if is_block(key))
    with pytest.raises(KeyError):
        isoc.isoc_merge(sd, cfg, central_weight={k: v for k, v in central.items() if k != "transformer.blocks.3.mlp.fc1.weight"})


def test_merge_ckpt_isoc_as_a_child_process(isoc, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {key: torch.from_numpy(v) for key, v in tiny_state("all_moe").items()}
    central = {key: torch.from_numpy(v) for key, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "iso.ckpt", tmp_path / "iso.json"
    cmd = [sys.executable, TOOL, "--method", "isoc", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.75", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = isoc.isoc_merge(to_dev(sd), merge_cfg(sum_lambda=0.75), central_weight=to_dev(central), report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for key in want:
        assert got[key].device.type == "cpu" and got[key].numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    assert rep["method"] == "isoc" and rep["sum_lambda"] == 0.75 and "merge_ratio" in rep and rep["density"] is None   # the keys stay
    mats = [t for t in rep["tensors"] if "shape" in t]
    assert len(mats) == 4 * 12 and mats == rows and len(rep["tensors"]) == 12 * 13
    assert all(t["converged"] is True and t["steps"] == 8 for t in mats)


def test_model_method_is_the_same_merge(isoc, pkg):
    """ViLTransformerSS.isoc_merge forwards to isoc.isoc_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    r_want, r_got, f_got = [], [], {}
    want = isoc.isoc_merge(sd, Stub.hparams.config, central_weight=central, report_out=r_want)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.isoc_merge(Stub(), sd, report_out=r_got, factors_out=f_got)
    torch.cuda.synchronize()
    assert all(got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes() for key in want if is_block(key))
    assert r_got == r_want and len(r_got) == 48 == len(f_got)
    ours = inspect.signature(isoc.isoc_merge).parameters
    theirs = inspect.signature(vm.ViLTransformerSS.isoc_merge).parameters
    assert all(theirs[p].default == ours[p].default for p in ("lam", "report_out", "factors_out"))
