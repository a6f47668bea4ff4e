"""WUDI on the GPU (csrc/wudi.hip, the products of csrc/f64ops.hip, wudi.py) against the numpy restatement of the rule
(wudi_restatement.py).  What is elementwise around the iteration is held bit for bit: the output given the device's own X_T.  The
iteration goes through matrix products that sum in another order than numpy and is held to a tolerance made per input from the
restatement's OWN noise: tol = min(2^-30 x0, max(16 spread, (n + T) 2^-52 x0)) with x0 = max |X_0| and spread = the difference
between the restatement's two summation orders.

Device against restatement as measured on the MI355X (max |X_T - X_ref| / tol per row of SHAPES at 40 steps): see
docs/experiments.md, "WUDI"."""
import importlib
import inspect
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, is_block, to_dev
import wudi_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
LAM = 0.75


@pytest.fixture(scope="module")
def wudi(pkg):
    return importlib.import_module("vl_merging_amd.wudi")


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(wudi, jobs, iters):
    """jobs: (c, srcs, lam).  Returns (outputs, states, report, plan), the first two as numpy."""
    plan = wudi.WudiPlan("cuda", iters=iters)
    outs = [plan.add([dev(s) for s in srcs], dev(c), lam=lam, name=str(i)) for i, (c, srcs, lam) in enumerate(jobs)]
    for o in outs:
        o.fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], [plan.state(i).cpu().numpy() for i in range(len(jobs))], plan.report(), plan


_REF = {}


def reference(c, srcs, lam, iters, key):
    """The restatement in both summation orders, computed once per key and left unchanged."""
    if key not in _REF:
        a, b = R.wudi(c, srcs, lam, iters), R.wudi(c, srcs, lam, iters, permute=True)
        _REF[key] = dict(a, spread=float(np.abs(a["X"] - b["X"]).max()), x0=float(np.abs(a["X0"]).max()))
    return _REF[key]


def check_matrix(got, X, row, c, srcs, lam, iters, ref, what):
    """Check 1 of one matrix: the device's fp64 state, fp32 output, losses and squared norms against the restatement."""
    m, n = c.shape
    tol = min(2.0 ** -30 * ref["x0"], max(16 * ref["spread"], (n + iters) * 2.0 ** -52 * ref["x0"]))
    err = float(np.abs(X - ref["X"]).max())
    u = R.ulp_diff(got, ref["out"])
    rel = [abs(row[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(row[k]) for k in ("loss_first", "loss_last")]
    print("wudi %s %dx%d S=%d T=%d: |X - X_ref| %.3e tol %.3e (spread %.3e, x0 %.3e); fp32 differing %d max %d ulp; loss rel %.1e %.1e; "
          "loss %.6e -> %.6e" % (what, m, n, len(srcs), iters, err, tol, ref["spread"], ref["x0"], int((u > 0).sum()), int(u.max()),
                                 rel[0], rel[1], row["loss_first"], row["loss_last"]))
    assert X.dtype == np.float64 and X.shape == (m, n)
    assert err <= tol
    assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * c.size)
    assert got.tobytes() == R.finish(c, X, lam).tobytes()              # the output is fl32(c + lam * state), the device's own state
    assert rel[0] <= 1e-9 and rel[1] <= 1e-9
    if iters > 1:
        assert row["loss_last"] < row["loss_first"]
    else:                                                              # one step: L(X_{T-1}) IS L(X_0)
        assert row["loss_last"] == row["loss_first"]
    assert len(row["sq"]) == len(srcs)
    for sq, t in zip(row["sq"], R.taus(c, srcs)):
        exact = math.fsum(float(v) * float(v) for v in t.ravel())
        assert abs(sq - exact) <= (t.size + 2) * 2.0 ** -53 * exact, (sq, exact)
    assert (row["n"], row["shape"], row["S"], row["iters"], row["lr"]) == (m * n, [m, n], len(srcs), iters, 1e-5)
    return err, tol


# ---------------------------------------------------------------------------------------------------------------- check 1
@pytest.mark.parametrize("iters", R.STEPS)
@pytest.mark.parametrize("m,n,S", R.SHAPES)
def test_against_the_restatement(m, n, S, iters, wudi):
    against_the_restatement(m, n, S, iters, wudi)


def boundary_counts(m, n):
    """(partials of an elementwise sum, tiles) of a shape from the library's own count, vlm_wudi_parts = partials + 2 tiles with
    64 x 64 tiles; the partials are those of the larger of [m][n] and [n][n]."""
    tiles = -(-m // 64) * -(-n // 64)
    return importlib.import_module("vl_merging_amd._lib").get_lib().vlm_wudi_parts(m, n) - 2 * tiles, tiles, n * max(m, n)


@pytest.mark.parametrize("case,iters", R.BOUNDARY_CASES)
def test_against_the_restatement_past_the_fold_and_the_cap(case, iters, wudi):
    m, n, S = case
    sums, tiles, N = boundary_counts(m, n)
    if m * n > 256 * 2048:   # the cap of 256 workgroups with more than 2048 elements each, and a loss fold over more than 64 tiles
        assert sums == 256 and N > 256 * 2048 and (m * n) % 2 == 1 and tiles == 144
    else:                    # a 65th partial for the one-wave fold
        assert sums == 65 and tiles == 36
    against_the_restatement(m, n, S, iters, wudi)


def against_the_restatement(m, n, S, iters, wudi):
    c, srcs = R.case(m, n, S)
    ref = reference(c, srcs, LAM, iters, (m, n, S, iters))
    (got,), (X,), (row,), _ = run(wudi, [(c, srcs, LAM)], iters)
    assert sorted(row) == sorted(["dst", "n", "shape", "S", "iters", "lr", "sq", "loss_first", "loss_last"]) and row["dst"] == "0"
    check_matrix(got, X, row, c, srcs, LAM, iters, ref, "case")


def test_the_default_step_count(wudi):
    (m, n, S), iters = R.LONG
    assert iters == 300 == inspect.signature(wudi.WudiPlan).parameters["iters"].default
    c, srcs = R.case(m, n, S)
    ref = reference(c, srcs, 1.0, iters, (m, n, S, iters))
    plan = wudi.WudiPlan("cuda")
    got = plan.add([dev(s) for s in srcs], dev(c), name="0")
    plan.run()
    torch.cuda.synchronize()
    check_matrix(got.cpu().numpy(), plan.state(0).cpu().numpy(), plan.report()[0], c, srcs, 1.0, iters, ref, "default")


# ---------------------------------------------------------------------------------------------------------------- check 2
def test_disjoint_supports_keep_the_sum(wudi):
    """Task vectors with disjoint column supports: tau_j tau_i^T = 0 exactly, X_0 is the minimiser; on the 2^-10 grid c + X_0 is
    a float32 and what 40 steps of rounding noise move (1e-11) cannot cross a rounding boundary (2^-22).  The output is held bit
    for bit to the plain sum c + sum_i tau_i, exact on the grid.  (The MERGE_TASKVEC job with ratios [1] * S cannot stand in for
    that sum: its rule is the recurrence acc += ratio * (src - acc), which with ratio 1 returns the LAST source.)"""
    m, n, S = 70, 48, 3
    c, draws = R.grid_inputs(m, n, S)
    srcs = []
    for i, d in enumerate(draws):
        s = c.copy()
        s[:, 16 * i: 16 * (i + 1)] = d[:, 16 * i: 16 * (i + 1)]
        srcs.append(s)
    (got,), (X,), (row,), _ = run(wudi, [(c, srcs, 1.0)], 40)
    x0 = R.wudi(c, srcs, 1.0, 1)["X0"]
    total = c.astype(np.float64) + x0
    assert np.array_equal(total, total.astype(F).astype(np.float64))   # the sum IS a float32
    assert got.tobytes() == total.astype(F).tobytes()
    for i in range(S):                                                 # and per support it is that expert's tensor
        assert got[:, 16 * i: 16 * (i + 1)].tobytes() == srcs[i][:, 16 * i: 16 * (i + 1)].tobytes()
    print("wudi disjoint supports: |X_40 - X_0| %.3e, losses %.3e %.3e" % (np.abs(X - x0).max(), row["loss_first"], row["loss_last"]))
    assert np.abs(X - x0).max() <= 1e-9


def test_one_expert_at_the_central_tensor_gives_the_other(wudi):
    c, (w, _) = R.grid_inputs(40, 24, 2)
    for srcs in ([c.copy(), w], [w, c.copy()]):
        (got,), _, (row,), _ = run(wudi, [(c, srcs, 1.0)], 40)
        assert got.tobytes() == w.tobytes()
        assert sorted(row["sq"])[0] == 0.0 and sorted(row["sq"])[1] > 0.0


def test_zero_task_vectors_give_the_central_tensor(wudi):
    c, srcs = R.grid_inputs(48, 16, 3)
    c2, srcs2 = R.inputs(48, 16, 3, seed=1)
    outs, states, rows, _ = run(wudi, [(c, [c.copy() for _ in srcs], LAM), (c2, srcs2, LAM)], 7)   # beside a live matrix of its group
    assert outs[0].tobytes() == c.tobytes() and not states[0].any()
    assert (rows[0]["loss_first"], rows[0]["loss_last"], rows[0]["sq"]) == (0.0, 0.0, [0.0, 0.0, 0.0])
    assert not np.isnan(outs[0]).any() and not np.isnan(states[0]).any()
    ref = reference(c2, srcs2, LAM, 7, "zero-neighbour")
    check_matrix(outs[1], states[1], rows[1], c2, srcs2, LAM, 7, ref, "beside zero")


def test_dst_may_be_the_central_tensor_or_a_source(wudi):
    for m, n in ((48, 16), (16, 80), (5, 3)):
        c, srcs = R.inputs(m, n, 3)
        (want,), (state,), rows, _ = run(wudi, [(c, srcs, LAM)], 7)
        for which in ("base", 1):
            b, ds = dev(c), [dev(s) for s in srcs]
            out = b if which == "base" else ds[which]
            plan = wudi.WudiPlan("cuda", iters=7)
            got = plan.add(ds, b, lam=LAM, out=out, name="0")
            assert got.data_ptr() == out.data_ptr()
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want.tobytes(), (m, n, which)
            assert plan.report() == rows and plan.state(0).cpu().numpy().tobytes() == state.tobytes()
            for k, s in enumerate(ds):
                if which != k:
                    assert s.cpu().numpy().tobytes() == srcs[k].tobytes()
            if which != "base":
                assert b.cpu().numpy().tobytes() == c.tobytes()


# ---------------------------------------------------------------------------------------------------------------- check 3
def same_as_singles(wudi, jobs, iters):
    outs, states, rows, plan = run(wudi, jobs, iters)
    for i, job in enumerate(jobs):
        (one,), (st,), (row,), _ = run(wudi, [job], iters)
        assert one.tobytes() == outs[i].tobytes(), i
        assert st.tobytes() == states[i].tobytes(), i
        assert {**row, "dst": str(i)} == rows[i]
    return plan


def test_two_matrices_of_one_shape(wudi):
    a, b = R.inputs(80, 48, 2, seed=1), R.inputs(80, 48, 2, seed=2)
    plan = same_as_singles(wudi, [(*a, 1.0), (*b, 0.3)], 7)
    assert len(plan.groups) == 1


def test_more_matrices_than_a_table_holds(wudi):
    jobs = [(*R.inputs(8, 8, 2, seed=i), 1.0) for i in range(66)]
    outs, states, rows, plan = run(wudi, jobs, 3)
    assert len(plan.groups) == 1 and len(plan.groups[0]["jobs"]) == 66
    for i in range(66):                                                # (64 in the first call of a step, 2 in the second)
        (one,), (st,), (row,), _ = run(wudi, [jobs[i]], 3)
        assert one.tobytes() == outs[i].tobytes() and st.tobytes() == states[i].tobytes() and {**row, "dst": str(i)} == rows[i], i
    keys = [o.tobytes() for o in outs]
    assert len(set(keys)) == 66 and not any(np.isnan(o).any() for o in outs)


def test_four_shapes_on_side_streams(wudi):
    jobs = [(*R.inputs(m, n, S, seed=3), lam) for (m, n, S, lam) in ((80, 48, 2, 1.0), (48, 80, 3, 0.75), (16, 16, 2, 1.0), (67, 1, 3, 0.3),
                                                                    (80, 48, 3, 0.75), (16, 16, 4, 1.0))]
    plan = same_as_singles(wudi, jobs, 7)
    assert sorted((g["shape"], len(g["jobs"])) for g in plan.groups) == [((16, 16), 2), ((48, 80), 1), ((67, 1), 1), ((80, 48), 2)]


# ---------------------------------------------------------------------------------------------------------------- check 4
def test_two_runs_same_bytes_same_report(wudi):
    jobs = [(*R.case(130, 70, 2), LAM), (*R.case(48, 80, 3), 1.0), (*R.inputs(130, 70, 3, seed=4), 1.0)]
    seen = []
    for _ in range(2):
        outs, states, rows, _ = run(wudi, jobs, 40)
        seen.append(([o.tobytes() for o in outs], [s.tobytes() for s in states], rows))
    assert seen[0] == seen[1]


# ---------------------------------------------------------------------------------------------------------------- check 5
def test_argument_checks(wudi, ops):
    L = importlib.import_module("vl_merging_amd._lib")
    plan = wudi.WudiPlan("cuda")
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
    for bad in (dict(iters=0), dict(iters=2.5), dict(lr=0.0), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            wudi.WudiPlan("cuda", **bad)
    work = torch.zeros(ops.wudi_work_doubles(4, 4), dtype=torch.float64, device="cuda")
    part = ops.wudi_partials(4, 4, 1, "cuda")
    with pytest.raises(L.VlmError):
        ops.wudi_prepare([c], [[c]], [work[:-1]], part)
    with pytest.raises(L.VlmError):
        ops.wudi_prepare([c], [[c]], [work], torch.zeros(0, dtype=torch.float64, device="cuda"))
    with pytest.raises(L.VlmError):
        ops.wudi_prepare([c], [[c], [c, c]], [work], part)
    with pytest.raises(L.VlmError):
        ops.wudi_step([work], 4, 4, 0, 1e-5, 1.0, part)
    with pytest.raises(L.VlmError):
        ops.wudi_step([work], 4, 4, 1, 0.0, 1.0, part)
    with pytest.raises(L.VlmError):
        ops.wudi_step([work] * 65, 4, 4, 1, 1e-5, 1.0, part)
    with pytest.raises(L.VlmError):
        ops.wudi_finish([work], [c], [c[:, :2]], 1, 1, 1.0, part)
    with pytest.raises(L.VlmError):
        ops.wudi_finish([work], [c], [c], 1, 0, 1.0, part)
    assert wudi.WudiPlan("cuda").run().report() == []


# ---------------------------------------------------------------------------------------------------------------- check 6
ITERS = 40


def check_state(res, sd_np, central_np, cfg, lam, rows, states, case):
    """Every block tensor of a merged tiny state against the rule."""
    by_dst = {r["dst"]: r for r in rows}
    n_mat, worst = 0, 0.0
    for i in range(12):
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            c, srcs = central_np[dst], [sd_np[src(m)] for m in mods]
            got = res[dst].cpu().numpy()
            assert got.shape == c.shape
            if len(mods) == 1:
                assert got.tobytes() == mo.taskvec(c, srcs, [1]).tobytes(), dst
                assert dst not in by_dst and dst not in states
            elif c.ndim != 2:
                assert got.tobytes() == mo.taskvec(c, srcs, [lam / len(srcs)] * len(srcs)).tobytes(), dst
                assert dst not in by_dst and dst not in states
            else:
                n_mat += 1
                ref = reference(c, srcs, lam, ITERS, (case, dst))
                err, tol = check_matrix(got, states[dst].cpu().numpy(), by_dst[dst], c, srcs, lam, ITERS, ref, dst)
                worst = max(worst, err / tol)
    assert n_mat == len(rows) == len(states)
    print("wudi tiny state %s: %d matrices, worst |X - X_ref| / tol %.3f" % (case, n_mat, worst))
    return n_mat


@pytest.mark.parametrize("case", sorted(CASES))
def test_wudi_merge_tiny_matches_the_rule(case, wudi):
    merge = importlib.import_module("vl_merging_amd.merge")
    cfg = merge_cfg(sum_lambda=LAM, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {key: v.clone() for key, v in central.items()}
    rows, plans, states = [], [], {}
    res = wudi.wudi_merge(sd, cfg, central_weight={"state_dict": central}, report_out=rows, plan_out=plans, states_out=states,
                          iters=ITERS)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    for key, v in res.items():
        if is_block(key):
            assert v.data_ptr() != central[key].data_ptr()
        else:
            assert v is sd[key]
    n_mat = check_state(res, sd_np, central_np, cfg, LAM, rows, states, case)
    assert n_mat == {"all": 48, "used_irtr": 48, "used_vqa": 40}[case]
    assert all(torch.equal(central[key], central_before[key]) for key in central)   # the central tensors are inputs only
    assert isinstance(plans[0], wudi.WudiPlan) and isinstance(plans[1], merge.MergePlan) and len(plans) == 2
    if case == "all":   # grouped by the exact shape: fc1 [32, 16] and fc2 [16, 32] apart; lam = None reads sum_lambda, an explicit lam wins
        assert sorted((g["shape"], len(g["jobs"])) for g in plans[0].groups) == [((16, 16), 12), ((16, 32), 12), ((32, 16), 12), ((48, 16), 12)]
        res2 = wudi.wudi_merge(sd, merge_cfg(sum_lambda=0.1), central_weight=central, lam=LAM, iters=ITERS)
        res3 = wudi.wudi_merge(sd, merge_cfg(sum_lambda=LAM), central_weight=central, iters=ITERS)
        torch.cuda.synchronize()
        for other in (res2, res3):
            assert all(other[key].cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes() for key in res if is_block(key))
    with pytest.raises(KeyError):
        wudi.wudi_merge(sd, cfg, central_weight={k: v for k, v in central.items() if k != "transformer.blocks.3.mlp.fc1.weight"},
                        iters=ITERS)


# ---------------------------------------------------------------------------------------------------------------- check 7
def test_merge_ckpt_wudi_as_a_child_process(wudi, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {key: torch.from_numpy(v) for key, v in tiny_state("all_moe").items()}
    central = {key: torch.from_numpy(v) for key, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "wudi.ckpt", tmp_path / "wudi.json"
    cmd = [sys.executable, TOOL, "--method", "wudi", "--wudi-iters", "40", "--wudi-lr", "2e-5", "--ckpt", str(tmp_path / "moe.ckpt"),
           "--out", str(out), "--report", str(rep), "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.75", "with",
           "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = wudi.wudi_merge(to_dev(sd), merge_cfg(sum_lambda=0.75), central_weight=to_dev(central), report_out=rows, iters=40, lr=2e-5)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for key in want:
        assert got[key].device.type == "cpu" and got[key].numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    assert rep["method"] == "wudi" and rep["sum_lambda"] == 0.75 and "merge_ratio" in rep and rep["density"] is None   # the keys stay
    iso_keys = {"method", "density", "drop", "seed", "dare_mode", "gamma", "band_mode", "epsilon", "della_mode", "rescale", "sphere_on",
                "sphere_rows", "tall_lambda", "consensus_k", "sum_lambda", "merge_ratio", "tensors"}
    assert set(rep) == iso_keys
    mats = [t for t in rep["tensors"] if "shape" in t]
    assert len(mats) == 4 * 12 and mats == rows and len(rep["tensors"]) == 12 * 13
    assert all(t["iters"] == 40 and t["lr"] == 2e-5 and t["loss_first"] > t["loss_last"] for t in mats)


def test_model_method_is_the_same_merge(wudi, pkg):
    """ViLTransformerSS.wudi_merge forwards to wudi.wudi_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    r_want, r_got, s_got = [], [], {}
    want = wudi.wudi_merge(sd, Stub.hparams.config, central_weight=central, report_out=r_want, iters=7)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.wudi_merge(Stub(), sd, report_out=r_got, states_out=s_got, iters=7)
    torch.cuda.synchronize()
    assert all(got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes() for key in want if is_block(key))
    assert r_got == r_want and len(r_got) == 48 == len(s_got)
    ours = inspect.signature(wudi.wudi_merge).parameters
    theirs = inspect.signature(vm.ViLTransformerSS.wudi_merge).parameters
    assert list(theirs) == ["self", "state_dict", "lam", "report_out", "states_out", "iters", "lr"]
    assert all(theirs[p].default == ours[p].default for p in ("lam", "report_out", "states_out", "iters", "lr"))
