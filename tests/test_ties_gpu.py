"""TIES merge on the GPU (csrc/ties.hip through the C ABI) against the numpy restatement of the rule (ties_restatement.py): every
comparison is over ALL elements and bit for bit.  The reference has no TIES; only the single-source layers of the vqa case can be
(and are) tied to the task-vector merge the reference's goldens pin."""
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
from ties_restatement import keep_count, ties

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def to_dev(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items()}


def is_block(k):
    return "transformer.blocks." in k and "gamma" not in k


def restate_state(sd, central, cfg, density, lam, layers=range(12)):
    """dst -> (expected tensor, info | None) for the block tensors of `layers`; single-source layers: the oracle's task-vector job."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None)
            else:
                out, info = ties(central[dst], srcs, density, lam)
                exp[dst] = (out.reshape(central[dst].shape), info)
    return exp


def check_report(rows, exp, density):
    by_dst = {r["dst"]: r for r in rows}
    assert sorted(by_dst) == sorted(k for k, (_, info) in exp.items() if info is not None)
    for dst, r in by_dst.items():
        info = exp[dst][1]
        assert r["threshold_bits"] == info["threshold_bits"], dst
        assert [np.float32(t).tobytes() for t in r["threshold"]] == [np.float32(t).tobytes() for t in info["threshold"]], dst
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), dst
        assert r["n"] == exp[dst][0].size and r["K"] == [keep_count(density, exp[dst][0].size)] * len(r["kept"])


CASES = {
    "all": dict(),
    "used_irtr": dict(only_activate_used_experts=True, loss_names={"irtr": 1}),
    "used_vqa": dict(only_activate_used_experts=True, loss_names={"vqa": 1}),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("lam", [1, 0.75])
@pytest.mark.parametrize("density", [0.05, 0.2, 1.0])
def test_ties_merge_tiny_matches_restatement(density, lam, case, merge):
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {k: v.clone() for k, v in central.items()}
    rows, plans = [], []
    res = merge.ties_merge(sd, cfg, central_weight={"state_dict": central}, density=density, report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, density, lam)
    n_block = 0
    for k, v in res.items():
        if is_block(k):
            assert v.cpu().numpy().tobytes() == exp[k][0].tobytes(), k
            assert v.shape == central[k].shape and v.data_ptr() != central[k].data_ptr()
            if exp[k][1] is None:  # one source: the task-vector job with ratio 1, as sum_task_vectors issues it
                assert v.cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), k
            n_block += 1
        else:
            assert v is sd[k]
    assert n_block == 12 * 13
    assert all(torch.equal(central[k], central_before[k]) for k in central)  # the central tensors are inputs only
    check_report(rows, exp, density)
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.TiesPlan)
    # lam=None takes config["sum_lambda"]
    res2 = merge.ties_merge(sd, cfg, central_weight=central, density=density)
    torch.cuda.synchronize()
    assert all(res2[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes() for k in res if is_block(k))


def planted(n, S, seed):
    """Half the elements on a coarse dyadic grid (task vectors are exact multiples of 1/8: many equal magnitudes -- ties wherever
    the K-th place falls --, exact cancellations t_0 = -t_1, zeros), half ordinary floats; -0.0 task-vector entries up front."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(n).astype(F)
    srcs = [(c + rng.standard_normal(n).astype(F) * F(0.1)).astype(F) for _ in range(S)]
    grid = np.arange(n) % 2 == 0
    cg = (rng.integers(-16, 17, n) / 8).astype(F)
    c[grid] = cg[grid]
    for m in range(S):
        tg = (rng.integers(-16, 17, n) / 8).astype(F)
        srcs[m][grid] = (cg + tg)[grid]  # exact: small dyadic numbers
    cancel = np.arange(n) % 6 == 0
    srcs[1][cancel] = (c - (srcs[0] - c))[cancel]  # on the grid this is exact: t_1 = -t_0
    k = min(n, 3)
    c[:k] = 0.0
    srcs[0][:k] = -0.0  # (-0.0) - (+0.0) = -0.0
    if n > 8:
        blk = slice(4, 8)  # a block of equal magnitudes with mixed signs
        c[blk] = 0.0
        for m in range(S):
            srcs[m][blk] = np.array([0.75, -0.75, 0.75, -0.75], F) * (1 if m != 1 else -1)
    return c, srcs


def run_plan(merge, jobs):
    """jobs: list of (c, srcs, density, lam).  Returns (outputs, report rows, plan)."""
    plan = merge.TiesPlan("cuda")
    outs = [plan.add([torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(c).cuda(), density=density, lam=lam, name=str(i))
            for i, (c, srcs, density, lam) in enumerate(jobs)]
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def check_jobs(jobs, outs, rows):
    for i, (c, srcs, density, lam) in enumerate(jobs):
        exp, info = ties(c, srcs, density, lam)
        assert outs[i].cpu().numpy().tobytes() == exp.tobytes(), (i, c.size)
        r = rows[i]
        assert r["dst"] == str(i) and r["n"] == c.size and r["K"] == [keep_count(density, c.size)] * len(srcs)
        assert r["threshold_bits"] == info["threshold_bits"], i
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), i


SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 1 << 20]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("density", ["one_over_n", 0.2, 1.0])
def test_ties_ragged_sizes(n, S, density, merge):
    d = 1.0 / n if density == "one_over_n" else density
    c, srcs = planted(n, S, seed=n + S)
    jobs = [(c, srcs, d, 0.75)]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)


def test_ties_several_jobs_in_one_plan_and_ties_at_the_threshold(merge):
    jobs = []
    for i, n in enumerate([12289, 1, 4097, 3, 1 << 20, 5, 8191, 4096, 70000, 1023]):
        c, srcs = planted(n, 2 + i % 2, seed=100 + i)
        jobs.append((c, srcs, [0.2, 0.05, 1.0][i % 3], [1, 0.75][i % 2]))
    # one source (trimmed, unlike ties_merge's single-source layers) and four sources with ragged tails / tiny sizes
    rng = np.random.default_rng(8)
    for n, S in ((4099, 1), (3, 1), (1 << 16, 1), (12291, 4), (8193, 4), (2, 4), (5, 4)):
        c, srcs = planted(n, max(S, 2), seed=200 + n)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(F) * F(0.3)).astype(F))
        jobs.append((c, srcs[:S], [0.2, 0.05, 1.0][n % 3], 0.75))
    # pure grid data: every threshold is a tie
    rng = np.random.default_rng(9)
    cg = (rng.integers(-16, 17, 50000) / 8).astype(F)
    jobs.append((cg, [(cg + (rng.integers(-16, 17, 50000) / 8).astype(F)) for _ in range(4)], 0.3, 1))
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert all(k > K for k, K in zip(rows[-1]["kept"], rows[-1]["K"]))  # all ties at the threshold are kept
    assert rows[-1]["conflict"] > 0 and rows[-1]["empty"] > 0


def test_ties_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one-chunk jobs (lengths cycled through 5, 1, 4097, 3, 2, 4099; 1 .. 4 sources; density and lambda
    cycled as above), every input a 16-byte aligned view into one device buffer: each workgroup of a histogram pass (4 per CU)
    owns about seven chunks and each of the apply pass (12 per CU) three, every one of another job -- so a run leaves a job,
    flushes and loads the next job's prefixes or thresholds at every step, which plans below the grid size (one chunk per
    workgroup) never do.  Outputs, thresholds and every counter against the restatement."""
    jobs = [(c, srcs, [0.2, 0.05, 1.0][i % 3], [1, 0.75][i % 2])
            for i, (c, srcs) in enumerate(tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted))]
    views = iter(one_buffer([a for c, srcs, _, _ in jobs for a in [c] + srcs]))
    plan = merge.TiesPlan("cuda")
    outs = []
    for i, (c, srcs, density, lam) in enumerate(jobs):
        base = next(views)
        outs.append(plan.add([next(views) for _ in srcs], base, density=density, lam=lam, name=str(i)))
        assert plan.jobs[-1].base == base.data_ptr()  # the view itself, not a staged copy
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, outs, plan.report())


def test_ties_constant_and_all_zero_task_vectors(merge):
    n = 5000
    c = np.linspace(-1, 1, n).astype(F)
    cz = np.zeros(n, F)
    jobs = [(cz, [np.full(n, 0.5, F), np.full(n, 0.5, F)], 0.2, 1),                             # every key equal: the threshold is that key, everything kept
            (cz, [np.full(n, 0.5, F), np.full(n, -0.25, F)], 0.01, 0.75),
            (c, [c.copy(), c.copy(), c.copy()], 0.2, 1)]           # task vectors all +0.0: thresholds 0, out = c
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert rows[0]["kept"] == [n, n] and rows[0]["threshold"] == [0.5, 0.5] and rows[0]["empty"] == 0
    assert outs[0].cpu().numpy().tobytes() == np.full(n, 0.5, F).tobytes()
    assert rows[1]["kept"] == [n, n] and rows[1]["conflict"] == n
    assert rows[2]["threshold_bits"] == [0, 0, 0] and rows[2]["kept"] == [n] * 3 and rows[2]["empty"] == n
    assert outs[2].cpu().numpy().tobytes() == (c + F(1) * np.zeros(n, F)).tobytes()


def test_ties_run_twice_same_bytes_same_counters(merge):
    jobs = [planted(n, S, seed=n) + (0.2, 0.75) for n, S in ((70001, 3), (4097, 2), (3, 2))]
    jobs = [(c, srcs, d, lam) for c, srcs, d, lam in jobs]
    outs, rows, plan = run_plan(merge, jobs)
    first = [o.cpu().numpy().tobytes() for o in outs]
    for o in outs:
        o.fill_(float("nan"))
    plan.run()
    plan.run()
    torch.cuda.synchronize()
    assert [o.cpu().numpy().tobytes() for o in outs] == first
    assert plan.report() == rows
    check_jobs(jobs, outs, rows)


def test_ties_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    plan = merge.TiesPlan("cuda")
    a = torch.zeros(64, device="cuda")
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, density=0.5)
    with pytest.raises(L.VlmError):
        plan.add([a, torch.zeros(32, device="cuda")], a, density=0.5)
    with pytest.raises(L.VlmError):
        plan.add([a.double()], a, density=0.5)
    out = plan.add([a + 1, a + 2], a, density=0.5)
    lib = L.get_lib()
    arr = (L.TiesJob * 1)(*plan.jobs)
    ws = torch.empty(lib.vlm_ties_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    assert lib.vlm_ties_plan_upload(arr, 1, L.ptr(ws), 1024, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [1.5] * 64


def test_ties_base_size(merge):
    """Base size (the inputs of test_merge_base_size_digests), density 0.2: layers 0 (two sources) and 11 (three) against the
    restatement bit for bit, every other output finite; and run() returns while its launches are still queued."""
    L = importlib.import_module("vl_merging_amd._lib")
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    plans, rows = [], []
    res = merge.ties_merge(sd, cfg, central_weight=central, density=0.2, plan_out=plans, report_out=rows)
    torch.cuda.synchronize()
    plan = plans[0]
    n_out = sum(v.numel() for k, v in res.items() if is_block(k))
    assert plan.bytes_written == 4 * n_out == 340180992
    # four passes (three of the selection, one apply), each reads every source and the central tensor once
    assert plan.bytes_read == 4 * 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs) == 4 * (737058816 + 340180992)
    exp = restate_state(sd_np, central_np, cfg, 0.2, 0.75, layers=(0, 11))
    by_dst = {r["dst"]: r for r in rows}
    for k, (want, info) in exp.items():
        assert res[k].cpu().numpy().tobytes() == want.tobytes(), k
        r = by_dst[k]
        assert r["threshold_bits"] == info["threshold_bits"], k
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), k
    assert len(rows) == 12 * 13
    for k, v in res.items():
        if is_block(k):
            assert bool(torch.isfinite(v).all()), k
    # no host synchronisation between upload and the end of run(): the ENQUEUE is timed behind a 0.2 s spin kernel on the same
    # stream.  Any stream or device synchronisation inside run() has to wait the spin out, so run() would take >= 0.2 s; seven
    # asynchronous launches take well under a millisecond.  The spin's own length is checked, so the bound cannot pass vacuously.
    import time
    first = {k: res[k].clone() for k in exp}
    torch.cuda.synchronize()
    t_spin = time.perf_counter()
    L.check(L.get_lib().vlm_debug_occupy(1, 64, 0, 200000, L.stream_ptr()), "vlm_debug_occupy")
    t0 = time.perf_counter()
    plan.run()
    dt = time.perf_counter() - t0
    ev = torch.cuda.Event()
    ev.record()
    still_queued = not ev.query()
    torch.cuda.synchronize()
    spin = time.perf_counter() - t_spin
    print("ties enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "TiesPlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert all(torch.equal(res[k], first[k]) for k in exp)


def test_merge_ckpt_tool_as_a_child_process(merge, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {k: torch.from_numpy(v) for k, v in tiny_state("all_moe").items()}
    central = {k: torch.from_numpy(v) for k, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    words = ["with", "vlffn_start_layer_index=10"]

    def run_tool(method, *opts):
        out, rep = tmp_path / (method + ".ckpt"), tmp_path / (method + ".json")
        cmd = [sys.executable, TOOL, "--method", method, "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep)]
        r = subprocess.run(cmd + list(opts) + words, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got = ckpt.load_ckpt(str(out))
        assert set(torch.load(str(out), map_location="cpu", weights_only=True).keys()) == {"state_dict"}
        return got, json.load(open(rep))

    def same(got, want):
        assert list(got.keys()) == list(want.keys())
        for k in want:
            assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k

    cfg = merge_cfg(sum_lambda=0.75, merge_ratio=0.3)
    got, rep = run_tool("ties", "--central", str(tmp_path / "ufo.ckpt"), "--density", "0.2", "--lambda", "0.75")
    same(got, merge.ties_merge(to_dev(sd), cfg, central_weight=to_dev(central), density=0.2))
    assert len(rep["tensors"]) == 12 * 13 and all(len(t["kept"]) == len(t["threshold"]) for t in rep["tensors"])
    got, rep = run_tool("taskvec", "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.75")
    same(got, merge.sum_task_vectors(to_dev(sd), cfg, central_weight=to_dev(central)))
    assert len(rep["tensors"]) == 12 * 13
    got, rep = run_tool("interp", "--ratio", "0.3")
    same(got, merge.merge_weights(to_dev(sd), cfg))
    assert len(rep["tensors"]) == 12 * 13 and sorted(t["dst"] for t in rep["tensors"]) == sorted(k for k in got if is_block(k))


def test_model_method_is_the_same_merge(merge, pkg):
    """ViLTransformerSS.ties_merge forwards to merge.ties_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    want = merge.ties_merge(sd, Stub.hparams.config, central_weight=central, density=0.2)
    Stub.hparams.config["central_weight"] = None
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.ties_merge(Stub(), sd, density=0.2)
    torch.cuda.synchronize()
    assert all(got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes() for k in want if is_block(k))
