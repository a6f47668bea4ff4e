"""DARE merge on the GPU (csrc/dare.hip through the C ABI) against the numpy restatement of the rule (dare_restatement.py): every
comparison is over ALL elements and bit for bit.  The reference has no DARE; only the single-source layers of the vqa case can be
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
from test_ties_gpu import CASES, is_block, planted, to_dev
from dare_restatement import LINEAR, TIES, dare, keep_below

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
SEED = 20231106
MODES = {"linear": LINEAR, "ties": TIES}


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def job(c, srcs, drop, lam=0.75, seed=SEED, stream=5, mode="linear", rescale=True):
    return dict(c=c, srcs=srcs, drop=drop, lam=lam, seed=seed, stream=stream, mode=mode, rescale=rescale)


def run_plan(merge, jobs):
    """jobs: list of job(...).  Returns (outputs, report rows, plan)."""
    plan = merge.DarePlan("cuda")
    outs = [plan.add([torch.from_numpy(s).cuda() for s in j["srcs"]], torch.from_numpy(j["c"]).cuda(), j["drop"], j["lam"], j["seed"],
                     j["stream"], j["mode"], rescale=j["rescale"], name=str(i)) for i, j in enumerate(jobs)]
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def restate(j):
    return dare(j["c"], j["srcs"], j["drop"], j["lam"], j["seed"], j["stream"], MODES[j["mode"]], j["rescale"])


def check_jobs(jobs, outs, rows):
    for i, j in enumerate(jobs):
        exp, info = restate(j)
        assert outs[i].cpu().numpy().tobytes() == exp.tobytes(), (i, j["c"].size, j["mode"], j["drop"])
        r = rows[i]
        assert r["dst"] == str(i) and r["n"] == j["c"].size and r["keep_below"] == info["keep_below"] == keep_below(j["drop"])
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), (i, j["mode"], j["drop"])


SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 1 << 20]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("mode", ["linear", "ties"])
@pytest.mark.parametrize("drop", [0.0, 0.5, 0.9])
def test_dare_ragged_sizes(n, S, mode, drop, merge):
    c, srcs = planted(n, S, seed=n + S)
    jobs = [job(c, srcs, drop, mode=mode)]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    if drop == 0.0:
        assert rows[0]["kept"] == [n] * S


def test_dare_a_dozen_jobs_in_one_plan(merge):
    """Mixed sizes, S = 1 .. 4, both modes, drop / lam / seed / stream / rescale different per job."""
    rng = np.random.default_rng(8)
    jobs = []
    sizes = [12289, 1, 4097, 3, 1 << 18, 5, 8191, 4096, 70000, 1023, 2, 8193, 4099]
    for i, n in enumerate(sizes):
        S = 1 + i % 4
        c, srcs = planted(n, max(S, 2), seed=300 + i)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(F) * F(0.3)).astype(F))
        jobs.append(job(c, srcs[:S], [0.9, 0.5, 0.0, 0.25, 0.99][i % 5], lam=[1, 0.75, 0.3][i % 3], seed=[SEED, 0, 2 ** 64 - 1, 2 ** 32 + 7][i % 4],
                        stream=[0, 5, 155, 2 ** 32 - 1][(i // 2) % 4], mode=["linear", "ties"][i % 2], rescale=i % 7 != 3))
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert sum(r["conflict"] for r in rows) > 0 and sum(r["empty"] for r in rows) > 0


def test_dare_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one-chunk jobs (lengths cycled through 5, 1, 4097, 3, 2, 4099; 1 .. 4 sources; both modes; drop, lambda,
    seed, stream and rescale cycled as above), every input a 16-byte aligned view into one device buffer: each of the 12
    workgroups per CU owns three chunks, every one of another job -- so a run leaves a job, flushes its counters and loads the
    next job's scalars at every step, which plans below the grid size (one chunk per workgroup) never do.  Outputs and every
    counter against the restatement."""
    jobs = [job(c, srcs, [0.9, 0.5, 0.0, 0.25, 0.99][i % 5], lam=[1, 0.75, 0.3][i % 3], seed=[SEED, 0, 2 ** 64 - 1, 2 ** 32 + 7][i % 4],
                stream=[0, 5, 155, 2 ** 32 - 1][(i // 2) % 4], mode=["linear", "ties"][i % 2], rescale=i % 7 != 3)
            for i, (c, srcs) in enumerate(tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted))]
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    plan = merge.DarePlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base = next(views)
        outs.append(plan.add([next(views) for _ in j["srcs"]], base, j["drop"], j["lam"], j["seed"], j["stream"], j["mode"],
                             rescale=j["rescale"], name=str(i)))
        assert plan.jobs[-1].base == base.data_ptr()  # the view itself, not a staged copy
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, outs, plan.report())


def test_dare_coordinates_not_position_decide_the_mask(merge):
    n = 12289
    c, srcs = planted(n, 2, seed=1)
    other = [job(*planted(m, 3, seed=m)[:2], 0.5, stream=9) for m in (4097, 70000)]
    a = job(c, srcs, 0.9, stream=5)
    outs1, rows1, _ = run_plan(merge, [a] + other)
    outs2, rows2, _ = run_plan(merge, other + [a])
    assert outs1[0].cpu().numpy().tobytes() == outs2[2].cpu().numpy().tobytes()
    assert rows1[0]["kept"] == rows2[2]["kept"]
    # another stream, another seed: another pattern (where an entry is kept, out != c for these inputs' non-zero task vectors)
    base = outs1[0].cpu().numpy()
    for change in (dict(stream=6), dict(seed=SEED + 1), dict(seed=SEED + 2 ** 32)):
        b = dict(a, **change)
        outs, rows, _ = run_plan(merge, [b])
        check_jobs([b], outs, rows)
        assert not np.array_equal((outs[0].cpu().numpy() != c), (base != c)), change


def test_dare_drop_zero_is_the_plain_sum(merge):
    for S in (1, 2, 3, 4):
        n = 8191
        rng = np.random.default_rng(S)
        c = rng.standard_normal(n).astype(F)
        srcs = [(c + rng.standard_normal(n).astype(F) * F(0.1)).astype(F) for _ in range(S)]
        j = job(c, srcs, 0.0, lam=0.75, mode="linear")
        outs, rows, _ = run_plan(merge, [j])
        d = np.zeros(n, F)
        for w in srcs:
            d = d + (w - c)
        assert outs[0].cpu().numpy().tobytes() == (c + F(0.75) * d).astype(F).tobytes()
        assert rows[0]["kept"] == [n] * S and rows[0]["empty"] == 0 and rows[0]["keep_below"] == 2 ** 32


@pytest.mark.parametrize("mode", ["linear", "ties"])
def test_dare_dst_may_be_base_or_a_source(mode, merge):
    for n in (12289, 3):
        c, srcs = planted(n, 3, seed=n)
        j = job(c, srcs, 0.5, mode=mode)
        (want,), rows, _ = run_plan(merge, [j])
        want = want.cpu().numpy().tobytes()
        for which in ("base", 1):
            dev = [torch.from_numpy(s).cuda() for s in srcs]
            b = torch.from_numpy(c).cuda()
            out = b if which == "base" else dev[which]
            plan = merge.DarePlan("cuda")
            got = plan.add(dev, b, 0.5, 0.75, SEED, 5, mode, out=out, name="0")
            assert got.data_ptr() == out.data_ptr()
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want, (n, which)
            assert plan.report() == rows
            for k, s in enumerate(dev):  # the other inputs are untouched
                if which != k:
                    assert s.cpu().numpy().tobytes() == srcs[k].tobytes()


def test_dare_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.DarePlan("cuda")
    a = torch.zeros(64, device="cuda")
    args = (0.5, 1.0, SEED, 5)
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, *args, "linear")
    with pytest.raises(L.VlmError):
        plan.add([a, torch.zeros(32, device="cuda")], a, *args, "linear")
    with pytest.raises(L.VlmError):
        plan.add([a.double()], a, *args, "linear")
    with pytest.raises(L.VlmError):
        plan.add([a], a, *args, "median")
    with pytest.raises(L.VlmError):
        plan.add([a], a, *args, 2)
    with pytest.raises(ValueError):
        plan.add([a], a, 1.0, 1.0, SEED, 5, "linear")
    assert plan.jobs == []
    out = plan.add([a + 1, a + 2], a, 0.0, 0.5, SEED, 5, "linear")
    arr = (L.DareJob * 1)(*plan.jobs)
    ws = torch.empty(lib.vlm_dare_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    assert lib.vlm_dare_plan_upload(arr, 1, L.ptr(ws), 512, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    # on real device pointers: a partial overlap of dst with an input, a bad mode, a bad keep_below
    buf = torch.zeros(256, device="cuda")
    for field, value in (("n_src", 2), ("dst", buf.data_ptr() + 16), ("mode", 2), ("keep_below", 0), ("keep_below", 2 ** 32 + 1)):
        bad = L.DareJob.from_buffer_copy(bytes(plan.jobs[0]))
        bad.base = buf.data_ptr()
        bad.dst = buf.data_ptr() + 4 * 64  # disjoint from base: fine
        setattr(bad, field, value)
        rc = lib.vlm_dare_plan_upload((L.DareJob * 1)(bad), 1, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert rc == (0 if field == "n_src" else -1), (field, value)  # n_src = 2 changes nothing: the control that passes
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [1.5] * 64  # 0 + 0.5 * (1 + 2)


def test_dare_run_three_times_same_bytes_same_counters(merge):
    jobs = [job(*planted(n, S, seed=n), 0.9, mode=mode) for n, S, mode in ((70001, 3, "ties"), (4097, 2, "linear"), (3, 2, "ties"))]
    plan = merge.DarePlan("cuda")
    outs = [plan.add([torch.from_numpy(s).cuda() for s in j["srcs"]], torch.from_numpy(j["c"]).cuda(), j["drop"], j["lam"], j["seed"],
                     j["stream"], j["mode"], rescale=j["rescale"], name=str(i)) for i, j in enumerate(jobs)]
    got, reports = [], []
    for _ in range(3):  # every run writes into outputs pre-filled with NaN
        for o in outs:
            o.fill_(float("nan"))
        plan.run()
        torch.cuda.synchronize()
        got.append([o.cpu().numpy().tobytes() for o in outs])
        reports.append(plan.report())
    assert got[0] == got[1] == got[2]
    assert reports[0] == reports[1] == reports[2]
    check_jobs(jobs, outs, reports[0])


def restate_state(sd, central, cfg, drop, lam, seed, mode, rescale=True, layers=range(12)):
    """dst -> (expected tensor, info | None) for the block tensors of `layers`; single-source layers: the oracle's task-vector job.
    The stream is restated here: 13 * layer + the position of the name in the layer."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for slot, (src, dst) in enumerate(mo._names(i)):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None)
            else:
                out, info = dare(central[dst], srcs, drop, lam, seed, 13 * i + slot, MODES[mode], rescale)
                exp[dst] = (out.reshape(central[dst].shape), info)
    return exp


def check_report(rows, exp):
    by_dst = {r["dst"]: r for r in rows}
    assert sorted(by_dst) == sorted(k for k, (_, info) in exp.items() if info is not None)
    for dst, r in by_dst.items():
        info = exp[dst][1]
        assert (r["n"], r["keep_below"]) == (exp[dst][0].size, info["keep_below"]), dst
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), dst


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("mode,drop,rescale", [("linear", 0.9, True), ("ties", 0.5, True), ("ties", 0.9, False)])
def test_dare_merge_tiny_matches_restatement(case, mode, drop, rescale, merge):
    lam = 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {k: v.clone() for k, v in central.items()}
    rows, plans = [], []
    res = merge.dare_merge(sd, cfg, central_weight={"state_dict": central}, drop=drop, seed=SEED, mode=mode, rescale=rescale,
                           report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, drop, lam, SEED, mode, rescale)
    n_block = 0
    for k, v in res.items():
        if is_block(k):
            assert v.cpu().numpy().tobytes() == exp[k][0].tobytes(), k
            assert v.shape == central[k].shape and v.data_ptr() != central[k].data_ptr()
            if exp[k][1] is None:  # one source: the task-vector job with ratio 1, undropped, as sum_task_vectors issues it
                assert v.cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes(), k
            n_block += 1
        else:
            assert v is sd[k]
    assert n_block == 12 * 13
    assert all(torch.equal(central[k], central_before[k]) for k in central)  # the central tensors are inputs only
    check_report(rows, exp)
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.DarePlan)
    # a tensor's mask does not depend on which other keys are present: without layer 0's experts (its merged keys pass through)
    # every other output is the same
    if case == "all":
        fewer = {k: v for k, v in sd.items() if "transformer.blocks.0." not in k}
        fewer.update({k: res[k] for k in res if "transformer.blocks.0." in k and is_block(k)})
        res2 = merge.dare_merge(fewer, cfg, central_weight=central, drop=drop, seed=SEED, mode=mode, rescale=rescale, lam=lam)
        torch.cuda.synchronize()
        for k in res:
            if is_block(k):
                assert res2[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
                assert (res2[k] is fewer.get(k)) == ("transformer.blocks.0." in k)


def test_dare_base_size(merge):
    """Base size (the inputs of test_ties_base_size), drop 0.9: layers 0 (two sources) and 11 (three) against the restatement bit
    for bit, every other output finite; the plan's byte counts; and run() returns while its launches are still queued."""
    L = importlib.import_module("vl_merging_amd._lib")
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    plans, rows = [], []
    res = merge.dare_merge(sd, cfg, central_weight=central, drop=0.9, seed=SEED, plan_out=plans, report_out=rows)
    torch.cuda.synchronize()
    plan = plans[0]
    n_out = sum(v.numel() for k, v in res.items() if is_block(k))
    assert plan.bytes_written == 4 * n_out == 340180992
    assert plan.bytes_read == 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs) == 737058816 + 340180992
    exp = restate_state(sd_np, central_np, cfg, 0.9, 0.75, SEED, "linear", layers=(0, 11))
    by_dst = {r["dst"]: r for r in rows}
    for k, (want, info) in exp.items():
        assert res[k].cpu().numpy().tobytes() == want.tobytes(), k
        r = by_dst[k]
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), k
    assert len(rows) == 12 * 13
    for k, v in res.items():
        if is_block(k):
            assert bool(torch.isfinite(v).all()), k
    # no host synchronisation between upload and the end of run(): the ENQUEUE is timed behind a 0.2 s spin kernel on the same
    # stream, as test_ties_base_size does.  The spin's own length is checked, so the bound cannot pass vacuously.
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
    print("dare enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "DarePlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert all(torch.equal(res[k], first[k]) for k in exp)
    assert plan.report() == rows


def test_merge_ckpt_dare_as_a_child_process(merge, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {k: torch.from_numpy(v) for k, v in tiny_state("all_moe").items()}
    central = {k: torch.from_numpy(v) for k, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "dare.ckpt", tmp_path / "dare.json"
    cmd = [sys.executable, TOOL, "--method", "dare", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--drop", "0.7", "--seed", str(SEED), "--dare-mode", "ties", "--no-rescale",
           "--lambda", "0.75", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = merge.dare_merge(to_dev(sd), merge_cfg(sum_lambda=0.75), central_weight=to_dev(central), drop=0.7, seed=SEED, mode="ties",
                            rescale=False, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert (rep["method"], rep["drop"], rep["seed"], rep["dare_mode"]) == ("dare", 0.7, SEED, "ties")
    assert rep["sum_lambda"] == 0.75 and "merge_ratio" in rep and rep["density"] is None  # the existing keys stay
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows


def test_model_method_is_the_same_merge(merge, pkg):
    """ViLTransformerSS.dare_merge forwards to merge.dare_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    want = merge.dare_merge(sd, Stub.hparams.config, central_weight=central, drop=0.8, seed=SEED, mode="ties", rescale=False)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.dare_merge(Stub(), sd, drop=0.8, seed=SEED, mode="ties", rescale=False)
    torch.cuda.synchronize()
    assert all(got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes() for k in want if is_block(k))
    default = vm.ViLTransformerSS.dare_merge.__defaults__
    assert default == (0.9, None, 0, "linear", True)  # merge.dare_merge's defaults
