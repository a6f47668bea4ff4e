"""SCE on the GPU (csrc/sce.hip through the C ABI) against the restatement of the rule (sce_restatement.py): the output tensor, the
threshold key, the counters, every double of the report and the weights' bits are compared bit for bit.  The reference has no
SCE."""
import hashlib
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
from test_stock_cpu import aligned
from pairstats_restatement import bits
from ties_restatement import keep_count
import sce_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
# workgroups per CU of the three chunk grids: SCE_HIST_BLOCKS_PER_CU, SCE_REDUCE_BLOCKS_PER_CU, SCE_APPLY_BLOCKS_PER_CU (csrc/sce.hip)
GRIDS_PER_CU = (4, 12, 12)


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def job(c, srcs, density=0.1, lam=0.75, keep=None):
    return dict(c=c, srcs=srcs, density=density, lam=lam, keep=keep)


def planted_job(n, S, seed, **kw):
    """planted (test_ties_gpu.py) data for S = 1 .. 4 sources: half the elements on a dyadic grid (many equal variances: ties
    wherever the K-th place falls), -0.0 task-vector entries, exact cancellations t_1 = -t_0 in a sixth of the elements (s = 0)."""
    c, srcs = planted(n, max(S, 2), seed=seed)
    return job(c, srcs[:S], **kw)


def aligned_job(n, S, seed, **kw):
    """aligned (test_stock_cpu.py) data: experts that share a component plus noise of their own: ordinary floats, few ties."""
    return job(*aligned(n, S, seed), **kw)


def run_plan(merge, jobs, tensors=None):
    """jobs: list of job(...); `tensors`: per job (base, [sources]) already on the device.  Returns (outputs, report rows, plan)."""
    plan = merge.ScePlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base, srcs = tensors[i] if tensors else (torch.from_numpy(j["c"]).cuda(), [torch.from_numpy(s).cuda() for s in j["srcs"]])
        outs.append(plan.add(srcs, base, density=j["density"], lam=j["lam"], keep=j["keep"], name=str(i)))
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))


def check_jobs(jobs, outs, rows):
    """Every output and every report row against the restatement; returns the restatement's rows."""
    assert len(rows) == len(jobs)
    want = []
    for i, j in enumerate(jobs):
        exp, row = R.sce(j["c"], j["srcs"], j["density"], j["lam"], keep=j["keep"], name=str(i))
        assert bits(rows[i]) == bits(row), (i, j["c"].size, len(j["srcs"]), rows[i], row)
        assert same_bits(outs[i], exp), (i, j["c"].size, len(j["srcs"]))
        want.append(row)
    return want


def raw_bytes(plan):
    """The raw results and counters of all jobs as the device left them."""
    L = importlib.import_module("vl_merging_amd._lib")
    hdr = L.SceHeader.from_buffer_copy(plan.ws[:96].cpu().numpy().tobytes())
    n = len(plan.jobs)
    return (plan.ws[hdr.state_off: hdr.state_off + 72 * n].cpu().numpy().tobytes(),
            plan.ws[hdr.counters_off: hdr.counters_off + 24 * n].cpu().numpy().tobytes())


SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 12289, 3 * 4096 + 2]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("density", [0.1, 1.0])
def test_sce_ragged_sizes(n, S, density, merge):
    """The tail alone, a partial wave, one float4, a float4 plus tail, one full chunk, a chunk plus tail, three chunks plus a tail
    of one and of two; K = 1 (density 0.1 of up to 5 elements) and K = n: aligned and planted inputs as two jobs of one plan."""
    jobs = [aligned_job(n, S, seed=n + S, density=density), planted_job(n, S, seed=n + S, density=density)]
    outs, rows, _ = run_plan(merge, jobs)
    want = check_jobs(jobs, outs, rows)
    assert rows[0]["K"] == keep_count(density, n) and all(r["kept"] >= r["K"] for r in rows)
    if density == 1.0:
        assert all(r["kept"] == n for r in rows)
    if S == 1:  # the task-vector job: var = +0.0 everywhere, everything selected, the weight is 1 unless the task vector is zero
        assert all((r["threshold_bits"], r["kept"]) == (0, n) for r in rows)
        assert want[0]["weight"] == [1.0]
        x = jobs[0]["srcs"][0] - jobs[0]["c"]
        assert same_bits(outs[0], jobs[0]["c"] + F(0.75) * x)


def test_sce_ties_at_the_threshold(merge):
    """x_1 = -x_0 = -a with a on a grid of eight magnitudes: var = a^2 takes eight values, each some 600 times, so the K-th place
    falls inside a block of equal keys and all of it is selected: kept > K.  Every selected element cancels (s = 0): all are
    empty and conflicts.  A second job adds a third source, so the selected elements elect a sign; a third is pure grid data with
    four sources."""
    n = 5003
    rng = np.random.default_rng(3)
    a = (rng.integers(1, 9, n) / 8).astype(F)
    c = (rng.integers(-16, 17, n) / 8).astype(F)
    third = (c + (rng.integers(-16, 17, n) / 8).astype(F)).astype(F)
    grid = [(c + (rng.integers(-16, 17, n) / 8).astype(F)).astype(F) for _ in range(4)]
    jobs = [job(c, [c + a, c - a], density=0.3), job(c, [c + a, c - a, third], density=0.3), job(c, grid, keep=1234),
            job(c, [c + a, c - a], keep=1), job(c, [c + a, c - a], keep=n)]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert all(r["kept"] > r["K"] for r in rows[:4]) and rows[4]["kept"] == n
    assert rows[0]["empty"] == n and rows[0]["conflict"] == rows[0]["kept"] and same_bits(outs[0], c)
    assert 0 < rows[1]["empty"] < n and rows[2]["conflict"] > 0 and rows[3]["threshold"] == 1.0  # the largest a is 8 / 8


def dozen_jobs():
    sizes = [12289, 1, 4097, 3, 1 << 16, 5, 8191, 4096, 70000, 1023, 2, 8193, 4099]
    dens = [0.1, 1.0, 0.3, 0.05]
    return [(aligned_job if i % 3 else planted_job)(n, 1 + i % 4, seed=300 + i, density=dens[i % 4], lam=[0.75, 1.0][i % 2])
            for i, n in enumerate(sizes)]


def test_sce_a_dozen_jobs_in_one_plan_and_position_does_not_show(merge):
    """Mixed sizes, S = 1 .. 4, densities and scales in one plan; what a job does not have is zero in its raw result; and the same
    jobs in another order leave the same bytes per job: results, counters and outputs."""
    jobs = dozen_jobs()
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert sorted({len(r["sq"]) for r in rows}) == [1, 2, 3, 4]
    for j, (res, _) in zip(jobs, plan.results()):
        S = len(j["srcs"])
        assert all((res.sq[m], res.w[m]) == (0, 0) for m in range(S, 4)) and res.reserved == 0 and res.rank >= 1
    order = list(range(len(jobs)))[::-1]
    order = order[3:] + order[:3]
    outs2, rows2, plan2 = run_plan(merge, [jobs[i] for i in order])
    (res1, cnt1), (res2, cnt2) = raw_bytes(plan), raw_bytes(plan2)
    for at, i in enumerate(order):
        assert res2[72 * at: 72 * (at + 1)] == res1[72 * i: 72 * (i + 1)], i
        assert cnt2[24 * at: 24 * (at + 1)] == cnt1[24 * i: 24 * (i + 1)], i
        assert same_bits(outs2[at], outs[i].cpu().numpy()), i
        assert bits({**rows2[at], "dst": None}) == bits({**rows[i], "dst": None})


def test_sce_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one- and two-chunk jobs (helpers/merge_inputs.tiny_jobs), every input a 16-byte aligned view into one
    device buffer, used unstaged: the plan has more chunks than twice the widest of the three grids (histogram passes 4 per CU,
    reducer and apply pass 12 per CU), so on each of them every workgroup's run of chunks holds several jobs: a histogram pass
    flushes and loads the next job's prefix, the reducer loads a new threshold and first-record index, the apply pass a new
    threshold and weights and flushes its counters at nearly every step."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    data = tiny_jobs(n_cus, planted)
    dens = [0.2, 0.05, 1.0]
    jobs = [job(c, srcs, density=dens[i % 3], lam=[1.0, 0.75][i % 2]) for i, (c, srcs) in enumerate(data)]
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    tensors = []
    for j in jobs:
        base = next(views)
        tensors.append((base, [next(views) for _ in j["srcs"]]))
    outs, rows, plan = run_plan(merge, jobs, tensors)
    for pj, (base, srcs) in zip(plan.jobs, tensors):  # the views themselves, not staged copies
        assert pj.base == base.data_ptr() and [pj.src[m] for m in range(len(srcs))] == [s.data_ptr() for s in srcs]
    L = importlib.import_module("vl_merging_amd._lib")
    hdr = L.SceHeader.from_buffer_copy(plan.ws[:96].cpu().numpy().tobytes())
    assert hdr.n_chunks > 2 * max(GRIDS_PER_CU) * n_cus and hdr.n_units == hdr.n_jobs == len(jobs)
    check_jobs(jobs, outs, rows)
    assert len({tuple(r["weight_bits"]) for r in rows}) > 10 and len({r["threshold_bits"] for r in rows}) > 10  # a stale one would show


def test_sce_a_job_that_fills_several_workgroups_whole_runs(merge):
    """One job of 12 x CUs + 37 chunks and a tail between small jobs of other thresholds and weights: on the 12-per-CU grids the
    runs are two chunks long, on the histogram grid six, so most workgroups' whole runs lie inside the one job -- many workgroups
    add to one histogram, many records fold into one sum -- and the runs at its ends cross into the neighbours."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (12 * n_cus + 37) * 4096 + 5
    jobs = [planted_job(4097, 2, seed=1), aligned_job(5000, 3, seed=2, density=0.3), aligned_job(big, 2, seed=3), planted_job(3, 2, seed=4),
            aligned_job(8191, 4, seed=5, density=1.0)]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert rows[2]["K"] == keep_count(0.1, big) and len({r["threshold_bits"] for r in rows}) >= 4


def test_sce_run_three_times_same_bytes_inputs_untouched(merge):
    jobs = [aligned_job(70001, 3, seed=1), planted_job(4097, 2, seed=2, density=0.3), aligned_job(3, 2, seed=3), aligned_job(5000, 4, seed=4)]
    plan = merge.ScePlan("cuda")
    outs = [plan.add([torch.from_numpy(s).cuda() for s in j["srcs"]], torch.from_numpy(j["c"]).cuda(), density=j["density"], lam=j["lam"],
                     name=str(i)) for i, j in enumerate(jobs)]
    inputs = [t for t in plan.keep if all(t is not o for o in outs)]
    assert len(inputs) == sum(len(j["srcs"]) + 1 for j in jobs)
    before = [t.cpu().numpy().tobytes() for t in inputs]
    got, raw, reports = [], [], []
    for _ in range(3):  # every run writes into outputs pre-filled with NaN
        for o in outs:
            o.fill_(float("nan"))
        plan.run()
        torch.cuda.synchronize()
        got.append([o.cpu().numpy().tobytes() for o in outs])
        raw.append(raw_bytes(plan))
        reports.append(plan.report())
    assert got[0] == got[1] == got[2] and raw[0] == raw[1] == raw[2]
    assert bits(reports[0]) == bits(reports[1]) == bits(reports[2])
    check_jobs(jobs, outs, reports[0])
    assert [t.cpu().numpy().tobytes() for t in inputs] == before  # every source and every base: read only
    n_in = sum(j["c"].size * (len(j["srcs"]) + 1) for j in jobs)
    assert plan.bytes_read == 5 * 4 * n_in and plan.bytes_written == 4 * sum(j["c"].size for j in jobs)  # five passes read


def test_sce_hand_cases_on_the_device(merge):
    """The cases of test_sce_cpu.py that are written from constants, as jobs of one plan."""
    f32 = lambda *v: np.array(v, dtype=F)  # noqa: E731
    c5, x5 = f32(0.5, -1.25, 3.0, 0.0, 7.0), f32(1.0, 1.0, -1.0, 0.125, 0.0)
    c3, c4, c6 = f32(1, 1, 1), f32(0.5, 0.5, 0.5, 0.5), f32(0.5, -1.25, 3.0, 0.0, 7.0, 1e-3)
    a, z = f32(5, 4, 3, 3, 3, 2, 1, 0), np.zeros(8, F)
    jobs = [job(c5, [c5 + x5, c5 + x5], density=0.2, lam=0.5), job(f32(1, 2, 3), [f32(1.5, -4, 3)], density=0.5, lam=1.0),
            job(c3, [c3 + f32(2, 1, 4), c3 + f32(-2, 3, 4)], density=0.5, lam=1.0),
            job(c4, [c4 + f32(0, 0, 1, 1), c4 + f32(4, -2, 1, 1)], density=0.5, lam=1.0),
            job(c6, [c6.copy(), c6.copy(), c6.copy()], density=0.3), job(z, [a, -a], density=0.3, lam=1.0)]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    same, one, opposite, zero, central, dup = rows
    assert (same["threshold_bits"], same["kept"], same["weight"], same["empty"]) == (0, 5, [0.5, 0.5], 1)
    assert outs[0].cpu().numpy().tolist() == (c5 + F(0.5) * x5).tolist()
    assert (one["weight"], one["sq"], one["kept"]) == ([1.0], [36.25], 3) and outs[1].cpu().numpy().tolist() == [1.5, -4.0, 3.0]
    assert (opposite["sq"], opposite["tot"], opposite["kept"], opposite["conflict"], opposite["empty"]) == ([5.0, 13.0], 18.0, 2, 1, 2)
    assert (zero["weight_bits"], zero["sq"]) == ([0, 0x3F800000], [0.0, 20.0]) and outs[3].cpu().numpy().tolist() == [4.5, -1.5, 0.5, 0.5]
    assert (central["tot"], central["empty"], central["weight_bits"]) == (0.0, 6, [int(F(1 / 3).view(np.uint32))] * 3) and same_bits(outs[4], c6)
    assert (dup["K"], dup["kept"], dup["threshold"]) == (3, 5, 9.0)


def test_sce_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.ScePlan("cuda")
    a = torch.arange(64, device="cuda", dtype=torch.float32)
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, density=0.5)
    with pytest.raises(L.VlmError):
        plan.add([a, torch.zeros(32, device="cuda")], a, density=0.5)
    with pytest.raises(L.VlmError):
        plan.add([a, a], torch.zeros(32, device="cuda"), density=0.5)
    with pytest.raises(L.VlmError):
        plan.add([a.double()], a, density=0.5)
    with pytest.raises(ValueError):
        plan.add([a, a], a, density=0.0)
    with pytest.raises(L.VlmError):
        plan.report()  # nothing has run
    assert plan.jobs == []
    out = plan.add([a + 1, 2 * a + 1], a, density=0.25, lam=0.5)
    ws = torch.empty(lib.vlm_sce_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    assert lib.vlm_sce_plan_upload((L.SceJob * 1)(*plan.jobs), 1, L.ptr(ws), 512, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    assert lib.vlm_sce_plan_upload((L.SceJob * 1)(*plan.jobs), 1, L.ptr(ws), ws.numel() - 256, L.stream_ptr()) == -3
    buf = torch.zeros(256, device="cuda")
    src0 = plan.jobs[0].src[0]
    for field, value, rc in (("n_src", 0, -1), ("n_src", 5, -1), ("n_elem", 0, -1), ("base", 0, -1), ("dst", 0, -1),
                             ("k", 0, -1), ("k", 65, -1),
                             ("base", buf.data_ptr() + 4, -1), ("src0", buf.data_ptr() + 8, -1), ("src0", 0, -1),
                             ("dst", a.data_ptr(), -1), ("dst", src0, -1), ("dst", src0 + 16, -1), ("dst", buf.data_ptr() + 4, -1),
                             ("dst", buf.data_ptr(), 0), ("n_src", 1, 0), ("k", 1, 0), ("k", 64, 0)):
        bad = L.SceJob.from_buffer_copy(bytes(plan.jobs[0]))
        if field == "src0":
            bad.src[0] = value
        else:
            setattr(bad, field, value)
        got = lib.vlm_sce_plan_upload((L.SceJob * 1)(bad), 1, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert got == rc, (field, value)  # another dst, n_src = 1, k = 1 and k = n are fine: the controls that pass
    plan.run()
    torch.cuda.synchronize()
    exp, row = R.sce(a.cpu().numpy(), [(a + 1).cpu().numpy(), (2 * a + 1).cpu().numpy()], 0.25, 0.5)
    assert same_bits(out, exp) and bits(plan.report()[0]) == bits(row) and row["kept"] == 16


def restate_state(sd, central, cfg, density, lam, layers=range(12)):
    """dst -> (expected tensor, report row | None) for the block tensors of `layers`; single-source layers: the oracle's
    task-vector job."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None)
            else:
                out, row = R.sce(central[dst], srcs, density, lam, name=dst)
                exp[dst] = (out.reshape(central[dst].shape), row)
    return exp


@pytest.fixture(scope="module")
def tiny():
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    return sd_np, central_np, to_dev(sd_np), to_dev(central_np)


@pytest.mark.parametrize("case", sorted(CASES))
def test_sce_merge_tiny_matches_restatement(case, merge, tiny):
    sd_np, central_np, sd, central = tiny
    density, lam = 0.2, 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    central_before = {k: v.clone() for k, v in central.items()}
    rows, plans = [], []
    res = merge.sce_merge(sd, cfg, central_weight={"state_dict": central}, density=density, report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, density, lam)
    n_block = 0
    for k, v in res.items():
        if is_block(k):
            assert same_bits(v, exp[k][0]), k
            assert v.shape == central[k].shape and v.data_ptr() != central[k].data_ptr()
            if exp[k][1] is None:  # one source: the task-vector job with ratio 1, as sum_task_vectors issues it
                assert same_bits(v, ref[k].cpu().numpy()), k
            n_block += 1
        else:
            assert v is sd[k]  # pass-through by identity
    assert n_block == 12 * 13
    assert all(torch.equal(central[k], central_before[k]) for k in central)
    assert [r["dst"] for r in rows] == [k for k in res if is_block(k) and exp[k][1] is not None]  # the walk's order
    assert bits(rows) == bits([exp[r["dst"]][1] for r in rows])
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.ScePlan)
    if case == "used_vqa":
        assert isinstance(plans[1], merge.MergePlan)
    assert json.loads(json.dumps(rows)) == rows  # the CLI's report rows
    # lam=None takes config["sum_lambda"]; another lambda gives other bytes
    res2 = merge.sce_merge(sd, cfg, central_weight=central, density=density, lam=lam)
    other = merge.sce_merge(sd, dict(cfg, sum_lambda=0.5), central_weight=central, density=density)
    torch.cuda.synchronize()
    assert all(same_bits(res2[k], res[k].cpu().numpy()) for k in res if is_block(k))
    assert any(not same_bits(other[k], res[k].cpu().numpy()) for k in res if is_block(k) and exp[k][1] is not None)
    with pytest.raises(KeyError):
        merge.sce_merge(sd, cfg, central_weight={k: v for k, v in central.items() if "blocks.3.norm1.weight" not in k})
    with pytest.raises(ValueError):
        merge.sce_merge(sd, cfg, central_weight=central, density=1.5)


def test_sce_base_size(merge):
    """Base size (the inputs of test_merge_base_size_digests), density 0.1, once: the digests of the outputs of layers 0 (two
    sources) and 11 (three) against the restatement's, their report rows bit for bit; for all 156 tensors the weights against
    step 5 in python doubles applied to the reported sums; and run() returns while its nine launches are still queued."""
    L = importlib.import_module("vl_merging_amd._lib")
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    plans, rows = [], []
    res = merge.sce_merge(sd, cfg, central_weight=central, density=0.1, plan_out=plans, report_out=rows)
    torch.cuda.synchronize()
    plan = plans[0]
    n_out = sum(v.numel() for k, v in res.items() if is_block(k))
    assert plan.bytes_written == 4 * n_out == 340180992
    assert plan.bytes_read == 5 * 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs)  # five passes
    exp = restate_state(sd_np, central_np, cfg, 0.1, 0.75, layers=(0, 11))
    by_dst = {r["dst"]: r for r in rows}
    digest = lambda b: hashlib.sha256(b).hexdigest()  # noqa: E731
    for k, (want, row) in exp.items():
        assert digest(res[k].cpu().numpy().tobytes()) == digest(np.ascontiguousarray(want).tobytes()), k
        assert bits(by_dst[k]) == bits(row), k
    assert len(rows) == 12 * 13
    for r in rows:
        tot, w = R.weights(r["sq"])
        assert bits((r["tot"], r["weight"])) == bits((tot, w)) and r["weight_bits"] == [R.f32_bits(v) for v in w], r["dst"]
        assert r["K"] == keep_count(0.1, r["n"]) <= r["kept"] <= r["n"] and r["tot"] > 0
    for k, v in res.items():
        if is_block(k):
            assert bool(torch.isfinite(v).all()), k
    # no host synchronisation between upload and the end of run(), although the reducer waits for the select's threshold and the
    # apply pass for the fold's weights: the ENQUEUE is timed behind a 0.2 s spin kernel on the same stream, as test_ties_base_size
    # does.  The spin's own length is checked, so the bound cannot pass vacuously.
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
    print("sce enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "ScePlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert bits(plan.report()) == bits(rows) and all(torch.equal(res[k].view(torch.int32), first[k].view(torch.int32)) for k in exp)


def test_merge_ckpt_sce_as_a_child_process(merge, tmp_path, tiny):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    _, _, sd, central = tiny
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in central.items()}}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "sce.ckpt", tmp_path / "sce.json"
    cmd = [sys.executable, TOOL, "--method", "sce", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.3", "--density", "0.4", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = merge.sce_merge(sd, merge_cfg(sum_lambda=0.3), central_weight=central, density=0.4, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert (rep["method"], rep["density"], rep["sum_lambda"]) == ("sce", 0.4, 0.3) and (rep["drop"], rep["seed"], rep["epsilon"]) == (None,) * 3
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows  # json round-trips a double exactly


def test_model_method_is_the_same_merge(merge, pkg, tiny):
    """ViLTransformerSS.sce_merge forwards to merge.sce_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    _, _, sd, central = tiny
    want = merge.sce_merge(sd, Stub.hparams.config, central_weight=central, density=0.3, lam=0.5)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.sce_merge(Stub(), sd, density=0.3, lam=0.5)
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(same_bits(got[k], want[k].cpu().numpy()) for k in want if is_block(k))


def test_the_generalised_select_still_serves_ties_and_band(merge):
    """ties_select.h now also holds the element-keyed form; its per-source instantiations, on a tiny plan each, against their own
    restatements: thresholds, counters and outputs (the existing suites do this at length; this one sits next to the change)."""
    import test_band_gpu as tb
    import test_ties_gpu as tt
    jobs = [(*planted(n, S, seed=n + S), d, 0.75) for n, S, d in ((4097, 2, 0.2), (12289, 3, 0.05), (5, 2, 1.0), (3 * 4096 + 2, 2, 0.3))]
    outs, rows, _ = tt.run_plan(merge, jobs)
    tt.check_jobs(jobs, outs, rows)
    bjobs = [tb.job(*planted(4097, 2, seed=9), dg=(0.9, 0.05)), tb.job(*planted(12289, 3, seed=10), dg=(0.5, 0.3), mode="ties"),
             tb.job(*planted(5, 2, seed=11), dg=(1.0, 0.0)), tb.job(*planted(3 * 4096 + 2, 2, seed=12), dg=(0.05, 0.3), mode="ties")]
    outs, rows, _ = tb.run_plan(merge, bjobs)
    tb.check_jobs(bjobs, outs, rows)
