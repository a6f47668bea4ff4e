"""Model Stock on the GPU (csrc/stock.hip through the C ABI) against the restatement of the rule (stock_restatement.py): the output
tensor and every double of the report are compared by their bytes -- among them cos_p, cos, t and scale, which the device makes
in f64 and python restates with its own doubles.  The reference has no Model Stock."""
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
import stock_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def job(c, srcs):
    return dict(c=c, srcs=srcs)


def planted_job(n, S, seed):
    """planted (test_ties_gpu.py) data for S = 1 .. 4 sources: -0.0 task-vector entries, exact cancellations t_1 = -t_0 in a sixth of
    the elements (the cosine falls to or below zero: the clamp), many equal magnitudes."""
    c, srcs = planted(n, max(S, 2), seed=seed)
    return job(c, srcs[:S])


def aligned_job(n, S, seed):
    return dict(job(*aligned(n, S, seed)), aligned=True)


def run_plan(merge, jobs, tensors=None):
    """jobs: list of job(...); `tensors`: per job (base, [sources]) already on the device.  Returns (outputs, report rows, plan)."""
    plan = merge.StockPlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base, srcs = tensors[i] if tensors else (torch.from_numpy(j["c"]).cuda(), [torch.from_numpy(s).cuda() for s in j["srcs"]])
        outs.append(plan.add(srcs, base, name=str(i)))
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))


def check_jobs(jobs, outs, rows):
    """Every output and every report row against the restatement; returns the restatement's rows.  An `aligned` job of 1023
    elements or more and several sources has its cosine well inside (0, 1): it does not test the clamp."""
    assert len(rows) == len(jobs)
    want = []
    for i, j in enumerate(jobs):
        exp, row = R.stock(j["c"], j["srcs"], name=str(i))
        if j.get("aligned") and j["c"].size >= 1023 and len(j["srcs"]) >= 2:
            assert 0.05 < row["cos"] < 0.95, (i, row["cos"])
        assert bits(rows[i]) == bits(row), (i, j["c"].size, len(j["srcs"]), rows[i], row)
        assert same_bits(outs[i], exp), (i, j["c"].size, len(j["srcs"]))
        want.append(row)
    return want


def result_bytes(plan):
    """The raw results of all jobs as the device left them."""
    L = importlib.import_module("vl_merging_amd._lib")
    hdr = L.StockHeader.from_buffer_copy(plan.ws[:56].cpu().numpy().tobytes())
    return plan.ws[hdr.results_off: hdr.results_off + 152 * len(plan.jobs)].cpu().numpy().tobytes()


SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 70001, 1 << 20]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_stock_ragged_sizes(n, S, merge):
    """The tail alone, a partial wave, one full chunk, a chunk plus tail, 18 chunks (one more than a fold batch) plus tail, 256
    records to fold: aligned and planted inputs as two jobs of one plan.  The aligned job's ratio lies strictly inside (0, 1) (one
    source has no cosine: t = 1), the planted job's cosine is at or below zero for two sources: the clamp."""
    jobs = [aligned_job(n, S, seed=n + S), planted_job(n, S, seed=n + S)]
    outs, rows, _ = run_plan(merge, jobs)
    want = check_jobs(jobs, outs, rows)
    if n >= 1023 and S >= 2:
        assert 0.05 < want[0]["cos"] < 0.95 and 0.0 < rows[0]["t"] < 1.0
    if S == 1:
        assert (rows[0]["cos"], rows[0]["t"], rows[0]["scale"]) == (0.0, 1.0, 1.0)


def test_stock_same_sums_as_pair_statistics(merge):
    """For the same device tensors, sq and dot are the bytes PairStatsPlan reports with a base."""
    specs = [(70001, 4, aligned_job), (12289, 3, planted_job), (4097, 2, aligned_job), (5, 2, planted_job), (1 << 18, 3, aligned_job)]
    jobs = [mk(n, S, seed=40 + i) for i, (n, S, mk) in enumerate(specs)]
    tensors = [(torch.from_numpy(j["c"]).cuda(), [torch.from_numpy(s).cuda() for s in j["srcs"]]) for j in jobs]
    outs, rows, _ = run_plan(merge, jobs, tensors)
    ps = merge.PairStatsPlan("cuda")
    for base, srcs in tensors:
        ps.add(srcs, base)
    ps.run()
    torch.cuda.synchronize()
    for mine, theirs in zip(rows, ps.report()):
        assert bits(mine["sq"]) == bits(theirs["sq"])
        assert [(p["a"], p["b"]) for p in mine["pairs"]] == [(p["a"], p["b"]) for p in theirs["pairs"]]
        assert bits([p["dot"] for p in mine["pairs"]]) == bits([p["dot"] for p in theirs["pairs"]])
    check_jobs(jobs, outs, rows)


def dozen_jobs():
    sizes = [12289, 1, 4097, 3, 1 << 18, 5, 8191, 4096, 70000, 1023, 2, 8193, 4099]
    return [(aligned_job if i % 3 else planted_job)(n, 1 + i % 4, seed=300 + i) for i, n in enumerate(sizes)]


def test_stock_a_dozen_jobs_in_one_plan(merge):
    """Mixed sizes and S = 1 .. 4: all six pair slots for S = 4, none for S = 1; what a job does not have is zero in the raw result."""
    jobs = dozen_jobs()
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    assert sorted({len(r["pairs"]) for r in rows}) == [0, 1, 3, 6]
    assert any(0 < r["t"] < 1 for r in rows) and any(r["t"] == 0 for r in rows) and any(r["t"] == 1 for r in rows)
    L = importlib.import_module("vl_merging_amd._lib")
    for j, res in zip(jobs, plan.results()):
        S = len(j["srcs"])
        assert all(res.sq[m] == 0 for m in range(S, 4)) and res.reserved == 0
        assert all((res.dot[k], res.cos_pair[k]) == (0, 0) for k in range(S * (S - 1) // 2, 6))
    assert len(result_bytes(plan)) == len(jobs) * 152 and isinstance(plan.results()[0], L.StockResult)


def test_stock_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one- and two-chunk jobs (helpers/merge_inputs.tiny_jobs), every input a 16-byte aligned view into one
    device buffer, used unstaged: every workgroup's run of chunks holds several jobs, so the reducer loads a new first-record index
    and the apply pass a new `scale` at nearly every step."""
    data = tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted)
    jobs = [job(c, srcs) for c, srcs in data]
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    tensors = []
    for j in jobs:
        base = next(views)
        tensors.append((base, [next(views) for _ in j["srcs"]]))
    outs, rows, plan = run_plan(merge, jobs, tensors)
    for pj, (base, srcs) in zip(plan.jobs, tensors):  # the views themselves, not staged copies
        assert pj.base == base.data_ptr() and [pj.src[m] for m in range(len(srcs))] == [s.data_ptr() for s in srcs]
    check_jobs(jobs, outs, rows)
    assert len({r["scale_bits"] for r in rows}) > 10  # neighbours differ in scale: a stale one would show


def test_stock_a_job_that_fills_several_workgroups_whole_runs(merge):
    """One job of 12 x CUs + 37 chunks and a tail between small jobs of other scales: the reducer's grid is 12 workgroups per CU, so
    its runs are two chunks long, most workgroups' whole runs lie inside the one job and the runs at its ends cross into the
    neighbours (the apply pass's runs, 96 per CU, are one chunk here; the next test is about them)."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (12 * n_cus + 37) * 4096 + 5
    jobs = [planted_job(4097, 2, seed=1), aligned_job(5000, 3, seed=2), aligned_job(big, 2, seed=3), planted_job(3, 2, seed=4),
            aligned_job(8191, 4, seed=5)]
    outs, rows, _ = run_plan(merge, jobs)
    want = check_jobs(jobs, outs, rows)
    assert 0.05 < want[2]["cos"] < 0.95 and len({r["scale_bits"] for r in rows}) >= 4


def test_stock_apply_runs_cross_job_boundaries_on_its_own_grid(merge):
    """The apply pass runs 96 workgroups per CU, so in the plans above each of its workgroups owns one chunk.  Here a plan has more
    than 2 x 96 x CUs chunks in jobs of one to four chunks (two sources, every tensor a 16-byte aligned view into one buffer per role):
    every workgroup's run is three chunks long and crosses a job boundary or two, loading a new `scale` each time.  The restatement
    of 190 M elements would take minutes on the host, so the yardstick is made in two halves: every job's ratio is step 3 in python
    doubles applied to the job's own reported sums (which the other tests hold to the restatement, with runs that cross jobs),
    and the output is step 4 with those scales in torch's elementwise fp32 operations on the device, one rounding each, no FMA."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    lengths = [3 * 4096, 2 * 4096 + 3, 4096 - 4, 3 * 4096 + 5, 4097, 2 * 4096]  # 3, 2, 1, 4, 1, 2 chunks: 13 in six jobs
    n_jobs = -(-(2 * 96 * n_cus + 7) * len(lengths) // 13)
    sizes = [lengths[i % len(lengths)] for i in range(n_jobs)]
    offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])])
    total = int(offs[-1])
    gen = torch.Generator(device="cuda").manual_seed(7)
    amp = torch.repeat_interleave(torch.linspace(0.0, 0.2, n_jobs, device="cuda"), torch.tensor(np.diff(offs), device="cuda"))
    c = torch.randn(total, device="cuda", generator=gen)
    g = torch.randn(total, device="cuda", generator=gen) * amp
    ws = [c + g + 0.05 * torch.randn(total, device="cuda", generator=gen) for _ in range(2)]
    del g, amp
    plan = merge.StockPlan("cuda")
    outs = []
    for i, n in enumerate(sizes):
        o = int(offs[i])
        outs.append(plan.add([w[o:o + n] for w in ws], c[o:o + n]))
        assert plan.jobs[-1].base == c.data_ptr() + 4 * o  # the view itself, not a staged copy
    plan.run()
    torch.cuda.synchronize()
    L = importlib.import_module("vl_merging_amd._lib")
    hdr = L.StockHeader.from_buffer_copy(plan.ws[:56].cpu().numpy().tobytes())
    assert hdr.n_chunks > 2 * 96 * n_cus and hdr.n_jobs == n_jobs
    rows = plan.report()
    for r in rows:
        cos_pair, cos, t, scale = R.ratio(r["sq"], [p["dot"] for p in r["pairs"]])
        assert bits((r["pairs"][0]["cosine"], r["cos"], r["t"], r["scale"])) == bits((cos_pair[0], cos, t, scale)), r
    assert len({r["scale_bits"] for r in rows}) > n_jobs // 2  # neighbours differ in scale: a stale one would show
    scales = torch.tensor([r["scale"] for r in rows], dtype=torch.float32, device="cuda")
    assert [R.f32_bits(float(v)) for v in scales[:64].cpu()] == [r["scale_bits"] for r in rows[:64]]
    for i in list(range(0, n_jobs, 997)) + [n_jobs - 1]:  # the sums of a sample of the jobs against the restatement itself
        o, n = int(offs[i]), sizes[i]
        exp, row = R.stock(c[o:o + n].cpu().numpy(), [w[o:o + n].cpu().numpy() for w in ws])
        assert bits({**rows[i], "dst": None}) == bits(row) and same_bits(outs[i], exp), i
    d = torch.zeros_like(c) + (ws[0] - c)
    d = d + (ws[1] - c)
    prod = torch.repeat_interleave(scales, torch.tensor(np.diff(offs), device="cuda")) * d
    want = c + prod
    got = torch.cat(outs).view(torch.int32)
    keep = torch.cat([torch.arange(int(offs[i]), int(offs[i]) + n, device="cuda") for i, n in enumerate(sizes)])
    assert torch.equal(got, want[keep].view(torch.int32))


def test_stock_position_in_a_plan_does_not_show(merge):
    a = aligned_job(12289, 3, seed=1)
    others = [planted_job(4097, 2, seed=2), aligned_job(70000, 2, seed=3)]
    outs1, rows1, plan1 = run_plan(merge, [a] + others)
    outs2, rows2, plan2 = run_plan(merge, others + [a])
    assert result_bytes(plan1)[:152] == result_bytes(plan2)[2 * 152:]
    assert same_bits(outs1[0], outs2[2].cpu().numpy())
    exp, row = R.stock(a["c"], a["srcs"])
    assert bits({**rows1[0], "dst": None}) == bits({**rows2[2], "dst": None}) == bits(row) and same_bits(outs1[0], exp)
    assert 0.05 < row["cos"] < 0.95
    check_jobs([a] + others, outs1, rows1)


def test_stock_run_three_times_same_bytes_inputs_untouched(merge):
    jobs = [aligned_job(70001, 3, seed=1), planted_job(4097, 2, seed=2), aligned_job(3, 2, seed=3), aligned_job(5000, 4, seed=4)]
    plan = merge.StockPlan("cuda")
    outs = [plan.add([torch.from_numpy(s).cuda() for s in j["srcs"]], torch.from_numpy(j["c"]).cuda(), name=str(i))
            for i, j in enumerate(jobs)]
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
        raw.append(result_bytes(plan))
        reports.append(plan.report())
    assert got[0] == got[1] == got[2] and raw[0] == raw[1] == raw[2]
    assert bits(reports[0]) == bits(reports[1]) == bits(reports[2])
    check_jobs(jobs, outs, reports[0])
    assert [t.cpu().numpy().tobytes() for t in inputs] == before  # every source and every base: read only
    n_in = sum(j["c"].size * (len(j["srcs"]) + 1) for j in jobs)
    assert plan.bytes_read == 2 * 4 * n_in and plan.bytes_written == 4 * sum(j["c"].size for j in jobs)  # two passes read


def test_stock_hand_cases_on_the_device(merge):
    """The cases of test_stock_cpu.py that are written from constants, as jobs of one plan."""
    f32 = lambda *v: np.array(v, dtype=F)  # noqa: E731
    c = f32(0.5, -1.25, 3.0, 0.0, 7.0, 1e-3)
    w = f32(1.5, -0.25, 2.0, 0.125, 7.0, 1e-3)
    w0, w1 = c.copy(), c.copy()
    w0[:3] += f32(1, -2, 0.5)
    w1[3:] += f32(4, 0.25, 1)
    c4, x = f32(1, 2, 3, 4), f32(0.5, -0.25, 2, 0.125)
    c2 = f32(2, -1)
    jobs = [job(c, [w, w.copy()]), job(c, [w, w.copy(), w.copy()]), job(c, [w0, w1]), job(c4, [c4 + x, c4 - x]),
            job(c4, [c4.copy(), c4 + x]), job(c4, [c4 + x]), job(c2, [c2 + f32(1, 0), c2 + f32(3, 4)])]
    outs, rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows)
    same, three, disjoint, opposite, zero, one, hand = rows
    assert (same["cos"], same["t"], same["scale"]) == (1.0, 1.0, 0.5) and outs[0].cpu().numpy().tolist() == w.tolist()
    assert (three["cos"], three["t"], three["scale_bits"]) == (1.0, 1.0, int(F(1 / 3).view(np.uint32)))
    assert (disjoint["cos"], disjoint["t"], disjoint["scale_bits"]) == (0.0, 0.0, 0) and outs[2].cpu().numpy().tobytes() == c.tobytes()
    assert (opposite["cos"], opposite["t"]) == (-1.0, 0.0) and outs[3].cpu().numpy().tobytes() == c4.tobytes()
    assert zero["sq"][0] == 0.0 and bits(zero["pairs"][0]["cosine"]) == bits(0.0) and zero["t"] == 0.0
    assert (one["pairs"], one["cos"], one["t"], one["scale"]) == ([], 0.0, 1.0, 1.0) and outs[5].cpu().numpy().tolist() == (c4 + x).tolist()
    assert hand["sq"] == [1.0, 25.0] and hand["pairs"][0] == {"a": 0, "b": 1, "dot": 3.0, "cosine": 0.6}
    assert (hand["cos"], hand["t"], hand["scale"]) == (0.6, 1.2 / 1.6, 0.375)


def test_stock_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.StockPlan("cuda")
    a = torch.arange(64, device="cuda", dtype=torch.float32)
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a)
    with pytest.raises(L.VlmError):
        plan.add([a, torch.zeros(32, device="cuda")], a)
    with pytest.raises(L.VlmError):
        plan.add([a, a], torch.zeros(32, device="cuda"))
    with pytest.raises(L.VlmError):
        plan.add([a.double()], a)
    with pytest.raises(L.VlmError):
        plan.report()  # nothing has run
    assert plan.jobs == []
    out = plan.add([a + 1, 2 * a + 1], a)
    ws = torch.empty(lib.vlm_stock_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    assert lib.vlm_stock_plan_upload((L.StockJob * 1)(*plan.jobs), 1, L.ptr(ws), 512, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    buf = torch.zeros(256, device="cuda")
    src0 = plan.jobs[0].src[0]
    for field, value, rc in (("n_src", 0, -1), ("n_src", 5, -1), ("n_elem", 0, -1), ("base", 0, -1), ("dst", 0, -1),
                             ("base", buf.data_ptr() + 4, -1), ("src0", buf.data_ptr() + 8, -1), ("src0", 0, -1),
                             ("dst", a.data_ptr(), -1), ("dst", src0, -1), ("dst", src0 + 16, -1), ("dst", buf.data_ptr() + 4, -1),
                             ("dst", buf.data_ptr(), 0), ("n_src", 1, 0)):
        bad = L.StockJob.from_buffer_copy(bytes(plan.jobs[0]))
        if field == "src0":
            bad.src[0] = value
        else:
            setattr(bad, field, value)
        got = lib.vlm_stock_plan_upload((L.StockJob * 1)(bad), 1, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert got == rc, (field, value)  # another dst and n_src = 1 are fine: the controls that pass
    plan.run()
    torch.cuda.synchronize()
    # x_0 = 1, x_1 = a + 1: the restatement, and scale read back
    exp, row = R.stock(a.cpu().numpy(), [(a + 1).cpu().numpy(), (2 * a + 1).cpu().numpy()], name=None)
    assert same_bits(out, exp) and bits(plan.report()[0]) == bits(row) and 0 < row["t"] < 1


def restate_state(sd, central, cfg, layers=range(12), want=None):
    """dst -> (expected tensor, report row | None) for the block tensors of `layers`; single-source layers: the oracle's
    task-vector job."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            if want is not None and dst not in want:
                continue
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None)
            else:
                out, row = R.stock(central[dst], srcs, name=dst)
                exp[dst] = (out.reshape(central[dst].shape), row)
    return exp


@pytest.fixture(scope="module")
def tiny():
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    return sd_np, central_np, to_dev(sd_np), to_dev(central_np)


@pytest.mark.parametrize("case", sorted(CASES))
def test_stock_merge_tiny_matches_restatement(case, merge, tiny):
    sd_np, central_np, sd, central = tiny
    cfg = merge_cfg(sum_lambda=0.75, **CASES[case])
    central_before = {k: v.clone() for k, v in central.items()}
    rows, plans = [], []
    res = merge.stock_merge(sd, cfg, central_weight={"state_dict": central}, report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg)
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
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.StockPlan)
    if case == "used_vqa":
        assert isinstance(plans[1], merge.MergePlan)
    assert json.loads(json.dumps(rows)) == rows  # the CLI's report rows
    # the method has no lambda: config["sum_lambda"] is not read
    for lam in (0.5, 2):
        other = merge.stock_merge(sd, dict(cfg, sum_lambda=lam), central_weight=central)
        torch.cuda.synchronize()
        assert all(same_bits(other[k], res[k].cpu().numpy()) for k in res if is_block(k)), lam
    no_lam = {k: v for k, v in cfg.items() if k != "sum_lambda"}
    other = merge.stock_merge(sd, no_lam, central_weight=central)
    torch.cuda.synchronize()
    assert all(same_bits(other[k], res[k].cpu().numpy()) for k in res if is_block(k))
    with pytest.raises(KeyError):
        merge.stock_merge(sd, cfg, central_weight={k: v for k, v in central.items() if "blocks.3.norm1.weight" not in k})


def test_stock_base_size(merge):
    """Base size: t and scale of all 156 tensors against step 3 (in python doubles) applied to the sums PairStatsPlan leaves for
    the same inputs; the output bytes of the largest weight, a bias and a tensor with three sources against the restatement; and
    run() returns while its three launches are still queued."""
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    rows, plans, ps = [], [], []
    res = merge.stock_merge(sd, cfg, central_weight=central, report_out=rows, plan_out=plans)
    merge.expert_stats(sd, cfg, central_weight=central, plan_out=ps)
    torch.cuda.synchronize()
    stats = ps[0].report()
    assert len(rows) == len(stats) == 12 * 13 and [r["dst"] for r in rows] == [s["dst"] for s in stats]
    for r, s in zip(rows, stats):
        cos_pair, cos, t, scale = R.ratio(s["sq"], [p["dot"] for p in s["pairs"]])
        assert bits(r["sq"]) == bits(s["sq"]) and bits([p["dot"] for p in r["pairs"]]) == bits([p["dot"] for p in s["pairs"]]), r["dst"]
        assert bits([p["cosine"] for p in r["pairs"]]) == bits(cos_pair), r["dst"]
        assert bits((r["cos"], r["t"], r["scale"])) == bits((cos, t, scale)) and r["scale_bits"] == R.f32_bits(scale), r["dst"]
        assert 0.0 <= r["t"] <= 1.0
    sample = ["transformer.blocks.0.mlp.fc1.weight", "transformer.blocks.5.attn.proj.bias", "transformer.blocks.11.mlp.fc2.weight"]
    exp = restate_state(sd_np, central_np, cfg, want=set(sample))
    assert sorted(exp) == sorted(sample) and len(exp[sample[2]][1]["sq"]) == 3
    by_dst = {r["dst"]: r for r in rows}
    for k, (want, row) in exp.items():
        assert same_bits(res[k], want) and bits(by_dst[k]) == bits(row), k
    plan = plans[0]
    assert plan.bytes_written == 4 * sum(v.numel() for k, v in res.items() if is_block(k))
    assert plan.bytes_read == 2 * 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs)
    # no host synchronisation between upload and the end of run(), although the apply pass waits for the fold's scalars: the
    # ENQUEUE is timed behind a 0.2 s spin kernel on the same stream, as test_pairstats_base_size does.  The spin's own length is
    # checked, so the bound cannot pass vacuously.
    import time
    L = importlib.import_module("vl_merging_amd._lib")
    before = [res[k].clone() for k in sample]
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
    print("stock enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "StockPlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert bits(plan.report()) == bits(rows) and all(torch.equal(res[k].view(torch.int32), b.view(torch.int32)) for k, b in zip(sample, before))


def test_merge_ckpt_stock_as_a_child_process(merge, tmp_path, tiny):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    _, _, sd, central = tiny
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in central.items()}}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "stock.ckpt", tmp_path / "stock.json"
    cmd = [sys.executable, TOOL, "--method", "stock", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--lambda", "0.3", "--density", "0.4", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = merge.stock_merge(sd, merge_cfg(sum_lambda=0.75), central_weight=central, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert rep["method"] == "stock" and (rep["density"], rep["drop"], rep["seed"], rep["epsilon"]) == (None,) * 4
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows  # json round-trips a double exactly


def test_model_method_is_the_same_merge(merge, pkg, tiny):
    """ViLTransformerSS.stock_merge forwards to merge.stock_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    _, _, sd, central = tiny
    want = merge.stock_merge(sd, Stub.hparams.config, central_weight=central)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.stock_merge(Stub(), sd)
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(same_bits(got[k], want[k].cpu().numpy()) for k in want if is_block(k))
