"""The spherical merge on the GPU (csrc/sphere.hip through the C ABI) against the restatement of the rule (sphere_restatement.py).
What is compared by its bytes: sq, dot, rho, status, the row counters rows_linear / rows_zero, coef32 against float32 of the
device's own coef64, and the output against the restatement's step 4 fed the device's own coef32.  What is compared by a bound:
coef64 against the restatement, which calls python's math.acos / sin / cos where the device calls its own library: at most 2^-44
of the group's largest |coef| (the rule moves by at most 2^-49.8 when every such call is perturbed by 4 ulp; the margin is for a
looser device library); coef32 against the restatement's: no coefficient by more than one fp32 ulp, and at most 1 group in 1 000
different at all.  `resid` (and its maximum over a job's rows) is the size of the last step of the iteration, a few ulp of noise on
a converged input (the root of nrm2's rounding noise, about 1e-8, where the Gram matrix is near-dependent): it is held to be finite
and below 2^-20, not to bytes.  Coefficients are compared on well-posed inputs only:
nearly orthogonal random sources and sources with a shared component for n >= 64, positive collinear ones for n < 64, planted zero
sources and exactly opposite pairs.  The reference has no such merge."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, is_block, to_dev
from test_stock_gpu import SIZES
from pairstats_restatement import bits
from oracle import merge_oracle as mo
import sphere_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F, D = np.float32, np.float64
BOUND = 2.0 ** -44
RESID = 2.0 ** -20  # nrm2 of a vanished step is rounding noise of a few 2^-53: its root, the last step, stays below 2^-20 with room
WORST = {"coef64": 0.0}  # the worst deviation of a device coefficient seen in this session, relative to its group's largest


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nsphere: worst |coef64 - restatement| / max |coef| on the device: %.3e = 2^%.1f (bound 2^-44)"
          % (WORST["coef64"], math.log2(WORST["coef64"]) if WORST["coef64"] > 0 else float("-inf")))


# ------------------------------------------------------------------------------------------------------------------ inputs
def sources(n, S, seed, row_len=0, base=True, kind=None):
    """Well-posed sources (see the module's docstring), float32 [n] each, and a central tensor or None.  Groups (the tensor, or rows
    of row_len) shorter than 64 get positive collinear task vectors; longer ones random directions (`kind` "orth") or a shared
    component (`kind` "shared"; default: by the seed's parity)."""
    rng = np.random.default_rng(seed)
    L = row_len or n
    c = rng.standard_normal(n).astype(F) if base else None
    if L < 64:
        g = rng.standard_normal(n).astype(F)
        g[g == 0] = F(1)
        xs = [(np.repeat(rng.uniform(0.5, 2.0, n // L).astype(F), L) * g).astype(F) for _ in range(S)]
    else:
        xs = [rng.standard_normal(n).astype(F) * F(0.1 * (1 + m)) for m in range(S)]
        if (kind or ("shared" if seed % 2 else "orth")) == "shared":
            g = rng.standard_normal(n).astype(F) * F(0.2)
            xs = [(x + g).astype(F) for x in xs]
    if c is None:
        return None, xs
    srcs = [(c + x).astype(F) for x in xs]
    return c, srcs


def job(c, srcs, w=None, lam=None, row_len=0):
    S = len(srcs)
    w = [0.5 + 0.25 * m for m in range(S)] if w is None else w
    return dict(c=c, srcs=srcs, w=w, lam=(0.75 if c is not None else 1.0) if lam is None else lam, row_len=row_len)


def make(n, S, seed, row_len=0, base=True, **kw):
    return job(*sources(n, S, seed, row_len, base, kw.pop("kind", None)), row_len=row_len, **kw)


def plant(j, row, what):
    """Plants in row `row` of a row job (or in the whole tensor): "zero": source 0's task vector is zero; "zeros": every task vector
    is zero; "opposite": sources 0 and 1 are exactly opposite and, with equal weights and the others zero, the row is LINEAR."""
    L = j["row_len"] or j["srcs"][0].size
    sl = slice(row * L, (row + 1) * L)
    c = j["c"][sl] if j["c"] is not None else np.zeros(L, F)
    if what == "zero":
        j["srcs"][0][sl] = c
    elif what == "zeros":
        for s in j["srcs"]:
            s[sl] = c
    else:
        x = (np.arange(1, L + 1) % 7 + 1).astype(F) / F(8)  # dyadic: c + x - c == x needs c dyadic too
        cd = np.round(c * 8) / 8
        if j["c"] is not None:
            j["c"][sl] = cd
        j["srcs"][0][sl] = cd + x
        j["srcs"][1][sl] = cd - x
        for s in j["srcs"][2:]:
            s[sl] = cd
    return j


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_plan(merge, jobs, tensors=None):
    """jobs: list of job(...).  Returns (outputs, raw results, plan); every job's coef32 is in plan.coefs."""
    plan = merge.SpherePlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base, srcs = tensors[i] if tensors else (None if j["c"] is None else dev(j["c"]), [dev(s) for s in j["srcs"]])
        outs.append(plan.add(srcs, base, j["w"], lam=j["lam"], row_len=j["row_len"] or None, coef_out=True, name=str(i)))
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.results(), plan


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))


def ulps(a, b):
    """|a - b| in units of the fp32 spacing at the larger magnitude's binade, elementwise (float32 arrays)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return np.abs(a.astype(D) - b.astype(D)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F)).astype(D)


def check_coef32(dev32, mine32, groups):
    """The device's coef32 against the restatement's, [groups, S] each: none by more than one ulp, at most 1 group in 1 000 at all."""
    dev32, mine32 = np.asarray(dev32, dtype=F).reshape(groups, -1), np.asarray(mine32, dtype=F).reshape(groups, -1)
    differ = dev32.view(np.uint32) != mine32.view(np.uint32)
    if differ.any():
        assert np.max(ulps(dev32[differ], mine32[differ])) <= 1.0, (dev32[differ][:4], mine32[differ][:4])
    assert 1000 * int(differ.any(axis=1).sum()) <= groups, "%d of %d groups differ in a coefficient" % (differ.any(axis=1).sum(), groups)


def check_jobs(jobs, outs, results, plan, coefficients=True):
    """Every job against the restatement (see the module's docstring)."""
    assert len(results) == len(jobs)
    for i, (j, out, res) in enumerate(zip(jobs, outs, results)):
        S, L = len(j["srcs"]), j["row_len"]
        coef_dev = plan.coefs[i].cpu().numpy()
        assert coef_dev.shape == ((j["srcs"][0].size // L if L else 1), 4) and not coef_dev[:, S:].any()
        exp, rs = R.sphere(j["c"], j["srcs"], j["w"], j["lam"], L, coef32=coef_dev if L else coef_dev[0])
        assert same_bits(out, exp), (i, j["srcs"][0].size, S, L)  # step 4 fed the device's own coefficients: bit for bit
        if L == 0:
            assert bits([res.sq[m] for m in range(S)]) == bits(rs["sq"]) and bits([res.dot[p] for p in range(len(rs["dot"]))]) == bits(rs["dot"]), i
            assert not any(res.sq[m] for m in range(S, 4)) and not any(res.dot[p] for p in range(len(rs["dot"]), 6)) and res.reserved == 0
            c64 = [res.coef64[m] for m in range(S)]
            assert [R.f32_bits(res.coef32[m]) for m in range(S)] == [R.f32_bits(R.f32(x)) for x in c64], i  # one rounding, on its own values
            assert coef_dev[0, :S].tobytes() == np.array([res.coef32[m] for m in range(S)], dtype=F).tobytes()
            assert merge_status(res.status) == rs["status"] and bits(res.rho) == bits(rs["rho"]), (i, res.status, rs["status"])
            assert (res.rows_linear, res.rows_zero, res.resid_max) == (0, 0, 0.0) and math.isfinite(res.resid) and 0 <= res.resid < RESID
            if coefficients:
                big = max(abs(x) for x in rs["coef64"])
                dev64 = max(abs(a - b) for a, b in zip(c64, rs["coef64"]))
                if big > 0:
                    WORST["coef64"] = max(WORST["coef64"], dev64 / big)
                assert dev64 <= BOUND * big, (i, S, dev64 / big if big else 0.0, c64, rs["coef64"])
                check_coef32(coef_dev[:, :S], [rs["coef32"]], 1)  # one group: it may not differ at all
        else:
            lin, zero, rmax = R.counters(rs)
            assert (res.rows_linear, res.rows_zero) == (lin, zero), (i, L)
            assert math.isfinite(res.resid_max) and 0 <= res.resid_max < RESID and res.status == 0 and not any(res.sq) and not any(res.coef64)
            if coefficients:
                check_coef32(coef_dev[:, :S], [r["coef32"] for r in rs], len(rs))


def merge_status(s):
    return {0: R.OK, 1: R.LINEAR, 2: R.ZERO}[int(s)]


# ------------------------------------------------------------------------------------------------------------ tensor groups
@pytest.mark.parametrize("n", [n for n in SIZES if n <= 70001])
def test_sphere_tensor_groups_ragged_sizes(n, merge):
    """The tail alone, a partial wave, one full chunk, a chunk plus tail, 18 chunks: S = 1 .. 4, with and without a base, in one plan."""
    jobs = [make(n, S, seed=n + S + 10 * base, base=bool(base)) for S in (1, 2, 3, 4) for base in (1, 0)]
    outs, results, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, results, plan)
    for j, res in zip(jobs, results):
        if len(j["srcs"]) == 1:
            assert (res.coef64[0], res.coef32[0], res.status, res.resid) == (1.0, 1.0, 0, 0.0)


def test_sphere_same_sums_as_model_stock(merge):
    """For the same device tensors, sq and dot are the bytes StockPlan leaves: one reducer serves both."""
    specs = [(70001, 4), (12289, 3), (4097, 2), (5, 2), (1 << 18, 3), (1023, 1)]
    jobs = [make(n, S, seed=40 + i) for i, (n, S) in enumerate(specs)]
    tensors = [(dev(j["c"]), [dev(s) for s in j["srcs"]]) for j in jobs]
    outs, results, plan = run_plan(merge, jobs, tensors)
    stock = merge.StockPlan("cuda")
    for base, srcs in tensors:
        stock.add(srcs, base)
    stock.run()
    torch.cuda.synchronize()
    for mine, theirs in zip(results, stock.results()):
        assert bytes(mine)[:80] == bytes(theirs)[:80]  # sq[4], dot[6]
    check_jobs(jobs[:4], outs[:4], results[:4], plan)


def test_sphere_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one- and two-chunk tensor jobs of 1 .. 4099 elements and 1 .. 4 sources (helpers/merge_inputs.tiny_jobs), in
    turn with and without a base, every input a 16-byte aligned view into one device buffer, used unstaged: every workgroup's run
    of chunks in the reducer holds several jobs, so it loads a new first-record index at nearly every step (and the apply pass new
    coefficients).  tiny_jobs is handed this file's `sources` as its generator, not test_ties_gpu's `planted`: planted data is
    ill-posed for a spherical mean (its one-element jobs are exactly opposite one-dimensional sources, where the restatement's own
    coefficients move by their whole size under a 4-ulp change of acos and its last step is 4e-3), and the coefficients are
    compared on well-posed inputs only.  With `sources` the restatement moves by 2^-49.4 at most over these jobs."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    # not through tiny_jobs' one-entry cache: the planted jobs of the other files stay in it
    data = tiny_jobs.__wrapped__(n_cus, lambda n, S, seed: sources(n, S, seed, base=seed % 2 == 0))
    jobs = [job(c, srcs) for c, srcs in data]
    assert [j["c"] is None for j in jobs[:4]] == [False, True, False, True]
    views = iter(one_buffer([a for j in jobs for a in ([] if j["c"] is None else [j["c"]]) + j["srcs"]]))
    tensors = []
    for j in jobs:
        base = None if j["c"] is None else next(views)
        tensors.append((base, [next(views) for _ in j["srcs"]]))
    outs, results, plan = run_plan(merge, jobs, tensors)
    for pj, (base, srcs) in zip(plan.jobs, tensors):  # the views themselves, not staged copies
        assert (pj.base or 0) == (0 if base is None else base.data_ptr())
        assert [pj.src[m] for m in range(len(srcs))] == [s.data_ptr() for s in srcs]
    hdr = plan.HEADER.from_buffer_copy(plan.ws[:72].cpu().numpy().tobytes())
    assert hdr.n_tiles == 0 and hdr.n_chunks == sum(max(1, -(-(j["srcs"][0].size // 4) // 1024)) for j in jobs) > 2 * 12 * n_cus
    check_jobs(jobs, outs, results, plan)
    assert len({bits(r.sq[0]) for r in results}) > len(jobs) // 2  # neighbours differ in their sums: a record at a stale index would show


def test_sphere_planted_zero_sources_and_opposite_pairs(merge):
    n = 4097
    jobs = [plant(make(n, 3, seed=1), 0, "zero"), plant(make(n, 2, seed=2, w=[0.5, 0.5]), 0, "opposite"),
            plant(make(n, 3, seed=3, w=[0.25, 0.25, 0.5], base=False), 0, "opposite"), plant(make(n, 2, seed=4), 0, "zeros"),
            plant(make(n, 2, seed=5, w=[0.7, 0.3]), 0, "opposite"), plant(make(n, 4, seed=6, w=[0.0, 1.0, 2.0, 0.0]), 0, "zero")]
    outs, results, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, results, plan)
    zero, opp, opp3, zeros, heavier, w0 = results
    assert zero.status == 0 and zero.coef64[0] == 0.0 and zero.sq[0] == 0.0 and zero.coef64[1] > 0
    assert (opp.status, opp.coef64[0], opp.coef64[1], opp.resid) == (1, 0.5, 0.5, 0.0) and same_bits(outs[1], jobs[1]["c"] + F(0.75) * np.zeros(n, F))
    assert (opp3.status, [opp3.coef64[m] for m in range(3)]) == (1, [0.5, 0.5, 0.0])  # the zero third source drops out with its weight
    assert (zeros.status, zeros.rho, zeros.coef32[0], zeros.coef32[1]) == (2, 0.0, 0.0, 0.0) and same_bits(outs[3], jobs[3]["c"] + F(0.75) * np.zeros(n, F))
    assert heavier.status == 0 and abs(heavier.coef64[0] - heavier.coef64[1] - 1.0) < 1e-12  # converges to the heavier side
    assert w0.status == 0 and (w0.coef64[0], w0.coef64[3]) == (0.0, 0.0)


# --------------------------------------------------------------------------------------------------------------- row groups
def row_counts(L):
    per = 4096 // L
    return [1, 2, (2 * per + 3) if per < 64 else per + 5]  # the last leaves a partial last tile


@pytest.mark.parametrize("L", [1, 3, 4, 64, 65, 768, 4096])
def test_sphere_row_groups(L, merge):
    """One row, two rows, and full tiles plus a partial one; S = 2 .. 4 and 1; with and without a base.  4096 / L rows make a tile:
    1, 5, 63 and 64 of them (one batch of step 3, at most one row per lane of a wave), 1024, 1365 and 4096 (several batches of 256).
    Zero rows, zero sources and opposite pairs are planted where there are rows to spare."""
    jobs = []
    for k, rows in enumerate(row_counts(L)):
        for base in (True, False):
            S = 2 + (k + base) % 3
            j = make(rows * L, S, seed=L + 7 * k + base, row_len=L, base=base, w=[0.5, 0.5] + [0.25] * (S - 2))
            if rows > 4:
                plant(plant(plant(j, 1, "zero"), rows - 1, "opposite"), 3, "zeros")
            jobs.append(j)
    jobs.append(make(row_counts(L)[2] * L, 1, seed=L, row_len=L))
    outs, results, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, results, plan)
    assert (results[4].rows_zero, results[4].rows_linear) == (1, 1)  # a zero third source drops out: the pair alone is LINEAR
    hdr = plan.HEADER.from_buffer_copy(plan.ws[:72].cpu().numpy().tobytes())
    per = 4096 // L
    assert hdr.n_chunks == 0 and hdr.n_tiles == sum(-(-(j["srcs"][0].size // L) // per) for j in jobs)
    one = plan.coefs[-1].cpu().numpy()
    assert (one[:, 0] == 1).all() and not one[:, 1:].any()  # S = 1: coef == 1 exactly, in every row


def dozen_jobs():
    spec = [(12289, 0), (768 * 7, 768), (4097, 0), (3 * 100, 3), (1 << 16, 0), (65 * 70, 65), (8191, 0), (4096 * 2, 4096), (5, 0),
            (64 * 130, 64), (70000, 0), (4 * 1500, 4), (1023, 0)]
    return [make(n, 1 + (i + 1) % 4, seed=300 + i, row_len=L, base=bool(i % 3)) for i, (n, L) in enumerate(spec)]


def test_sphere_a_dozen_mixed_jobs_in_one_plan(merge):
    """Tensor jobs and row jobs in turn, S = 1 .. 4, with and without a base: both tables of one plan, four launches."""
    jobs = dozen_jobs()
    outs, results, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, results, plan)
    hdr = plan.HEADER.from_buffer_copy(plan.ws[:72].cpu().numpy().tobytes())
    assert hdr.n_jobs == 13 and hdr.n_chunks > 0 and hdr.n_tiles > 0
    rows = plan.report()
    assert json.loads(json.dumps(rows)) == rows and [r["row_len"] for r in rows] == [j["row_len"] for j in jobs]
    assert all(("coef64" in r) == (r["row_len"] == 0) and ("rows_linear" in r) == (r["row_len"] != 0) for r in rows)
    n_in = sum(j["srcs"][0].size * (len(j["srcs"]) + (j["c"] is not None)) * (1 if j["row_len"] else 2) for j in jobs)
    assert plan.bytes_read == 4 * n_in and plan.bytes_written == 4 * sum(j["srcs"][0].size for j in jobs)


def result_bytes(plan):
    hdr = plan.HEADER.from_buffer_copy(plan.ws[:72].cpu().numpy().tobytes())
    return plan.ws[hdr.results_off: hdr.results_off + 176 * len(plan.jobs)].cpu().numpy().tobytes()


def test_sphere_position_in_a_plan_does_not_show(merge):
    a, b = make(12289, 3, seed=1), make(768 * 7, 3, seed=2, row_len=768)
    others = [make(4097, 2, seed=3), make(64 * 70, 2, seed=4, row_len=64, base=False), make(70000, 2, seed=5)]
    outs1, _, plan1 = run_plan(merge, [a, b] + others)
    outs2, _, plan2 = run_plan(merge, others + [b, a])
    r1, r2 = result_bytes(plan1), result_bytes(plan2)
    assert r1[:176] == r2[4 * 176:] and r1[176:352] == r2[3 * 176:4 * 176]
    assert same_bits(outs1[0], outs2[4].cpu().numpy()) and same_bits(outs1[1], outs2[3].cpu().numpy())
    assert plan1.coefs[1].cpu().numpy().tobytes() == plan2.coefs[3].cpu().numpy().tobytes()
    check_jobs([a, b] + others, outs1, plan1.results(), plan1)


def test_sphere_run_three_times_same_bytes_inputs_untouched(merge):
    jobs = [make(70001, 3, seed=1), plant(make(65 * 70, 2, seed=2, row_len=65, w=[0.5, 0.5]), 5, "opposite"), make(3, 2, seed=3),
            make(4096 * 3, 4, seed=4, row_len=4096, base=False), make(5000, 4, seed=5, base=False)]
    plan = merge.SpherePlan("cuda")
    outs = [plan.add([dev(s) for s in j["srcs"]], None if j["c"] is None else dev(j["c"]), j["w"], lam=j["lam"],
                     row_len=j["row_len"] or None, coef_out=True, name=str(i)) for i, j in enumerate(jobs)]
    inputs = [t for t in plan.keep if all(t is not o for o in outs)]
    assert len(inputs) == sum(len(j["srcs"]) + (j["c"] is not None) for j in jobs)
    before = [t.cpu().numpy().tobytes() for t in inputs]
    got, raw, coefs = [], [], []
    for _ in range(3):  # every run writes into outputs and coefficients pre-filled with NaN
        for o in outs + plan.coefs:
            o.fill_(float("nan"))
        plan.run()
        torch.cuda.synchronize()
        got.append([o.cpu().numpy().tobytes() for o in outs])
        coefs.append([c.cpu().numpy().tobytes() for c in plan.coefs])
        raw.append(plan.ws.cpu().numpy().tobytes())  # the whole workspace: tables, records, results, counters
    assert got[0] == got[1] == got[2] and raw[0] == raw[1] == raw[2] and coefs[0] == coefs[1] == coefs[2]
    check_jobs(jobs, outs, plan.results(), plan)
    assert plan.results()[1].rows_linear == 1  # counted once per run, not three times
    assert [t.cpu().numpy().tobytes() for t in inputs] == before  # every source and every base: read only


# --------------------------------------------------------------------------------------------------------------- the upload
def test_sphere_upload_rejections_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.SpherePlan("cuda")
    a = torch.arange(64, device="cuda", dtype=torch.float32)
    for bad in (dict(weights=[1.0]), dict(weights=[-1.0, 2.0]), dict(weights=[0.0, 0.0]), dict(weights=[float("nan"), 1.0]),
                dict(weights=[float("inf"), 1.0]), dict(weights=[1, 1], row_len=5), dict(weights=[1, 1], row_len=0),
                dict(weights=[1, 1], base=None, lam=0.5)):
        with pytest.raises(L.VlmError):
            plan.add([a + 1, 2 * a + 1], bad.pop("base", a), **bad)
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, [1] * 5)
    with pytest.raises(L.VlmError):
        plan.add([torch.zeros(2, 8192, device="cuda")], None, [1], rows=True)  # a row longer than a tile
    with pytest.raises(L.VlmError):
        plan.report()  # nothing has run
    assert plan.jobs == [] and plan.coefs == []
    out = plan.add([a + 1, 2 * a + 1], a, [0.25, 0.75], lam=0.5, row_len=16, coef_out=True)
    ws = torch.empty(lib.vlm_sphere_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    good = plan.jobs[0]

    def upload(**fields):
        j = L.SphereJob.from_buffer_copy(bytes(good))
        for k, v in fields.items():
            if k.startswith("w"):
                j.w[int(k[1:])] = v
            else:
                setattr(j, k, v)
        return lib.vlm_sphere_plan_upload((L.SphereJob * 1)(j), 1, L.ptr(ws), ws.numel(), L.stream_ptr())

    assert lib.vlm_sphere_plan_upload((L.SphereJob * 1)(good), 1, L.ptr(ws), 256, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    buf = torch.zeros(256, device="cuda")
    for fields in (dict(w0=-0.25), dict(w1=float("nan")), dict(w0=float("inf")), dict(w0=0.0, w1=0.0),  # the weights
                   dict(row_len=5), dict(row_len=4097), dict(row_len=48),                                # a bad row_len
                   dict(base=0, lam=0.5),                                                                # lam != 1 without a base
                   dict(coef_out=out.data_ptr()), dict(coef_out=a.data_ptr() + 16), dict(coef_out=good.src[1] + 240),
                   dict(coef_out=buf.data_ptr() + 4), dict(dst=a.data_ptr()), dict(dst=good.src[0] + 16), dict(n_src=0), dict(n_elem=0)):
        assert upload(**fields) == -1, fields
    for fields in (dict(), dict(base=0, lam=1.0), dict(row_len=0), dict(w0=0.0), dict(coef_out=0), dict(coef_out=buf.data_ptr()),
                   dict(n_src=1), dict(row_len=64), dict(row_len=1, coef_out=buf.data_ptr())):
        assert upload(**fields) == 0, fields  # the controls that pass
    plan.run()
    torch.cuda.synchronize()
    j = job(a.cpu().numpy(), [(a + 1).cpu().numpy(), (2 * a + 1).cpu().numpy()], [0.25, 0.75], 0.5, 16)
    check_jobs([j], [out], plan.results(), plan)


# --------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tiny():
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    return sd_np, central_np, to_dev(sd_np), to_dev(central_np)


def restate_state(sd, central, cfg, on, rows, lam, coefs=None):
    """dst -> (expected tensor, the restatement's result | None) for the block tensors; single-source layers: the oracle's job.
    `coefs`: dst -> the device's coef32 of a tensor job, fed to step 4."""
    exp = {}
    for i in range(12):
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            c = central[dst] if on == "delta" else None
            if len(mods) == 1:
                exp[dst] = ((mo.taskvec(c, srcs, [1]) if on == "delta" else srcs[0]), None)
                continue
            if len(mods) == 3:
                r = cfg["merge_ratio"]
                w = [(2 / 3) * r, (2 / 3) * (1 - r), 1 / 3]
            else:
                w = [cfg["merge_ratio"], 1 - cfg["merge_ratio"]]
            L = (srcs[0].shape[-1] if srcs[0].ndim >= 2 else srcs[0].size) if rows else 0
            out, res = R.sphere(c, srcs, w, lam if on == "delta" else 1.0, L, coef32=None if coefs is None or L else coefs[dst])
            exp[dst] = (out.reshape(srcs[0].shape), res)
    return exp


@pytest.mark.parametrize("on,rows", [("weights", False), ("weights", True), ("delta", False), ("delta", True)])
@pytest.mark.parametrize("case", ["all", "used_vqa"])
def test_sphere_merge_tiny_matches_restatement(case, on, rows, merge, tiny):
    """The tensors of a tiny all_moe state are short (16 to 1 536 entries, rows of 16 and 32) and random, so a group is not
    always as well conditioned as the kernels' own tests ask: the coefficients are held to one fp32 ulp, and step 4 is exact
    wherever the device's coefficients are known (the tensor jobs' results).  A row job's coefficients are not kept here, so its
    output is held to the restatement's: the same bytes in all but at most 1 tensor in 1 000 rows' worth, and never further off than
    two ulp of a coefficient can carry."""
    sd_np, central_np, sd, central = tiny
    cfg = merge_cfg(sum_lambda=0.75, merge_ratio=0.3, **CASES[case])
    rep, plans = [], []
    kw = dict(central_weight={"state_dict": central}) if on == "delta" else {}
    res = merge.sphere_merge(sd, cfg, on=on, rows=rows, report_out=rep, plan_out=plans, **kw)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central) if on == "delta" else merge.merge_weights(sd, cfg)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    plan = plans[0]
    assert isinstance(plan, merge.SpherePlan) and len(plans) == (2 if case == "used_vqa" else 1)
    coefs = {r["dst"]: r["coef32"] for r in rep if r["row_len"] == 0}
    exp = restate_state(sd_np, central_np, cfg, on, rows, 0.75, coefs)
    n_block = groups = differ = 0
    for k, v in res.items():
        if not is_block(k):
            assert v is sd[k]  # pass-through by identity
            continue
        n_block += 1
        want, r = exp[k]
        if r is None:  # one source: the job merge_weights / sum_task_vectors issues for it
            assert same_bits(v, ref[k].cpu().numpy()) and same_bits(v, want), k
        elif not rows:
            assert same_bits(v, want), k
            row = [x for x in rep if x["dst"] == k][0]
            assert bits(row["sq"]) == bits(r["sq"]) and bits(row["rho"]) == bits(r["rho"]) and row["status"] == r["status"], k
            assert np.max(ulps(row["coef32"], r["coef32"])) <= 1.0, (k, row["coef32"], r["coef32"])
            groups += 1
            differ += [R.f32_bits(x) for x in row["coef32"]] != [R.f32_bits(x) for x in r["coef32"]]
        else:
            groups += len(r)
            if not same_bits(v, want):
                differ += 1
                assert np.max(np.abs(v.cpu().numpy().astype(D) - want.astype(D))) <= 2.0 ** -20 * float(np.max(np.abs(want))), k
    assert n_block == 12 * 13 and 1000 * differ <= max(groups, 1000), (differ, groups)
    assert [r["dst"] for r in rep] == [k for k in res if is_block(k) and exp[k][1] is not None]  # the walk's order
    assert json.loads(json.dumps(rep)) == rep
    if on == "weights":
        with pytest.raises(KeyError):  # merge_weights' KeyError behaviour
            merge.sphere_merge({k: v for k, v in sd.items() if "blocks.3.norm1.v.weight" not in k}, cfg, on=on, rows=rows)
    else:
        with pytest.raises(KeyError):  # sum_task_vectors': a key the central checkpoint lacks
            merge.sphere_merge(sd, cfg, on=on, rows=rows, central_weight={k: v for k, v in central.items() if "blocks.3.norm1.weight" not in k})


def test_merge_ckpt_slerp_as_a_child_process(merge, tmp_path, tiny):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    _, _, sd, central = tiny
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in central.items()}}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "slerp.ckpt", tmp_path / "slerp.json"
    cmd = [sys.executable, TOOL, "--method", "karcher", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--sphere-on", "delta", "--lambda", "0.3", "--ratio", "0.25", "with",
           "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = merge.sphere_merge(sd, merge_cfg(sum_lambda=0.3, merge_ratio=0.25), central_weight=central, on="delta", report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert (rep["method"], rep["sphere_on"], rep["sphere_rows"], rep["density"]) == ("karcher", "delta", False, None)
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows  # json round-trips a double exactly
    # `slerp` is the same method; on the weights, by row, no central checkpoint is named or read
    out2 = tmp_path / "slerp_rows.ckpt"
    cmd = [sys.executable, TOOL, "--method", "slerp", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out2), "--sphere-rows", "with",
           "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out2))
    want = merge.sphere_merge(sd, merge_cfg(), on="weights", rows=True)
    torch.cuda.synchronize()
    assert all(got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes() for k in want)


def test_model_method_is_the_same_merge(merge, pkg, tiny):
    """ViLTransformerSS.sphere_merge forwards to merge.sphere_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75, merge_ratio=0.4), central_weight=None)

    _, _, sd, central = tiny
    want = merge.sphere_merge(sd, Stub.hparams.config, on="weights", rows=True)
    got = vm.ViLTransformerSS.sphere_merge(Stub(), sd, rows=True)
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(same_bits(got[k], want[k].cpu().numpy()) for k in want if is_block(k))
    want = merge.sphere_merge(sd, Stub.hparams.config, central_weight=central, on="delta", lam=0.5)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.sphere_merge(Stub(), sd, on="delta", lam=0.5)
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(same_bits(got[k], want[k].cpu().numpy()) for k in want if is_block(k))


def test_rows_keep_the_norm_where_interpolation_shrinks_it(merge, tiny):
    """merge_ratio 0.5 and two modalities: every merged row is as long as the mean of the two experts' rows, to fp32 accuracy (the
    coefficients are rounded to fp32 and a row's L products and sums each err by 2^-24: 1e-5 relative covers both for L <= 32).
    The interpolation merge fails this: where the experts point apart its rows are shorter."""
    _, _, sd, _ = tiny
    cfg = merge_cfg(merge_ratio=0.5)
    got = merge.sphere_merge(sd, cfg, on="weights", rows=True)
    lerp = merge.merge_weights(sd, cfg)
    torch.cuda.synchronize()
    checked, short = 0, 0
    for i in range(10):  # the layers with two modalities
        for src, dst in mo._names(i):
            v, l = sd[src("v")].double(), sd[src("l")].double()
            L = v.shape[-1] if v.dim() >= 2 else v.numel()
            mean = 0.5 * (v.reshape(-1, L).norm(dim=1) + l.reshape(-1, L).norm(dim=1))
            mine = got[dst].double().reshape(-1, L).norm(dim=1)
            assert torch.all((mine - mean).abs() <= 1e-5 * mean), dst
            theirs = lerp[dst].double().reshape(-1, L).norm(dim=1)
            checked += mean.numel()
            short += int((theirs < 0.99 * mean).sum())
    assert checked > 1000 and short > checked // 2, (short, checked)
