"""DELLA merge on the GPU (csrc/della.hip through the C ABI) against the numpy restatement of the rule (della_restatement.py):
every comparison is over the uint32 view of the output and every counter, exactly.  The reference has no DELLA; the rule's three
consequences tie it to DarePlan (epsilon = 0) and to MergePlan's task-vector sum (the full window)."""
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
from della_restatement import LINEAR, TIES, della, window

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
F = np.float32
SEED = 20240617
MODES = {"linear": LINEAR, "ties": TIES}
WINDOWS = {"0.2+-0.1": window(0.2, 0.1), "1..2^32": (1, 2 ** 32), "0.5+-0": window(0.5, 0.0)}
# rows x row length: one element; a ragged Philox block; unaligned tiles; the 16-B path; around the wave and the workgroup; two
# tiles with the second partial; the longest rows; four-thousand short rows whose tiles begin inside a Philox block
SHAPES = [(1, 1), (1, 3), (3, 5), (7, 4), (2, 63), (3, 64), (2, 65), (5, 255), (3, 257), (6, 768), (2, 3072), (3, 4096), (1366, 3)]


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def data(rows, L, S, seed):
    """planted (test_ties_gpu.py) data for S = 1 .. 4 sources: many equal magnitudes, +-x pairs, zeros."""
    c, srcs = planted(rows * L, max(S, 2), seed=seed)
    return c, srcs[:S]


def job(c, srcs, L, win, lam=0.75, seed=SEED, stream=5, mode="linear", rescale=True):
    return dict(c=c, srcs=srcs, L=L, win=win, lam=lam, seed=seed, stream=stream, mode=mode, rescale=rescale)


def add(plan, j, name, tensors=None):
    base, srcs = tensors or (torch.from_numpy(j["c"]).cuda(), [torch.from_numpy(s).cuda() for s in j["srcs"]])
    return plan.add(srcs, base, None, None, j["lam"], j["seed"], j["stream"], j["mode"], rescale=j["rescale"], row_len=j["L"],
                    window=j["win"], name=name)


def run_plan(merge, jobs):
    """jobs: list of job(...).  Returns (outputs, report rows, plan)."""
    plan = merge.DellaPlan("cuda")
    outs = [add(plan, j, str(i)) for i, j in enumerate(jobs)]
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def restate(j):
    return della(j["c"], j["srcs"], j["L"], j["win"][0], j["win"][1], j["lam"], j["seed"], j["stream"], MODES[j["mode"]], j["rescale"])


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32))


def check_jobs(jobs, outs, rows):
    for i, j in enumerate(jobs):
        exp, info = restate(j)
        assert same_bits(outs[i], exp), (i, j["c"].size, j["L"], j["mode"], j["win"])
        r = rows[i]
        assert r["dst"] == str(i) and r["n"] == j["c"].size
        assert (r["keep_lo"], r["keep_hi"], r["row_len"]) == (j["win"][0], j["win"][1], j["L"])
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), (i, j["L"], j["mode"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["linear", "ties"])
@pytest.mark.parametrize("win", sorted(WINDOWS))
def test_della_row_shapes(shape, S, mode, win, merge):
    rows, L = shape
    c, srcs = data(rows, L, S, seed=rows * L + S)
    jobs = [job(c, srcs, L, WINDOWS[win], mode=mode)]
    outs, rep, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rep)


def test_della_equal_magnitudes_rank_by_index(merge):
    """A row of +-0.5 only, and a source equal to the base (every key is 0): the rank rests on the index alone."""
    rng = np.random.default_rng(3)
    jobs = []
    for L, rows in ((768, 6), (3072, 2), (5, 7), (4096, 1)):
        n = rows * L
        c = rng.standard_normal(n).astype(F)
        half = (c + np.where(rng.integers(0, 2, n) == 1, F(0.5), F(-0.5)).astype(F)).astype(F)
        c[:L] = 0.0
        half[:L] = np.where(np.arange(L) % 3 == 0, F(-0.5), F(0.5))  # exactly +-0.5 in the first row
        for mode in ("linear", "ties"):
            jobs.append(job(c, [half, c.copy(), planted(n, 2, seed=n)[1][0]], L, window(0.5, 0.4), mode=mode))
    outs, rep, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rep)
    exp, info = restate(jobs[0])
    assert np.array_equal(info["ranks"][1].reshape(-1, 768), np.broadcast_to(np.arange(768, dtype=np.uint64), (6, 768)))


def dozen():
    jobs = []
    for i, (rows, L) in enumerate(SHAPES[:12]):
        S = 1 + i % 4
        c, srcs = data(rows, L, S, seed=500 + i)
        jobs.append(job(c, srcs, L, [window(0.2, 0.1), (1, 2 ** 32), window(0.5, 0.0), window(0.7, 0.3)][i % 4], lam=[1, 0.75, 0.3][i % 3],
                        seed=[SEED, 0, 2 ** 64 - 1, 2 ** 32 + 7][i % 4], stream=[0, 5, 155, 2 ** 32 - 1][(i // 2) % 4],
                        mode=["linear", "ties"][i % 2], rescale=i % 5 != 3))
    return jobs


def test_della_a_dozen_jobs_in_one_plan(merge):
    jobs = dozen()
    outs, rep, _ = run_plan(merge, jobs)
    check_jobs(jobs, outs, rep)
    assert sum(r["conflict"] for r in rep) > 0 and sum(r["empty"] for r in rep) > 0


TINY_SHAPES = [(1, 5), (1, 1), (241, 17), (1, 3), (2, 1), (2, 768)]


def test_della_runs_of_tiles_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 jobs of one or two tiles each (shapes cycled through TINY_SHAPES; 1 .. 4 sources; both modes; window,
    lambda, seed, stream and rescale cycled), every input a 16-byte aligned view into one device buffer: every workgroup's run of
    tiles holds several jobs, so it leaves a job, flushes its counters, loads the next job's scalars and rebuilds the threshold
    table at nearly every step.  Outputs and every counter against the restatement."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    jobs = []
    for i in range(2 * 12 * n_cus + 7):
        rows, L = TINY_SHAPES[i % len(TINY_SHAPES)]
        c, srcs = data(rows, L, 1 + i % 4, seed=1000 + i)
        jobs.append(job(c, srcs, L, [window(0.2, 0.1), (1, 2 ** 32), window(0.5, 0.0), window(0.7, 0.3)][i % 4], lam=[1, 0.75, 0.3][i % 3],
                        seed=[SEED, 0, 2 ** 64 - 1, 2 ** 32 + 7][i % 4], stream=[0, 5, 155, 2 ** 32 - 1][(i // 2) % 4],
                        mode=["linear", "ties"][i % 2], rescale=i % 7 != 3))
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    plan = merge.DellaPlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base = next(views)
        outs.append(add(plan, j, str(i), (base, [next(views) for _ in j["srcs"]])))
        assert plan.jobs[-1].base == base.data_ptr()  # the view itself, not a staged copy
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, outs, plan.report())


def test_della_a_run_stays_inside_one_job_for_several_tiles(merge):
    """One job of 8 x 12 x CUs rows of 768, two sources: every workgroup's run holds several tiles of the one job.  The restatement
    of the whole tensor takes a few seconds on the host, so every row and every counter is compared -- among them the first row, the
    last and all between."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, L = 8 * 12 * n_cus, 768
    rng = np.random.default_rng(11)
    c = rng.standard_normal(rows * L).astype(F)
    srcs = [(c + rng.standard_normal(rows * L).astype(F) * F(0.1)).astype(F) for _ in range(2)]
    jobs = [job(c, srcs, L, window(0.3, 0.2), mode="ties")]
    outs, rep, _ = run_plan(merge, jobs)
    exp, info = restate(jobs[0])
    got = outs[0].cpu().numpy().view(np.uint32).reshape(rows, L)
    want = exp.view(np.uint32).reshape(rows, L)
    for r in [0, rows - 1] + list(np.linspace(0, rows - 1, 64).astype(int)):
        assert np.array_equal(got[r], want[r]), r
    assert np.array_equal(got, want)
    assert (rep[0]["kept"], rep[0]["conflict"], rep[0]["empty"]) == (info["kept"], info["conflict"], info["empty"])


def test_della_mask_is_a_function_of_coordinates_and_rank(merge):
    rows, L = 6, 768
    c, srcs = data(rows, L, 2, seed=1)
    a = job(c, srcs, L, window(0.3, 0.2), stream=5)
    others = dozen()[:7]
    outs1, rep1, _ = run_plan(merge, [a] + others)
    outs2, rep2, _ = run_plan(merge, others + [a])
    assert same_bits(outs1[0], outs2[7].cpu().numpy())  # job 0 of one plan, job 7 of another
    assert rep1[0]["kept"] == rep2[7]["kept"]
    # one row of one source changed: no other row's output changes
    changed = [s.copy() for s in srcs]
    changed[1][2 * L:3 * L] = (c[2 * L:3 * L] + np.linspace(-1, 1, L).astype(F)).astype(F)
    b = dict(a, srcs=changed)
    outs, rep, _ = run_plan(merge, [b])
    check_jobs([b], outs, rep)
    got, before = outs[0].cpu().numpy().reshape(rows, L), outs1[0].cpu().numpy().reshape(rows, L)
    assert all(np.array_equal(got[r].view(np.uint32), before[r].view(np.uint32)) == (r != 2) for r in range(rows))
    # another stream, another seed: another mask
    base = outs1[0].cpu().numpy()
    for change in (dict(stream=6), dict(seed=SEED + 1), dict(seed=SEED + 2 ** 32)):
        b = dict(a, **change)
        outs, rep, _ = run_plan(merge, [b])
        check_jobs([b], outs, rep)
        assert not np.array_equal(outs[0].cpu().numpy() != c, base != c), change


@pytest.mark.parametrize("mode", ["linear", "ties"])
@pytest.mark.parametrize("drop,rescale", [(0.5, True), (0.75, True), (0.9, False)])
def test_della_epsilon_zero_is_dare(mode, drop, rescale, merge):
    """keep_lo == keep_hi: DarePlan's bytes and counters, where DARE's float32(1 / (1 - drop)) is 2^32 / float(keep_lo)."""
    for (rows, L), S in zip(((6, 768), (3, 5), (2, 3072), (1366, 3)), (2, 3, 4, 1)):
        c, srcs = data(rows, L, S, seed=rows + L)
        kb = merge.dare_keep_below(drop)
        j = job(c, srcs, L, (kb, kb), mode=mode, rescale=rescale)
        outs, rep, _ = run_plan(merge, [j])
        dare = merge.DarePlan("cuda")
        want = dare.add([torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(c).cuda(), drop, j["lam"], j["seed"], j["stream"],
                        mode, rescale=rescale, name="0")
        dare.run()
        torch.cuda.synchronize()
        assert same_bits(outs[0], want.cpu().numpy()), (rows, L, S)
        d = dare.report()[0]
        assert (rep[0]["kept"], rep[0]["conflict"], rep[0]["empty"]) == (d["kept"], d["conflict"], d["empty"])
        assert rep[0]["keep_lo"] == rep[0]["keep_hi"] == d["keep_below"]


def test_della_full_window_is_the_task_vector_sum(merge):
    """keep_lo = keep_hi = 2^32 keeps everything with scale exactly 1.0: LINEAR is c + lam * (t_0 + t_1 + ...), restated here in
    numpy for 1 .. 4 sources.  MergePlan's task-vector job is that sum for ONE source -- the single-source rule of the drivers;
    with several sources it follows the reference's in-place accumulation, acc += r (W_m - acc), another rule -- so its bytes are
    compared where the two rules are one."""
    L = importlib.import_module("vl_merging_amd._lib")
    for (rows, rl), S in zip(((6, 768), (3, 5), (2, 3072), (1, 1), (5, 255), (1366, 3), (3, 4096)), (2, 3, 4, 1, 1, 1, 1)):
        c, srcs = data(rows, rl, S, seed=rows + rl)
        j = job(c, srcs, rl, (2 ** 32, 2 ** 32), lam=0.75)
        outs, rep, _ = run_plan(merge, [j])
        d = np.zeros(c.size, F)
        for w in srcs:
            d = d + (w - c)
        assert same_bits(outs[0], (c + F(0.75) * d).astype(F)), (rows, rl, S)
        assert rep[0]["kept"] == [rows * rl] * S and rep[0]["empty"] == 0
        if S == 1:
            plain = merge.MergePlan("cuda")
            want = plain.add(L.MERGE_TASKVEC, [torch.from_numpy(srcs[0]).cuda()], [0.75], base=torch.from_numpy(c).cuda())
            plain.run()
            torch.cuda.synchronize()
            assert same_bits(outs[0], want.cpu().numpy()), (rows, rl)


def test_della_run_three_times_same_bytes_same_counters(merge):
    jobs = dozen()[4:10]
    plan = merge.DellaPlan("cuda")
    outs = [add(plan, j, str(i)) for i, j in enumerate(jobs)]
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


def test_della_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    plan = merge.DellaPlan("cuda")
    a = torch.zeros(8, 8, device="cuda")
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, 0.5, 0.1, 1.0, SEED, 5, "linear")
    with pytest.raises(L.VlmError):
        plan.add([a], a, 0.5, 0.1, 1.0, SEED, 5, "median")
    with pytest.raises(L.VlmError):
        plan.add([torch.zeros(2, 4097, device="cuda")], torch.zeros(2, 4097, device="cuda"), 0.5, 0.1, 1.0, SEED, 5, "linear")
    with pytest.raises(L.VlmError):
        plan.add([a], a, 0.5, 0.1, 1.0, SEED, 5, "linear", row_len=3)
    with pytest.raises(L.VlmError):
        plan.add([a], a, None, None, 1.0, SEED, 5, "linear", window=(0, 5))
    with pytest.raises(ValueError):
        plan.add([a], a, 0.5, 0.6, 1.0, SEED, 5, "linear")
    assert plan.jobs == []
    out = plan.add([a + 1, a + 2], a, None, None, 0.5, SEED, 5, "linear", window=(2 ** 32, 2 ** 32))
    assert plan.jobs[0].row_len == 8
    lib = L.get_lib()
    ws = torch.empty(lib.vlm_della_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    for field, value in (("n_src", 2), ("dst", a.data_ptr()), ("row_len", 0), ("row_len", 7), ("keep_lo", 0), ("mode", 2)):
        bad = L.DellaJob.from_buffer_copy(bytes(plan.jobs[0]))
        setattr(bad, field, value)
        rc = lib.vlm_della_plan_upload((L.DellaJob * 1)(bad), 1, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert rc == {"n_src": 0, "row_len": -4 if value == 0 else -1}.get(field, -1), (field, value)
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().reshape(-1).tolist() == [1.5] * 64  # 0 + 0.5 * (1 + 2)


def restate_state(sd, central, cfg, density, epsilon, lam, seed, mode, rescale=True, layers=range(12)):
    """dst -> (expected tensor, info | None) for the block tensors of `layers`; single-source layers: the oracle's task-vector job.
    The stream (13 * layer + the position of the name in the layer) and the row (the last dimension of a matrix, a vector as a
    whole) are restated here."""
    exp = {}
    lo, hi = window(density, epsilon)
    for i in layers:
        mods = mo._modalities(cfg, i)
        for slot, (src, dst) in enumerate(mo._names(i)):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None)
            else:
                shape = central[dst].shape
                out, info = della(central[dst], srcs, shape[-1] if len(shape) >= 2 else central[dst].size, lo, hi, lam, seed,
                                  13 * i + slot, MODES[mode], rescale)
                exp[dst] = (out.reshape(shape), info)
    return exp


def check_report(rows, exp):
    by_dst = {r["dst"]: r for r in rows}
    assert sorted(by_dst) == sorted(k for k, (_, info) in exp.items() if info is not None)
    for dst, r in by_dst.items():
        info = exp[dst][1]
        assert (r["n"], r["keep_lo"], r["keep_hi"], r["row_len"]) == (exp[dst][0].size, info["keep_lo"], info["keep_hi"], info["row_len"]), dst
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), dst


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("mode", ["linear", "ties"])
def test_della_merge_tiny_matches_restatement(case, mode, merge):
    lam = 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {k: v.clone() for k, v in central.items()}
    rows, plans = [], []
    res = merge.della_merge(sd, cfg, central_weight={"state_dict": central}, density=0.4, epsilon=0.3, seed=SEED, mode=mode,
                            report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, 0.4, 0.3, lam, SEED, mode)
    n_block = 0
    for k, v in res.items():
        if is_block(k):
            assert same_bits(v, exp[k][0]), k
            assert v.shape == central[k].shape and v.data_ptr() != central[k].data_ptr()
            if exp[k][1] is None:  # one source: the task-vector job with ratio 1, undropped, as sum_task_vectors issues it
                assert same_bits(v, ref[k].cpu().numpy()), k
            n_block += 1
        else:
            assert v is sd[k]  # pass-through by identity
    assert n_block == 12 * 13
    assert all(torch.equal(central[k], central_before[k]) for k in central)
    check_report(rows, exp)
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.DellaPlan)
    if case == "used_vqa":
        assert isinstance(plans[1], merge.MergePlan)
    assert [r["dst"] for r in rows] == [k for k in res if is_block(k) and exp[k][1] is not None]  # the walk's order


@pytest.fixture(scope="module")
def base_state():
    sd_np, central_np = base_size_state()
    return sd_np, central_np, to_dev(sd_np), to_dev(central_np)


@pytest.mark.parametrize("mode", ["linear", "ties"])
def test_della_base_size(mode, merge, base_state):
    """Base size: layers 0 (two sources) and 11 (three) against the restatement tensor by tensor; the whole checkpoint twice with
    the same bytes; every tensor's kept share inside the window."""
    sd_np, central_np, sd, central = base_state
    cfg = merge_cfg(sum_lambda=0.75)
    density, epsilon = 0.2, 0.1
    rows, plans = [], []
    res = merge.della_merge(sd, cfg, central_weight=central, density=density, epsilon=epsilon, seed=SEED, mode=mode, plan_out=plans,
                            report_out=rows)
    torch.cuda.synchronize()
    exp = restate_state(sd_np, central_np, cfg, density, epsilon, 0.75, SEED, mode, layers=(0, 11))
    by_dst = {r["dst"]: r for r in rows}
    for k, (want, info) in exp.items():
        assert same_bits(res[k], want), k
        r = by_dst[k]
        assert (r["kept"], r["conflict"], r["empty"]) == (info["kept"], info["conflict"], info["empty"]), k
    assert len(rows) == 12 * 13
    again = merge.della_merge(sd, cfg, central_weight=central, density=density, epsilon=epsilon, seed=SEED, mode=mode)
    torch.cuda.synchronize()
    for k, v in res.items():
        if is_block(k):
            assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), k
    for r in rows:
        for kept in r["kept"]:
            assert density - epsilon <= kept / r["n"] <= density + epsilon, r
    plan = plans[0]
    assert plan.bytes_written == 4 * sum(v.numel() for k, v in res.items() if is_block(k))
    assert plan.bytes_read == 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs)  # one pass: DARE's traffic


def test_merge_ckpt_della_as_a_child_process(merge, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {k: torch.from_numpy(v) for k, v in tiny_state("all_moe").items()}
    central = {k: torch.from_numpy(v) for k, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep = tmp_path / "della.ckpt", tmp_path / "della.json"
    cmd = [sys.executable, TOOL, "--method", "della", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--density", "0.4", "--epsilon", "0.3", "--seed", str(SEED), "--della-mode", "ties",
           "--no-rescale", "--lambda", "0.75", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    rows = []
    want = merge.della_merge(to_dev(sd), merge_cfg(sum_lambda=0.75), central_weight=to_dev(central), density=0.4, epsilon=0.3, seed=SEED,
                             mode="ties", rescale=False, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k].device.type == "cpu" and got[k].numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    assert (rep["method"], rep["density"], rep["epsilon"], rep["seed"], rep["della_mode"]) == ("della", 0.4, 0.3, SEED, "ties")
    assert rep["rescale"] is False and rep["sum_lambda"] == 0.75 and rep["drop"] is None
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows


def test_model_method_is_the_same_merge(merge, pkg):
    """ViLTransformerSS.della_merge forwards to merge.della_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    want = merge.della_merge(sd, Stub.hparams.config, central_weight=central, density=0.4, epsilon=0.3, seed=SEED, mode="ties",
                             rescale=False)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.della_merge(Stub(), sd, density=0.4, epsilon=0.3, seed=SEED, mode="ties", rescale=False)
    torch.cuda.synchronize()
    assert all(same_bits(got[k], want[k].cpu().numpy()) for k in want if is_block(k))
    assert vm.ViLTransformerSS.della_merge.__defaults__ == (0.2, 0.1, "linear", None, 0, True)  # merge.della_merge's defaults
