"""Consensus merge with TALL masks on the GPU (csrc/tall.hip through the C ABI) against the numpy restatement of the rule
(tall_restatement.py): every comparison is over ALL elements and bit for bit -- outputs, every mask word with its padding bits, every
counter.  The reference has no such merge; only the single-source layers of the vqa case can be (and are) tied to the task-vector
merge the reference's goldens pin."""
import importlib
import inspect
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
from tall_restatement import consensus, pack, restore

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, dev_words, one_buffer, poison, tiny_jobs, words_of  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
RESTORE_TOOL = os.path.join(ROOT, "vl-merging_amd", "tall_restore.py")
F = np.float32


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def cjob(c, srcs, tall_lambda, k, lam=0.75, masks=True):
    return dict(op="consensus", c=c, srcs=srcs, tall_lambda=tall_lambda, k=k, lam=lam, masks=masks)


def rjob(u, c, words):
    return dict(op="restore", u=u, c=c, words=words)


def add_job(plan, j, name, base=None, srcs=None, out=None):
    """One job(...) into `plan`; `base` / `srcs`: device tensors to use instead of fresh copies."""
    base = torch.from_numpy(j["c"]).cuda() if base is None else base
    if j["op"] == "restore":
        u = torch.from_numpy(j["u"]).cuda() if srcs is None else srcs[0]
        return plan.add_restore(u, base, dev_words(j["words"]), out=out, name=name)
    srcs = [torch.from_numpy(s).cuda() for s in j["srcs"]] if srcs is None else srcs
    return plan.add(srcs, base, j["tall_lambda"], j["k"], lam=j["lam"], masks=j["masks"], out=out, name=name)


def run_plan(merge, jobs):
    """jobs: list of cjob(...) / rjob(...).  Returns (outputs, report rows, plan)."""
    plan = merge.TallPlan("cuda")
    outs = [add_job(plan, j, str(i)) for i, j in enumerate(jobs)]
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def restate(j):
    if j["op"] == "restore":
        return restore(j["u"], j["c"], j["words"])
    return consensus(j["c"], j["srcs"], j["tall_lambda"], j["k"], j["lam"])


def check_jobs(jobs, outs, rows, plan):
    for i, j in enumerate(jobs):
        exp, info = restate(j)
        tag = (i, j["op"], exp.size)
        assert outs[i].cpu().numpy().tobytes() == exp.tobytes(), tag
        r = rows[i]
        assert (r["dst"], r["n"], r["op"]) == (str(i), exp.size, j["op"]), tag
        assert (r["kept"], r["selected"], r["empty"]) == (info["kept"], info["selected"], info["empty"]), tag
        if j["op"] == "restore":
            continue
        assert (r["k"], r["tall_lambda"]) == (j["k"], float(F(j["tall_lambda"]))), tag
        if not j["masks"]:
            assert plan.masks[i] is None
            continue
        assert len(plan.masks[i]) == len(j["srcs"])
        for m, t in enumerate(plan.masks[i]):
            got = words_of(t)
            assert t.dtype == torch.int32 and got.size == (exp.size + 31) // 32
            assert got.tobytes() == info["words"][m].tobytes(), tag + (m,)        # every word, padding bits included
            assert int(np.unpackbits(got.view(np.uint8)).sum()) == r["kept"][m]   # popcount(mask m) == kept[m]


SIZES = [1, 3, 4, 5, 23, 31, 32, 33, 63, 1023, 4096, 4097, 4110, 8191, 12289, 1 << 20]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_tall_ragged_sizes(n, S, which, merge):
    """n = 23 and n = 4110: the last word mixes float4 lanes and tail elements; n = 1 and n = 3: tail only; n = 4097: the tail's
    word lies behind the chunk's last float4 (the fifth slot)."""
    tall_lambda, k = [(0.4, 2), (0.5, 1), (1.0, S)][which]
    c, srcs = planted(n, S, seed=n + S)
    jobs = [cjob(c, srcs, tall_lambda, k)]
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows, plan)


def test_planted_inputs_exercise_every_vote_level_and_the_tie():
    """What the ragged-size cases rely on (numpy only): on planted(12289, S, 7) every vote level 1 .. S occurs for every tall_lambda
    used, and exact |x| == tall_lambda |r| ties are plentiful, so >= against > is tested."""
    for S in (2, 3, 4):
        c, srcs = planted(12289, S, 7)
        for tl in (0.2, 0.4, 0.5, 1.0):
            _, info = consensus(c, srcs, tl, 1, 1)
            assert set(range(1, S + 1)) <= set(np.unique(info["votes"]).tolist()), (S, tl)
            ties = sum(int((np.abs(w - c) == F(tl) * np.abs(info["d"] - (w - c))).sum()) for w in srcs)
            assert ties >= 200, (S, tl, ties)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_tall_k_zero_is_plain_task_arithmetic(S, merge):
    n = 8191
    rng = np.random.default_rng(S)
    c = rng.standard_normal(n).astype(F)
    srcs = [(c + rng.standard_normal(n).astype(F) * F(0.1)).astype(F) for _ in range(S)]
    jobs = [cjob(c, srcs, 0.4, 0, masks=False), cjob(c, srcs, 0.4, 0, masks=True)]
    outs, rows, plan = run_plan(merge, jobs)
    d = np.zeros(n, F)
    for w in srcs:
        d = d + (w - c)
    want = (c + F(0.75) * d).astype(F).tobytes()
    assert outs[0].cpu().numpy().tobytes() == want and outs[1].cpu().numpy().tobytes() == want
    check_jobs(jobs, outs, rows, plan)
    assert rows[0]["selected"] == n and rows[0]["kept"] == rows[1]["kept"]
    if S == 1:
        assert rows[0]["kept"] == [n]  # one source keeps everything


def mixed_jobs():
    """Mixed sizes, S = 1 .. 4, both ops, masks on and off, tall_lambda / k / lam different per job."""
    rng = np.random.default_rng(8)
    jobs = []
    sizes = [12289, 1, 4097, 3, 1 << 18, 5, 8191, 4096, 70000, 1023, 23, 8193, 4110]
    for i, n in enumerate(sizes):
        S = 1 + i % 4
        c, srcs = planted(n, max(S, 2), seed=300 + i)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(F) * F(0.3)).astype(F))
        if i % 3 == 2:  # a restore job: random words, garbage in the padding bits too
            words = rng.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype("<u4")
            jobs.append(rjob(srcs[0], c, words))
        else:
            jobs.append(cjob(c, srcs[:S], [0.4, 0.5, 1.0, 0.2, 0.0][i % 5], min(S, [2, 3, 1, 0][(i // 2) % 4]),
                             lam=[1, 0.75, 0.3][i % 3], masks=i % 2 == 0))
    return jobs


def test_tall_a_dozen_jobs_in_one_plan(merge):
    jobs = mixed_jobs()
    assert {j["op"] for j in jobs} == {"consensus", "restore"} and {j.get("masks") for j in jobs} == {True, False, None}
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows, plan)
    assert sum(r["empty"] for r in rows) > 0 and sum(r["selected"] for r in rows) > 0


def test_tall_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one-chunk jobs (lengths cycled through 5, 1, 4097, 3, 2, 4099; 1 .. 4 sources), every input a 16-byte
    aligned view into one device buffer: each of the 12 workgroups per CU owns three chunks, every one of another job -- so a run
    leaves a job, flushes its counters and loads the next job's scalars at every step.  Masks on for two jobs of three.  Outputs,
    words and every counter against the restatement."""
    jobs = [cjob(c, srcs, [0.4, 0.5, 1.0, 0.2][i % 4], min(i % 3, len(srcs)), lam=[1, 0.75, 0.3][i % 3], masks=i % 3 != 1)
            for i, (c, srcs) in enumerate(tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted))]
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    plan = merge.TallPlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base = next(views)
        outs.append(add_job(plan, j, str(i), base=base, srcs=[next(views) for _ in j["srcs"]]))
        assert plan.jobs[-1].base == base.data_ptr()  # the view itself, not a staged copy
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, outs, plan.report(), plan)


def test_tall_dst_may_be_base_or_a_source(merge):
    for n in (12289, 23, 3):
        c, srcs = planted(n, 3, seed=n)
        j = cjob(c, srcs, 0.4, 2)
        (want,), rows, plan0 = run_plan(merge, [j])
        want = want.cpu().numpy().tobytes()
        for which in ("base", 1):
            dev = [torch.from_numpy(s).cuda() for s in srcs]
            b = torch.from_numpy(c).cuda()
            out = b if which == "base" else dev[which]
            plan = merge.TallPlan("cuda")
            got = add_job(plan, j, "0", base=b, srcs=dev, out=out)
            assert got.data_ptr() == out.data_ptr()
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want, (n, which)
            assert plan.report() == rows
            assert [words_of(t).tobytes() for t in plan.masks[0]] == [words_of(t).tobytes() for t in plan0.masks[0]]
            for k, s in enumerate(dev):  # the other inputs are untouched
                if which != k:
                    assert s.cpu().numpy().tobytes() == srcs[k].tobytes()
        # restore in place: dst is the unified tensor, then the central tensor
        u, info = consensus(c, srcs, 0.4, 0, 1)
        exp, _ = restore(u, c, info["words"][1])
        for which in ("u", "base"):
            du, db = torch.from_numpy(u).cuda(), torch.from_numpy(c).cuda()
            plan = merge.TallPlan("cuda")
            got = plan.add_restore(du, db, dev_words(info["words"][1]), out=du if which == "u" else db)
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == exp.tobytes(), (n, which)


def test_tall_run_three_times_same_bytes_same_words_same_counters(merge):
    jobs = [cjob(*planted(70001, 3, seed=1), 0.4, 2), cjob(*planted(4097, 2, seed=2), 0.5, 1), cjob(*planted(23, 2, seed=3), 1.0, 2),
            rjob(planted(4110, 2, seed=4)[1][0], planted(4110, 2, seed=4)[0], pack(np.arange(4110) % 3 == 0))]
    plan = merge.TallPlan("cuda")
    outs = [add_job(plan, j, str(i)) for i, j in enumerate(jobs)]
    got, reports = [], []
    for _ in range(3):
        poison(plan, outs)
        plan.run()
        torch.cuda.synchronize()
        got.append([o.cpu().numpy().tobytes() for o in outs] + [words_of(t).tobytes() for ms in plan.masks[:3] for t in ms])
        reports.append(plan.report())
    assert got[0] == got[1] == got[2]
    assert reports[0] == reports[1] == reports[2]
    check_jobs(jobs, outs, reports[0], plan)


# ---------------------------------------------------------------------------------------------------------------- restore
@pytest.mark.parametrize("n", [1, 3, 23, 32, 4097, 4110, 12289])
def test_tall_restore_is_the_papers_reconstruction(n, merge):
    """restore(u = consensus(k = 0, lam = 1), c, mask_m) == float32(c + where(keep_m, d, 0)); all ones gives u, all zeros gives c."""
    S = 3
    c, srcs = planted(n, S, seed=40 + n)
    j0 = cjob(c, srcs, 0.4, 0, lam=1)
    (u_dev,), _, plan0 = run_plan(merge, [j0])
    u, info = consensus(c, srcs, 0.4, 0, 1)
    assert u_dev.cpu().numpy().tobytes() == u.tobytes()
    ones, zeros = np.full((n + 31) // 32, 0xFFFFFFFF, "<u4"), np.zeros((n + 31) // 32, "<u4")
    plan = merge.TallPlan("cuda")
    cd = torch.from_numpy(c).cuda()
    outs = [plan.add_restore(u_dev, cd, plan0.masks[0][m], name=str(m)) for m in range(S)]   # the device's own masks, as they are
    assert [plan.jobs[m].mask[0] for m in range(S)] == [t.data_ptr() for t in plan0.masks[0]]
    outs += [plan.add_restore(u_dev, cd, dev_words(w), name=nm) for w, nm in ((ones, "ones"), (zeros, "zeros"))]
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    rows = plan.report()
    for m in range(S):
        want = (c + np.where(info["keep"][m], info["d"], F(0.0)).astype(F)).astype(F)
        assert outs[m].cpu().numpy().tobytes() == want.tobytes() == restore(u, c, info["words"][m])[0].tobytes(), (n, m)
        assert (rows[m]["op"], rows[m]["kept"], rows[m]["selected"], rows[m]["empty"]) == ("restore", [info["kept"][m]], 0, 0)
    assert outs[S].cpu().numpy().tobytes() == u.tobytes() and rows[S]["kept"] == [n]
    assert outs[S + 1].cpu().numpy().tobytes() == c.tobytes() and rows[S + 1]["kept"] == [0]


@pytest.mark.parametrize("n", [23, 100, 4097, 4110, 8192 + 3])
def test_tall_restore_reads_no_word_past_the_mask(n, merge):
    """The mask is the leading view of a buffer whose following words -- and the padding bits of its own last word -- are all ones:
    what lies behind ceil(n / 32) words, or behind bit n, decides nothing."""
    c, srcs = planted(n, 2, seed=n)
    keep = np.arange(n) % 5 == 1
    words = pack(keep)
    nw = words.size
    buf = torch.full((nw + 64,), -1, dtype=torch.int32, device="cuda")
    dirty = words.copy()
    if n % 32:
        dirty[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    buf[:nw] = dev_words(dirty)
    view = buf[:nw]
    plan = merge.TallPlan("cuda")
    out = plan.add_restore(torch.from_numpy(srcs[0]).cuda(), torch.from_numpy(c).cuda(), view)
    assert plan.jobs[0].mask[0] == view.data_ptr() == buf.data_ptr()  # the view itself
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == np.where(keep, srcs[0], c).astype(F).tobytes()
    assert plan.report()[0]["kept"] == [int(keep.sum())]
    assert bool((buf[nw:] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- upload checks
def test_tall_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.TallPlan("cuda")
    a = torch.zeros(64, device="cuda")
    with pytest.raises(L.VlmError):
        plan.add([a] * 5, a, 0.4, 2)
    with pytest.raises(L.VlmError):
        plan.add([a, torch.zeros(32, device="cuda")], a, 0.4, 2)
    with pytest.raises(L.VlmError):
        plan.add([a.double()], a, 0.4, 1)
    with pytest.raises(ValueError):
        plan.add([a, a], a, 0.4, 3)
    with pytest.raises(ValueError):
        plan.add([a, a], a, float("nan"), 2)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), None):
        with pytest.raises(L.VlmError):
            plan.add_restore(a, a, bad)
    assert plan.jobs == [] and plan.masks == []
    out = plan.add([a + 1, a + 2], a, 0.0, 2, lam=0.5, masks=True)
    ws = torch.empty(lib.vlm_tall_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")

    def upload(j, nbytes=None):
        return lib.vlm_tall_plan_upload((L.TallJob * 1)(j), 1, L.ptr(ws), ws.numel() if nbytes is None else nbytes, L.stream_ptr())

    assert upload(plan.jobs[0], 512) == -3  # VLM_ERR_WORKSPACE
    good = plan.jobs[0]
    m0, m1 = good.mask[0], good.mask[1]
    spare = torch.zeros(64, dtype=torch.int32, device="cuda")
    cases = [("control", {}, 0), ("mask is dst", dict(mask_0=good.dst), -1), ("mask is a source", dict(mask_1=good.src[0]), -1),
             ("mask inside a source", dict(mask_1=good.src[1] + 128), -1), ("mask is the other mask", dict(mask_1=m0), -1),
             ("misaligned mask", dict(mask_1=spare.data_ptr() + 4), -1), ("spare mask", dict(mask_1=spare.data_ptr()), 0),
             ("k = S + 1", dict(k=3), -1), ("NaN lambda", dict(tall_lambda=float("nan")), -1),
             ("partial mask set", dict(mask_1=0), -1), ("restore with two sources", dict(op=L.TALL_RESTORE), -1),
             ("restore", dict(op=L.TALL_RESTORE, n_src=1, k=0), 0), ("no masks", dict(mask_0=0, mask_1=0), 0)]
    for name, fields, want in cases:
        j = L.TallJob.from_buffer_copy(bytes(good))
        for f, v in fields.items():
            if f.startswith("mask_"):
                j.mask[int(f[5:])] = v
            else:
                setattr(j, f, v)
        assert upload(j) == want, name
    assert (good.mask[0], good.mask[1]) == (m0, m1)
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [1.5] * 64  # 0 + 0.5 * (1 + 2): tall_lambda = 0 keeps everything
    assert [words_of(t).tolist() for t in plan.masks[0]] == [[0xFFFFFFFF] * 2] * 2


# ---------------------------------------------------------------------------------------------------------------- state dicts
def restate_state(sd, central, cfg, tall_lambda, k, lam, layers=range(12)):
    """dst -> (expected tensor, info | None, source keys) for the block tensors of `layers`; single-source layers: the oracle's
    task-vector job.  k is clamped per layer: min(k, S)."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None, [src(mods[0])])
            else:
                out, info = consensus(central[dst], srcs, tall_lambda, min(k, len(mods)), lam)
                exp[dst] = (out.reshape(central[dst].shape), info, [src(m) for m in mods])
    return exp


def check_report(rows, exp, tall_lambda, k):
    by_dst = {r["dst"]: r for r in rows}
    assert sorted(by_dst) == sorted(d for d, (_, info, _) in exp.items() if info is not None)
    for dst, r in by_dst.items():
        want, info, keys = exp[dst]
        assert (r["n"], r["op"], r["k"], r["tall_lambda"]) == (want.size, "consensus", min(k, len(keys)), float(F(tall_lambda))), dst
        assert (r["kept"], r["selected"], r["empty"]) == (info["kept"], info["selected"], info["empty"]), dst


def check_masks(masks, exp):
    want = {key: info["words"][m] for _, info, keys in exp.values() if info is not None for m, key in enumerate(keys)}
    assert sorted(masks) == sorted(want)
    for key, t in masks.items():
        assert t.dtype == torch.int32 and t.is_cuda and words_of(t).tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("tall_lambda,k", [(0.4, 2), (0.5, 1), (0.2, 3)])
def test_consensus_merge_tiny_matches_restatement(case, tall_lambda, k, merge):
    lam = 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {key: v.clone() for key, v in central.items()}
    rows, plans, masks = [], [], {}
    res = merge.consensus_merge(sd, cfg, central_weight={"state_dict": central}, tall_lambda=tall_lambda, k=k, masks_out=masks,
                                report_out=rows, plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, tall_lambda, k, lam)
    n_block = 0
    for key, v in res.items():
        if is_block(key):
            assert v.cpu().numpy().tobytes() == exp[key][0].tobytes(), key
            assert v.shape == central[key].shape and v.data_ptr() != central[key].data_ptr()
            if exp[key][1] is None:  # one source: the task-vector job with ratio 1, as sum_task_vectors issues it
                assert v.cpu().numpy().tobytes() == ref[key].cpu().numpy().tobytes(), key
            n_block += 1
        else:
            assert v is sd[key]
    assert n_block == 12 * 13
    assert all(torch.equal(central[key], central_before[key]) for key in central)  # the central tensors are inputs only
    check_report(rows, exp, tall_lambda, k)
    check_masks(masks, exp)
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.TallPlan)
    if case == "used_vqa":
        assert isinstance(plans[1], merge.MergePlan)
    # without masks_out: the same tensors, no mask allocated
    plans2 = []
    res2 = merge.consensus_merge(sd, cfg, central_weight=central, tall_lambda=tall_lambda, k=k, lam=lam, plan_out=plans2)
    torch.cuda.synchronize()
    assert all(res2[key].cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes() for key in res if is_block(key))
    assert all(ms is None for ms in plans2[0].masks)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tall_restore_round_trip(case, merge):
    """tall_restore(consensus_merge(k = 0, lam = 1), masks) returns exactly the source keys consumed, each the restatement's select
    of the unified and the central tensor; single-source layers get the unified tensor itself; the rest passes through."""
    L = importlib.import_module("vl_merging_amd._lib")
    cfg = merge_cfg(sum_lambda=0.3, **CASES[case])   # lam = 1 is passed explicitly and wins
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    masks, plans = {}, []
    uni = merge.consensus_merge(sd, cfg, central_weight=central, tall_lambda=0.4, k=0, lam=1.0, masks_out=masks)
    back = merge.tall_restore(uni, masks, cfg, central_weight={"state_dict": central}, plan_out=plans)
    torch.cuda.synchronize()
    exp = restate_state(sd_np, central_np, cfg, 0.4, 0, 1.0)
    consumed = [key for _, _, keys in exp.values() for key in keys]
    assert sorted(key for key in back if is_block(key)) == sorted(consumed)
    for dst, (u, info, keys) in exp.items():
        for m, key in enumerate(keys):
            if info is None:
                assert back[key] is uni[dst]
            else:
                want = restore(u, central_np[dst], info["words"][m])[0]
                assert want.tobytes() == (central_np[dst].reshape(-1) + np.where(info["keep"][m], info["d"], F(0)).astype(F)).astype(F).tobytes()
                assert back[key].cpu().numpy().tobytes() == want.tobytes() and back[key].shape == sd[key].shape, key
    for key, v in back.items():
        if not is_block(key):
            assert v is uni[key] and v is sd[key]
    assert len(plans) == 1 and isinstance(plans[0], merge.TallPlan) and len(plans[0].jobs) == len(masks)
    assert all(r["op"] == "restore" for r in plans[0].report())
    # masks from the CPU (as a masks file holds them) give the same tensors; a mask that does not fit is refused; so is a stray key
    back2 = merge.tall_restore(uni, {key: t.cpu() for key, t in masks.items()}, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert all(back2[key].cpu().numpy().tobytes() == back[key].cpu().numpy().tobytes() for key in back if is_block(key))
    key0 = sorted(masks)[0]
    with pytest.raises(L.VlmError):
        merge.tall_restore(uni, {key0: masks[key0][:-1]}, cfg, central_weight=central)
    with pytest.raises(KeyError):
        merge.tall_restore(uni, {"transformer.blocks.0.attn.zz.qkv.weight": masks[key0]}, cfg, central_weight=central)


def test_tall_base_size(merge):
    """Base size (the inputs of test_ties_base_size), masks on: layers 0 (two sources) and 11 (three) against the restatement bit for
    bit, words included; every other output finite; the plan's byte counts; and run() returns while its launches are still queued."""
    L = importlib.import_module("vl_merging_amd._lib")
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    plans, rows, masks = [], [], {}
    res = merge.consensus_merge(sd, cfg, central_weight=central, tall_lambda=0.4, k=2, masks_out=masks, plan_out=plans, report_out=rows)
    torch.cuda.synchronize()
    plan = plans[0]
    n_out = sum(v.numel() for key, v in res.items() if is_block(key))
    mask_bytes = sum(4 * t.numel() for t in masks.values())
    assert mask_bytes == sum(4 * ((int(j.n_elem) + 31) // 32) * j.n_src for j in plan.jobs)
    assert plan.bytes_written == 4 * n_out + mask_bytes and 4 * n_out == 340180992
    assert plan.bytes_read == 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs) == 737058816 + 340180992
    exp = restate_state(sd_np, central_np, cfg, 0.4, 2, 0.75, layers=(0, 11))
    by_dst = {r["dst"]: r for r in rows}
    for dst, (want, info, keys) in exp.items():
        assert res[dst].cpu().numpy().tobytes() == want.tobytes(), dst
        r = by_dst[dst]
        assert (r["kept"], r["selected"], r["empty"]) == (info["kept"], info["selected"], info["empty"]), dst
        for m, key in enumerate(keys):
            assert words_of(masks[key]).tobytes() == info["words"][m].tobytes(), key
    assert len(rows) == 12 * 13 and len(masks) == 10 * 13 * 2 + 2 * 13 * 3
    for key, v in res.items():
        if is_block(key):
            assert bool(torch.isfinite(v).all()), key
    # no host synchronisation between upload and the end of run(): the ENQUEUE is timed behind a 0.2 s spin kernel on the same
    # stream, as test_dare_base_size does.  The spin's own length is checked, so the bound cannot pass vacuously.
    import time
    first = {dst: res[dst].clone() for dst in exp}
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
    print("consensus enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "TallPlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert all(torch.equal(res[dst], first[dst]) for dst in exp)
    assert plan.report() == rows


# ---------------------------------------------------------------------------------------------------------------- command lines
def test_merge_ckpt_consensus_and_tall_restore_as_child_processes(merge, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {key: torch.from_numpy(v) for key, v in tiny_state("all_moe").items()}
    central = {key: torch.from_numpy(v) for key, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep, mfile = tmp_path / "uni.ckpt", tmp_path / "uni.json", tmp_path / "masks.pt"
    cmd = [sys.executable, TOOL, "--method", "consensus", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--tall-lambda", "0.5", "--consensus-k", "0", "--masks-out", str(mfile),
           "--lambda", "1", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    saved = ckpt.load_file(str(mfile))
    rows, masks = [], {}
    cfg = merge_cfg(sum_lambda=1)
    want = merge.consensus_merge(to_dev(sd), cfg, central_weight=to_dev(central), tall_lambda=0.5, k=0, masks_out=masks, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for key in want:
        assert got[key].device.type == "cpu" and got[key].numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    assert (rep["method"], rep["tall_lambda"], rep["consensus_k"]) == ("consensus", 0.5, 0)
    assert rep["sum_lambda"] == 1 and "merge_ratio" in rep and rep["density"] is None and rep["drop"] is None  # the existing keys stay
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows
    assert (saved["format"], saved["tall_lambda"], saved["k"]) == ("tall-masks-1", 0.5, 0)
    assert sorted(saved["masks"]) == sorted(masks) and len(masks) == 10 * 13 * 2 + 2 * 13 * 3
    for key, t in saved["masks"].items():
        assert t.dtype == torch.int32 and t.device.type == "cpu" and t.numpy().tobytes() == masks[key].cpu().numpy().tobytes(), key
    # and back: ufo + masks -> all_moe
    back_file = tmp_path / "back.ckpt"
    cmd = [sys.executable, RESTORE_TOOL, "--unified", str(out), "--central", str(tmp_path / "ufo.ckpt"), "--masks", str(mfile),
           "--out", str(back_file), "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    back = ckpt.load_ckpt(str(back_file))
    want_back = merge.tall_restore(want, masks, cfg, central_weight=to_dev(central))
    torch.cuda.synchronize()
    assert list(back.keys()) == list(want_back.keys()) and sorted(key for key in back if is_block(key)) == sorted(masks)
    for key in want_back:
        assert back[key].device.type == "cpu" and back[key].numpy().tobytes() == want_back[key].cpu().numpy().tobytes(), key


def test_model_method_is_the_same_merge(merge, pkg):
    """ViLTransformerSS.consensus_merge forwards to merge.consensus_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    m_want, m_got = {}, {}
    want = merge.consensus_merge(sd, Stub.hparams.config, central_weight=central, tall_lambda=0.5, k=1, masks_out=m_want)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.consensus_merge(Stub(), sd, tall_lambda=0.5, k=1, masks_out=m_got)
    torch.cuda.synchronize()
    assert all(got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes() for key in want if is_block(key))
    assert sorted(m_got) == sorted(m_want) and all(torch.equal(m_got[key], m_want[key]) for key in m_want)
    ours = inspect.signature(merge.consensus_merge).parameters
    theirs = inspect.signature(vm.ViLTransformerSS.consensus_merge).parameters
    assert vm.ViLTransformerSS.consensus_merge.__defaults__ == (0.4, 2, None, None)
    assert all(theirs[p].default == ours[p].default for p in ("tall_lambda", "k", "lam", "masks_out"))
