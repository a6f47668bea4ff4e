"""EMR-Merging on the GPU (csrc/emr.hip through the C ABI) against the numpy restatement of the rule (emr_restatement.py): every
comparison is over ALL elements and bit for bit -- outputs, every mask word with its padding bits, every count, and the sums and
rescalers by their bit patterns.  The reference has no such merge; only the single-source layers of the vqa case can be (and are)
tied to the task-vector merge the reference's goldens pin."""
import importlib
import inspect
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, is_block, planted, to_dev
from emr_restatement import emr, pack, restore

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import dev_words, one_buffer, poison, tiny_jobs, words_of  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
RESTORE_TOOL = os.path.join(ROOT, "vl-merging_amd", "tall_restore.py")
F = np.float32


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def inputs(n, S, seed):
    """planted(n, S, seed); planted needs two sources, so S = 1 is the first source of planted(n, 2, seed)."""
    c, srcs = planted(n, max(S, 2), seed)
    return c, srcs[:S]


def d64(v):
    return struct.pack("<d", v)


def f32(v):
    return struct.pack("<f", v)


def mjob(c, srcs, lam=0.75, masks=True):
    return dict(op="emr", c=c, srcs=srcs, lam=lam, masks=masks)


def rjob(uni, c, words, rescale):
    return dict(op="restore", u=uni, c=c, words=words, rescale=rescale)


def add_job(plan, j, name, base=None, srcs=None, out=None):
    """One job(...) into `plan`; `base` / `srcs`: device tensors to use instead of fresh copies."""
    base = torch.from_numpy(j["c"]).cuda() if base is None else base
    if j["op"] == "restore":
        u = torch.from_numpy(j["u"]).cuda() if srcs is None else srcs[0]
        return plan.add_restore(u, base, dev_words(j["words"]), j["rescale"], out=out, name=name)
    srcs = [torch.from_numpy(s).cuda() for s in j["srcs"]] if srcs is None else srcs
    return plan.add(srcs, base, lam=j["lam"], masks=j["masks"], out=out, name=name)


def run_plan(merge, jobs):
    """jobs: list of mjob(...) / rjob(...).  Returns (outputs, report rows, plan)."""
    plan = merge.EmrPlan("cuda")
    outs = [add_job(plan, j, str(i)) for i, j in enumerate(jobs)]
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    return outs, plan.report(), plan


def restate(j):
    if j["op"] == "restore":
        return restore(j["u"], j["c"], j["words"], j["rescale"])
    return emr(j["c"], j["srcs"], j["lam"])


def check_result(r, raw, info, S, tag):
    """A report row and the raw vlm_emr_result_t of a merge job against the restatement: counts exactly, doubles and floats by bits;
    the slots the job does not have are zero."""
    assert (r["kept"], r["zero"], r["conflict"]) == (info["kept"], info["zero"], info["conflict"]), tag
    assert [d64(v) for v in r["abs_sum"]] == [d64(v) for v in info["abs_sum"]], tag
    assert [d64(v) for v in r["uni_sum"]] == [d64(v) for v in info["uni_sum"]], tag
    assert [f32(v) for v in r["rescale"]] == [v.tobytes() for v in info["rescale"]], tag
    assert [F(v) == v for v in r["rescale"]] == [True] * S          # python floats that hold fp32 values exactly
    for m in range(S, 4):
        assert (raw.abs_sum[m], raw.uni_sum[m], raw.kept[m], raw.rescale[m]) == (0.0, 0.0, 0, 0.0), tag


def check_jobs(jobs, outs, rows, plan):
    raws = plan.results()
    for i, j in enumerate(jobs):
        exp, info = restate(j)
        tag = (i, j["op"], exp.size)
        assert outs[i].cpu().numpy().tobytes() == exp.tobytes(), tag
        r = rows[i]
        assert (r["dst"], r["n"], r["op"]) == (str(i), exp.size, j["op"]), tag
        if j["op"] == "restore":
            assert (r["kept"], r["zero"], r["conflict"], r["abs_sum"], r["uni_sum"], r["rescale"]) == (info["kept"], 0, 0, [], [], []), tag
            assert bytes(raws[i])[:64] == bytes(64) and bytes(raws[i])[72:] == bytes(56), tag   # everything but kept[0] is zero
            continue
        check_result(r, raws[i], info, len(j["srcs"]), tag)
        if not j["masks"]:
            assert plan.masks[i] is None
            continue
        assert len(plan.masks[i]) == len(j["srcs"])
        for m, t in enumerate(plan.masks[i]):
            got = words_of(t)
            assert t.dtype == torch.int32 and got.size == (exp.size + 31) // 32
            assert got.tobytes() == info["words"][m].tobytes(), tag + (m,)        # every word, padding bits included
            assert int(np.unpackbits(got.view(np.uint8)).sum()) == r["kept"][m]   # popcount(mask m) == kept[m]


SIZES = [1, 3, 4, 5, 23, 31, 32, 33, 63, 1023, 4096, 4097, 4110, 8191, 12289, 70001]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_emr_ragged_sizes(n, S, merge):
    """n = 23 and n = 4110: the last word mixes float4 lanes and tail elements; n = 1 and n = 3: tail only, the sums come from the
    tail alone; n = 4097: the tail stands behind the chunk's last float4 (the fifth slot, thread 0)."""
    c, srcs = inputs(n, S, seed=n + S)
    jobs = [mjob(c, srcs)]
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows, plan)


def mixed_jobs():
    """Mixed sizes, S = 1 .. 4, both ops, masks on and off, lam different per job; restore jobs with random words, garbage in the
    padding bits, and rescalers 0, 1 and a non-dyadic value."""
    rng = np.random.default_rng(8)
    jobs = []
    sizes = [12289, 1, 4097, 3, 1 << 18, 5, 8191, 4096, 70000, 1023, 23, 8193, 4110]
    for i, n in enumerate(sizes):
        S = 1 + i % 4
        c, srcs = planted(n, max(S, 2), seed=300 + i)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(F) * F(0.3)).astype(F))
        if i % 3 == 2:
            words = rng.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype("<u4")
            jobs.append(rjob(srcs[0], c, words, [0.0, 1.0, 1.7, 0.3][(i // 3) % 4]))
        else:
            jobs.append(mjob(c, srcs[:S], lam=[1, 0.75, 0.3][i % 3], masks=i % 2 == 0))
    return jobs


def test_emr_a_dozen_jobs_in_one_plan(merge):
    jobs = mixed_jobs()
    assert {j["op"] for j in jobs} == {"emr", "restore"} and {j.get("masks") for j in jobs} == {True, False, None}
    assert {j["rescale"] for j in jobs if j["op"] == "restore"} == {0.0, 1.0, 1.7, 0.3}
    outs, rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, outs, rows, plan)
    assert sum(r["zero"] for r in rows) > 0 and sum(r["conflict"] for r in rows) > 0


def test_emr_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one-chunk jobs (lengths cycled through 5, 1, 4097, 3, 2, 4099; 1 .. 4 sources), every input a 16-byte
    aligned view into one device buffer: each of the 12 workgroups per CU owns three chunks, every one of another job -- so a run
    loads another job's first record index at every step.  Masks on for two jobs of three.  Outputs, words and every result
    against the restatement."""
    jobs = [mjob(c, srcs, lam=[1, 0.75, 0.3][i % 3], masks=i % 3 != 1)
            for i, (c, srcs) in enumerate(tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted))]
    views = iter(one_buffer([a for j in jobs for a in [j["c"]] + j["srcs"]]))
    plan = merge.EmrPlan("cuda")
    outs = []
    for i, j in enumerate(jobs):
        base = next(views)
        outs.append(add_job(plan, j, str(i), base=base, srcs=[next(views) for _ in j["srcs"]]))
        assert plan.jobs[-1].base == base.data_ptr()  # the view itself, not a staged copy
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, outs, plan.report(), plan)


def test_emr_every_workgroup_owns_two_chunks_of_one_job(merge):
    """n = 4096 (2 grid + 3) + 5, S = 2, grid = 12 workgroups per CU (the launch rule of vlm_emr_run: EMR_BLOCKS_PER_CU x CUs): the
    one job's 2 grid + 4 chunks deal at least two to every workgroup that has any, so the record index advances inside a run and
    the fold adds more records than there are workgroups."""
    grid = 12 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 4096 * (2 * grid + 3) + 5
    src = open(os.path.join(ROOT, "vl-merging_amd", "csrc", "emr.hip")).read()
    assert "#define EMR_BLOCKS_PER_CU 12" in src and "chunk_grid(EMR_BLOCKS_PER_CU)" in src   # the launch rule read above
    c, srcs = inputs(n, 2, seed=5)
    jobs = [mjob(c, srcs)]
    outs, rows, plan = run_plan(merge, jobs)
    assert plan._header().n_chunks == 2 * grid + 4
    check_jobs(jobs, outs, rows, plan)


def test_emr_dst_may_be_base_or_a_source(merge):
    for n in (12289, 23, 3):
        c, srcs = planted(n, 3, seed=n)
        j = mjob(c, srcs)
        (want,), rows, plan0 = run_plan(merge, [j])
        want = want.cpu().numpy().tobytes()
        for which in ("base", 1):
            dev = [torch.from_numpy(s).cuda() for s in srcs]
            b = torch.from_numpy(c).cuda()
            out = b if which == "base" else dev[which]
            plan = merge.EmrPlan("cuda")
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
            if which != "base":
                assert b.cpu().numpy().tobytes() == c.tobytes()
        # restore in place: dst is the unified tensor, then the central tensor
        u, info = emr(c, srcs, 1)
        exp, _ = restore(u, c, info["words"][1], float(info["rescale"][1]))
        for which in ("u", "base"):
            du, db = torch.from_numpy(u).cuda(), torch.from_numpy(c).cuda()
            plan = merge.EmrPlan("cuda")
            got = plan.add_restore(du, db, dev_words(info["words"][1]), float(info["rescale"][1]), out=du if which == "u" else db)
            plan.run()
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == exp.tobytes(), (n, which)
            other, orig = (db, c) if which == "u" else (du, u)
            assert other.cpu().numpy().tobytes() == orig.tobytes()


def test_emr_run_three_times_same_bytes_same_words_same_results(merge):
    c4, s4 = planted(4110, 2, seed=4)
    jobs = [mjob(*planted(70001, 3, seed=1)), mjob(*planted(4097, 2, seed=2)), mjob(*planted(23, 2, seed=3)),
            rjob(s4[0], c4, pack(np.arange(4110) % 3 == 0), 1.7)]
    plan = merge.EmrPlan("cuda")
    outs = [add_job(plan, j, str(i)) for i, j in enumerate(jobs)]
    got, reports, raws = [], [], []
    for _ in range(3):
        poison(plan, outs)
        plan.run()
        torch.cuda.synchronize()
        got.append([o.cpu().numpy().tobytes() for o in outs] + [words_of(t).tobytes() for ms in plan.masks[:3] for t in ms])
        reports.append(plan.report())
        raws.append([bytes(r) for r in plan.results()])
    assert got[0] == got[1] == got[2]
    assert reports[0] == reports[1] == reports[2] and raws[0] == raws[1] == raws[2]
    check_jobs(jobs, outs, reports[0], plan)


# ---------------------------------------------------------------------------------------------------------------- restore
@pytest.mark.parametrize("n", [1, 3, 23, 32, 4097, 4110, 12289])
def test_emr_restore_with_the_devices_own_masks_and_rescalers(n, merge):
    """restore(uni = emr(lam = 1), c, mask_m, rescale_m) with the device's masks as they are and its rescalers as the report gives
    them == the restatement; all ones with rescale 1 gives c + (uni - c); all zeros gives c."""
    S = 3
    c, srcs = planted(n, S, seed=40 + n)
    (u_dev,), rows0, plan0 = run_plan(merge, [mjob(c, srcs, lam=1)])
    u, info = emr(c, srcs, 1)
    assert u_dev.cpu().numpy().tobytes() == u.tobytes()
    ones, zeros = np.full((n + 31) // 32, 0xFFFFFFFF, "<u4"), np.zeros((n + 31) // 32, "<u4")
    plan = merge.EmrPlan("cuda")
    cd = torch.from_numpy(c).cuda()
    outs = [plan.add_restore(u_dev, cd, plan0.masks[0][m], rows0[0]["rescale"][m], name=str(m)) for m in range(S)]
    assert [plan.jobs[m].mask[0] for m in range(S)] == [t.data_ptr() for t in plan0.masks[0]]
    outs += [plan.add_restore(u_dev, cd, dev_words(w), 1.0, name=nm) for w, nm in ((ones, "ones"), (zeros, "zeros"))]
    poison(plan, outs)
    plan.run()
    torch.cuda.synchronize()
    rows = plan.report()
    for m in range(S):
        want = restore(u, c, info["words"][m], info["rescale"][m])[0]
        assert outs[m].cpu().numpy().tobytes() == want.tobytes(), (n, m)
        assert (rows[m]["op"], rows[m]["kept"]) == ("restore", [info["kept"][m]])
    assert outs[S].cpu().numpy().tobytes() == (c + (u - c)).astype(F).tobytes() and rows[S]["kept"] == [n]
    assert outs[S + 1].cpu().numpy().tobytes() == c.tobytes() and rows[S + 1]["kept"] == [0]


@pytest.mark.parametrize("n", [23, 100, 4097, 4110, 8192 + 3])
def test_emr_restore_reads_no_word_past_the_mask(n, merge):
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
    plan = merge.EmrPlan("cuda")
    out = plan.add_restore(torch.from_numpy(srcs[0]).cuda(), torch.from_numpy(c).cuda(), view, 1.7)
    assert plan.jobs[0].mask[0] == view.data_ptr() == buf.data_ptr()  # the view itself
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == restore(srcs[0], c, words, 1.7)[0].tobytes()
    assert plan.report()[0]["kept"] == [int(keep.sum())]
    assert bool((buf[nw:] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- state dicts
def restate_state(sd, central, cfg, lam, layers=range(12)):
    """dst -> (expected tensor, info | None, source keys) for the block tensors of `layers`; single-source layers: the oracle's
    task-vector job."""
    exp = {}
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            if len(mods) == 1:
                exp[dst] = (mo.taskvec(central[dst], srcs, [1]), None, [src(mods[0])])
            else:
                out, info = emr(central[dst], srcs, lam)
                exp[dst] = (out.reshape(central[dst].shape), info, [src(m) for m in mods])
    return exp


@pytest.mark.parametrize("case", sorted(CASES))
def test_emr_merge_tiny_matches_restatement(case, merge):
    lam = 0.75
    cfg = merge_cfg(sum_lambda=lam, **CASES[case])
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    central_before = {key: v.clone() for key, v in central.items()}
    rows, plans, masks, rescalers = [], [], {}, {}
    res = merge.emr_merge(sd, cfg, central_weight={"state_dict": central}, masks_out=masks, rescalers_out=rescalers, report_out=rows,
                          plan_out=plans)
    torch.cuda.synchronize()
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    assert list(res.keys()) == list(ref.keys())
    exp = restate_state(sd_np, central_np, cfg, lam)
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
    by_dst = {r["dst"]: r for r in rows}
    assert sorted(by_dst) == sorted(d for d, (_, info, _) in exp.items() if info is not None)
    raws = dict(zip([r["dst"] for r in rows], plans[0].results()))
    want_masks, want_rescale = {}, {}
    for dst, r in by_dst.items():
        want, info, keys = exp[dst]
        assert (r["n"], r["op"]) == (want.size, "emr"), dst
        check_result(r, raws[dst], info, len(keys), dst)
        for m, key in enumerate(keys):
            want_masks[key], want_rescale[key] = info["words"][m], info["rescale"][m]
    assert sorted(masks) == sorted(want_masks) == sorted(rescalers)
    for key, t in masks.items():
        assert t.dtype == torch.int32 and t.is_cuda and words_of(t).tobytes() == want_masks[key].tobytes(), key
        assert type(rescalers[key]) is float and f32(rescalers[key]) == want_rescale[key].tobytes(), key
    assert len(plans) == (2 if case == "used_vqa" else 1) and isinstance(plans[0], merge.EmrPlan)
    if case == "used_vqa":
        assert isinstance(plans[1], merge.MergePlan)
    # without masks_out: the same tensors, no mask allocated
    plans2 = []
    res2 = merge.emr_merge(sd, cfg, central_weight=central, lam=lam, plan_out=plans2)
    torch.cuda.synchronize()
    assert all(res2[key].cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes() for key in res if is_block(key))
    assert all(ms is None for ms in plans2[0].masks)


@pytest.mark.parametrize("case", sorted(CASES))
def test_emr_restore_round_trip(case, merge):
    """emr_restore(emr_merge(lam = 1), masks, rescalers) returns exactly the source keys consumed, each the restatement's restore of
    the unified and the central tensor; single-source layers get the unified tensor itself; the rest passes through."""
    L = importlib.import_module("vl_merging_amd._lib")
    cfg = merge_cfg(sum_lambda=0.3, **CASES[case])   # lam = 1 is passed explicitly and wins
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    sd, central = to_dev(sd_np), to_dev(central_np)
    masks, rescalers, plans = {}, {}, []
    uni = merge.emr_merge(sd, cfg, central_weight=central, lam=1.0, masks_out=masks, rescalers_out=rescalers)
    back = merge.emr_restore(uni, masks, rescalers, cfg, central_weight={"state_dict": central}, plan_out=plans)
    torch.cuda.synchronize()
    exp = restate_state(sd_np, central_np, cfg, 1.0)
    consumed = [key for _, _, keys in exp.values() for key in keys]
    assert sorted(key for key in back if is_block(key)) == sorted(consumed)
    for dst, (u, info, keys) in exp.items():
        for m, key in enumerate(keys):
            if info is None:
                assert back[key] is uni[dst]
            else:
                want = restore(u, central_np[dst], info["words"][m], info["rescale"][m])[0]
                assert back[key].cpu().numpy().tobytes() == want.tobytes() and back[key].shape == sd[key].shape, key
    for key, v in back.items():
        if not is_block(key):
            assert v is uni[key] and v is sd[key]
    assert len(plans) == 1 and isinstance(plans[0], merge.EmrPlan) and len(plans[0].jobs) == len(masks)
    assert all(r["op"] == "restore" for r in plans[0].report())
    # masks from the CPU (as a masks file holds them) give the same tensors; a mask that does not fit is refused; so is a stray key;
    # a mask without its rescaler is a KeyError
    back2 = merge.emr_restore(uni, {key: t.cpu() for key, t in masks.items()}, dict(rescalers), cfg, central_weight=central)
    torch.cuda.synchronize()
    assert all(back2[key].cpu().numpy().tobytes() == back[key].cpu().numpy().tobytes() for key in back if is_block(key))
    key0 = sorted(masks)[0]
    with pytest.raises(L.VlmError):
        merge.emr_restore(uni, {key0: masks[key0][:-1]}, rescalers, cfg, central_weight=central)
    with pytest.raises(KeyError):
        merge.emr_restore(uni, {"transformer.blocks.0.attn.zz.qkv.weight": masks[key0]}, rescalers, cfg, central_weight=central)
    with pytest.raises(KeyError):
        merge.emr_restore(uni, masks, {key: v for key, v in rescalers.items() if key != key0}, cfg, central_weight=central)


# ---------------------------------------------------------------------------------------------------------------- command lines
def test_merge_ckpt_emr_and_tall_restore_as_child_processes(merge, tmp_path):
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = {key: torch.from_numpy(v) for key, v in tiny_state("all_moe").items()}
    central = {key: torch.from_numpy(v) for key, v in tiny_state("ufo", salt=7).items()}
    torch.save({"state_dict": sd}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": central}, tmp_path / "ufo.ckpt")
    out, rep, mfile = tmp_path / "uni.ckpt", tmp_path / "uni.json", tmp_path / "masks.pt"
    cmd = [sys.executable, TOOL, "--method", "emr", "--ckpt", str(tmp_path / "moe.ckpt"), "--out", str(out), "--report", str(rep),
           "--central", str(tmp_path / "ufo.ckpt"), "--masks-out", str(mfile), "--lambda", "1", "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = ckpt.load_ckpt(str(out))
    rep = json.load(open(rep))
    saved = ckpt.load_file(str(mfile))
    rows, masks, rescalers = [], {}, {}
    cfg = merge_cfg(sum_lambda=1)
    want = merge.emr_merge(to_dev(sd), cfg, central_weight=to_dev(central), masks_out=masks, rescalers_out=rescalers, report_out=rows)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(want.keys())
    for key in want:
        assert got[key].device.type == "cpu" and got[key].numpy().tobytes() == want[key].cpu().numpy().tobytes(), key
    assert rep["method"] == "emr" and rep["sum_lambda"] == 1 and "merge_ratio" in rep and rep["density"] is None   # the existing keys stay
    assert len(rep["tensors"]) == 12 * 13 and rep["tensors"] == rows   # JSON round-trips doubles, and floats that hold fp32 values
    assert saved["format"] == "emr-masks-1" and sorted(saved) == ["format", "masks", "rescalers"]
    assert sorted(saved["masks"]) == sorted(masks) == sorted(saved["rescalers"]) and len(masks) == 10 * 13 * 2 + 2 * 13 * 3
    for key, t in saved["masks"].items():
        assert t.dtype == torch.int32 and t.device.type == "cpu" and t.numpy().tobytes() == masks[key].cpu().numpy().tobytes(), key
        assert type(saved["rescalers"][key]) is float and saved["rescalers"][key] == rescalers[key], key
    # and back: ufo + masks + rescalers -> all_moe
    back_file = tmp_path / "back.ckpt"
    cmd = [sys.executable, RESTORE_TOOL, "--unified", str(out), "--central", str(tmp_path / "ufo.ckpt"), "--masks", str(mfile),
           "--out", str(back_file), "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    back = ckpt.load_ckpt(str(back_file))
    want_back = merge.emr_restore(want, masks, rescalers, cfg, central_weight=to_dev(central))
    torch.cuda.synchronize()
    assert list(back.keys()) == list(want_back.keys()) and sorted(key for key in back if is_block(key)) == sorted(masks)
    for key in want_back:
        assert back[key].device.type == "cpu" and back[key].numpy().tobytes() == want_back[key].cpu().numpy().tobytes(), key


def test_model_method_is_the_same_merge(merge, pkg):
    """ViLTransformerSS.emr_merge forwards to merge.emr_merge with the model's config (it is not wired to a config key)."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    m_want, m_got, r_want, r_got = {}, {}, {}, {}
    want = merge.emr_merge(sd, Stub.hparams.config, central_weight=central, masks_out=m_want, rescalers_out=r_want)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.emr_merge(Stub(), sd, masks_out=m_got, rescalers_out=r_got)
    torch.cuda.synchronize()
    assert all(got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes() for key in want if is_block(key))
    assert sorted(m_got) == sorted(m_want) and all(torch.equal(m_got[key], m_want[key]) for key in m_want)
    assert r_got == r_want and len(r_got) == len(m_got)
    ours = inspect.signature(merge.emr_merge).parameters
    theirs = inspect.signature(vm.ViLTransformerSS.emr_merge).parameters
    assert all(theirs[p].default == ours[p].default for p in ("lam", "masks_out", "rescalers_out"))
