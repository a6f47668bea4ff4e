"""Expert-pair statistics on the GPU (csrc/pairstats.hip through the C ABI) against the numpy restatement of the rule
(pairstats_restatement.py): every double is compared by its bytes, every count exactly.  The reference has no such measure."""
import importlib
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
from test_ties_gpu import CASES, planted, to_dev
import pairstats_restatement as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state, one_buffer, tiny_jobs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "expert_stats.py")
F = np.float32
PAIR_NAMES = ["v-l", "v-vl", "l-vl"]


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def job(srcs, c=None, tkeys=None):
    return dict(srcs=srcs, c=c, tkeys=tkeys)


def add_jobs(plan, jobs):
    for i, j in enumerate(jobs):
        plan.add([torch.from_numpy(s).cuda() for s in j["srcs"]], None if j["c"] is None else torch.from_numpy(j["c"]).cuda(),
                 tkeys=j["tkeys"], name=str(i))


def run_plan(merge, jobs):
    plan = merge.PairStatsPlan("cuda")
    add_jobs(plan, jobs)
    plan.run()
    torch.cuda.synchronize()
    return plan.report(), plan


def restate(j, name):
    return R.pair_stats(j["srcs"], j["c"], j["tkeys"], name=name)


def check_jobs(jobs, rows):
    assert len(rows) == len(jobs)
    for i, j in enumerate(jobs):
        assert R.bits(rows[i]) == R.bits(restate(j, str(i))), (i, j["srcs"][0].size, len(j["srcs"]))


def result_bytes(plan, i):
    """The raw result of job i as the device left it."""
    L = importlib.import_module("vl_merging_amd._lib")
    hdr = L.PairStatsHeader.from_buffer_copy(plan.ws[:56].cpu().numpy().tobytes())
    return plan.ws[hdr.results_off + 448 * i: hdr.results_off + 448 * (i + 1)].cpu().numpy().tobytes()


SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 1 << 20]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", [2, 3])
def test_pairstats_ragged_sizes(n, S, merge):
    """The tail alone, a partial wave, one full chunk, a chunk plus tail, 256 records to fold; with and without a base; every
    threshold zero and the keys TIES takes at density 0.2 -- the four variants as four jobs of one plan."""
    c, srcs = planted(n, S, seed=n + S)
    jobs = [job(srcs, c), job(srcs, c, R.density_keys(srcs, c, 0.2)), job(srcs), job(srcs, None, R.density_keys(srcs, None, 0.2))]
    rows, _ = run_plan(merge, jobs)
    check_jobs(jobs, rows)
    for r in rows[::2]:  # tkey = 0: the truncated statistics are the plain ones
        for p in r["pairs"]:
            assert (p["tlive"], p["tconflict"]) == (p["live"], p["conflict"]) and R.bits(p["tssd_sum"]) == R.bits(p["ssd_sum"])
    if n >= 1023:
        assert any(p["tlive"] < p["live"] for p in rows[1]["pairs"])


def dozen_jobs():
    rng = np.random.default_rng(8)
    jobs = []
    sizes = [12289, 1, 4097, 3, 1 << 18, 5, 8191, 4096, 70000, 1023, 2, 8193, 4099]
    for i, n in enumerate(sizes):
        S = 1 + i % 4
        c, srcs = planted(n, max(S, 2), seed=300 + i)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(F) * F(0.3)).astype(F))
        srcs = srcs[:S]
        base = None if i % 3 == 2 else c
        jobs.append(job(srcs, base, R.density_keys(srcs, base, [0.2, 0.05, 1.0][i % 3]) if i % 2 else None))
    return jobs


def test_pairstats_a_dozen_jobs_in_one_plan(merge):
    """Mixed sizes, S = 1 .. 4, with and without a base, zero and density keys: all six slots for S = 4, none for S = 1."""
    jobs = dozen_jobs()
    rows, plan = run_plan(merge, jobs)
    check_jobs(jobs, rows)
    assert sorted({len(r["pairs"]) for r in rows}) == [0, 1, 3, 6]
    assert sum(p["conflict"] for r in rows for p in r["pairs"]) > 0
    L = importlib.import_module("vl_merging_amd._lib")
    for i, j in enumerate(jobs):  # the slots a job does not have are zero in the raw result
        res = L.PairStatsResult.from_buffer_copy(result_bytes(plan, i))
        S = len(j["srcs"])
        assert all(res.sq[m] == 0 and res.nnz[m] == 0 for m in range(S, 4))
        for k in range(S * (S - 1) // 2, 6):
            assert (res.dot[k], res.dist2[k], res.ssd[k], res.tssd[k], res.live[k], res.conflict[k], res.tlive[k],
                    res.tconflict[k]) == (0,) * 8


def test_pairstats_runs_of_chunks_cross_job_boundaries(merge):
    """2 x 12 x CUs + 7 one- and two-chunk jobs (helpers/merge_inputs.tiny_jobs), every input a 16-byte aligned view into one
    device buffer, used unstaged: every workgroup's run of chunks holds several jobs, so it enters a job, loads its keys and its
    first record index at every step.  Every result against the restatement."""
    data = tiny_jobs(torch.cuda.get_device_properties(0).multi_processor_count, planted)
    some_keys = [0, 0x3E000000, 0x3E800000, 0x3F000000, 0x3F800000]  # the keys of 0, 1/8, 1/4, 1/2, 1
    jobs = [job(srcs, c if i % 3 else None, [some_keys[(7 * i + m) % 5] for m in range(len(srcs))] if i % 2 else None)
            for i, (c, srcs) in enumerate(data)]
    views = iter(one_buffer([a for j, (c, _) in zip(jobs, data) for a in [c] + j["srcs"]]))
    plan = merge.PairStatsPlan("cuda")
    for i, j in enumerate(jobs):
        base = next(views)
        srcs = [next(views) for _ in j["srcs"]]
        plan.add(srcs, base if j["c"] is not None else None, tkeys=j["tkeys"], name=str(i))
        assert plan.jobs[-1].base == (base.data_ptr() if j["c"] is not None else None)  # the view itself, not a staged copy
        assert [plan.jobs[-1].src[m] for m in range(len(srcs))] == [s.data_ptr() for s in srcs]
    plan.run()
    torch.cuda.synchronize()
    check_jobs(jobs, plan.report())


def test_pairstats_position_in_a_plan_does_not_show(merge):
    n = 12289
    c, srcs = planted(n, 3, seed=1)
    a = job(srcs, c, R.density_keys(srcs, c, 0.2))
    other = []
    for m in (4097, 70000):
        oc, osrcs = planted(m, 2, seed=m)
        other.append(job(osrcs, oc))
    rows1, plan1 = run_plan(merge, [a] + other)
    rows2, plan2 = run_plan(merge, other + [a])
    assert result_bytes(plan1, 0) == result_bytes(plan2, 2)
    assert R.bits({**rows1[0], "dst": None}) == R.bits({**rows2[2], "dst": None}) == R.bits(restate(a, None))


def test_pairstats_run_three_times_same_bytes_inputs_untouched(merge):
    shapes = ((70001, 3), (4097, 2), (3, 2), (5000, 4))
    jobs = []
    for n, S in shapes:
        c, srcs = planted(n, min(S, 3), seed=n)
        srcs = srcs + [c[::-1].copy()] * (S - len(srcs))
        jobs.append(job(srcs, c, R.density_keys(srcs, c, 0.2)))
    plan = merge.PairStatsPlan("cuda")
    add_jobs(plan, jobs)
    inputs = list(plan.keep)
    before = [t.cpu().numpy().tobytes() for t in inputs]
    got, reports = [], []
    for _ in range(3):
        plan.run()
        torch.cuda.synchronize()
        got.append([result_bytes(plan, i) for i in range(len(jobs))])
        reports.append(plan.report())
    assert got[0] == got[1] == got[2]
    assert R.bits(reports[0]) == R.bits(reports[1]) == R.bits(reports[2])
    check_jobs(jobs, reports[0])
    assert len(inputs) == sum(S + 1 for _, S in shapes)
    assert [t.cpu().numpy().tobytes() for t in inputs] == before  # every source and every base: read only
    assert plan.bytes_written == 0 and plan.bytes_read == 4 * sum(n * (S + 1) for n, S in shapes)
    # other keys for a job: the plan is uploaded again and the truncated statistics follow
    plan.set_tkeys(1, [0, 0])
    plan.run()
    torch.cuda.synchronize()
    jobs[1]["tkeys"] = [0, 0]
    check_jobs(jobs, plan.report())


def test_pairstats_upload_argument_checks_on_device(merge):
    L = importlib.import_module("vl_merging_amd._lib")
    lib = L.get_lib()
    plan = merge.PairStatsPlan("cuda")
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
        plan.add([a, a], a, tkeys=[0])
    with pytest.raises(L.VlmError):
        plan.add([a, a], a, tkeys=[0, 2 ** 32])
    assert plan.jobs == []
    assert plan.add([a + 1, 2 - a], a) is None  # nothing is allocated: there is no output
    # a misaligned source is staged by add(); handed to the library as it is, it is refused
    arr = (L.PairStatsJob * 1)(*plan.jobs)
    ws = torch.empty(lib.vlm_pairstats_plan_bytes(1, 64), dtype=torch.uint8, device="cuda")
    assert lib.vlm_pairstats_plan_upload(arr, 1, L.ptr(ws), 512, L.stream_ptr()) == -3  # VLM_ERR_WORKSPACE
    buf = torch.zeros(256, device="cuda")
    for field, value, rc in (("n_src", 0, -1), ("n_src", 5, -1), ("n_elem", 0, -1), ("base", buf.data_ptr() + 4, -1),
                             ("src0", buf.data_ptr() + 8, -1), ("src0", 0, -1), ("base", 0, 0), ("n_src", 1, 0)):
        bad = L.PairStatsJob.from_buffer_copy(bytes(plan.jobs[0]))
        if field == "src0":
            bad.src[0] = value
        else:
            setattr(bad, field, value)
        got = lib.vlm_pairstats_plan_upload((L.PairStatsJob * 1)(bad), 1, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert got == rc, (field, value)  # base = NULL and n_src = 1 are fine: the controls that pass
    misaligned = torch.zeros(68, device="cuda")[1:65]
    plan.add([misaligned, a], a)
    assert plan.jobs[-1].src[0] != misaligned.data_ptr() and plan.jobs[-1].src[0] % 16 == 0
    plan.run()
    torch.cuda.synchronize()
    rows = plan.report()
    x, y = np.ones(64), 2.0 - 2.0 * np.arange(64)  # (a + 1) - a, (2 - a) - a: exact in fp32
    p = rows[0]["pairs"][0]
    assert rows[0]["sq"] == [float((x * x).sum()), float((y * y).sum())] and p["dot"] == float((x * y).sum())
    assert (p["live"], p["conflict"], rows[0]["nnz"]) == (64, 62, [64, 63])


def restate_state(sd, central, cfg, raw=False, trunc_rms=None, layers=range(12)):
    """What expert_stats returns for the tensors of `layers`, from the restatement; the walk is restated from the oracle's names."""
    tensors = []
    for i in layers:
        mods = mo._modalities(cfg, i)
        for src, dst in mo._names(i):
            srcs = [sd[src(m)] for m in mods]
            c = None if raw else central[dst]
            row = R.pair_stats(srcs, c, name=dst)
            if trunc_rms is not None:
                row = R.pair_stats(srcs, c, R.rms_keys(row, trunc_rms), name=dst)
            tensors.append({"dst": dst, "n": row["n"], "sources": list(mods),
                            **{k: dict(zip(mods, row[k])) for k in ("sq", "nnz", "tkey")},
                            "pairs": {"%s-%s" % (mods[p["a"]], mods[p["b"]]): {k: v for k, v in p.items() if k not in ("a", "b")}
                                      for p in row["pairs"]}})
    by_pair = {name: [(t["n"], t["pairs"][name]) for t in tensors if name in t["pairs"]] for name in PAIR_NAMES}
    return {"raw": raw, "trunc_rms": trunc_rms, "tensors": tensors,
            "summary": R.summary({k: v for k, v in by_pair.items() if v})}


@pytest.fixture(scope="module")
def tiny():
    sd_np, central_np = tiny_state("all_moe"), tiny_state("ufo", salt=7)
    return sd_np, central_np, to_dev(sd_np), to_dev(central_np)


@pytest.mark.parametrize("case", sorted(CASES))
def test_expert_stats_tiny_matches_restatement(case, merge, tiny):
    sd_np, central_np, sd, central = tiny
    cfg = merge_cfg(sum_lambda=0.75, **CASES[case])
    inputs = dict(sd, **{"central." + k: v for k, v in central.items()})
    before = {k: v.clone() for k, v in inputs.items()}
    plans = []
    got = merge.expert_stats(sd, cfg, central_weight={"state_dict": central}, plan_out=plans)
    ref = merge.sum_task_vectors(sd, cfg, central_weight=central)
    torch.cuda.synchronize()
    block = [k for k in ref if "transformer.blocks." in k and "gamma" not in k]
    assert len(got["tensors"]) == 12 * 13 and [t["dst"] for t in got["tensors"]] == block  # keys and order of sum_task_vectors
    want = restate_state(sd_np, central_np, cfg)
    assert R.bits(got) == R.bits(want)
    assert list(got["summary"]) == (["v-l"] if case != "all" else PAIR_NAMES)
    for t in got["tensors"]:
        for p in t["pairs"].values():  # trunc_rms=None: every threshold is zero
            assert R.bits(p["tssd_sum"]) == R.bits(p["ssd_sum"]) and (p["tlive"], p["tconflict"]) == (p["live"], p["conflict"])
    if case == "used_vqa":  # layers 10, 11: the vl expert alone -- sq and nnz only
        assert [t["sources"] for t in got["tensors"][-26:]] == [["vl"]] * 26 and all(t["pairs"] == {} for t in got["tensors"][-26:])
    assert len(plans) == 1 and isinstance(plans[0], merge.PairStatsPlan) and plans[0].bytes_written == 0
    assert json.loads(json.dumps(got)) == got  # the CLI's report is this dictionary
    # raw: no central checkpoint is needed (none can be loaded from this config), the walk is merge_weights'
    raw = merge.expert_stats(sd, cfg, raw=True)
    assert R.bits(raw) == R.bits(restate_state(sd_np, None, cfg, raw=True))
    assert [t["dst"] for t in raw["tensors"]] == [k for k in merge.merge_weights(sd, cfg) if k in set(block)]
    # the truncated statistics at one root mean square: the restatement fed the host-computed keys
    tr = merge.expert_stats(sd, cfg, central_weight=central, trunc_rms=1.0)
    assert R.bits(tr) == R.bits(restate_state(sd_np, central_np, cfg, trunc_rms=1.0))
    assert any(p["tlive"] < p["live"] for t in tr["tensors"] for p in t["pairs"].values())
    # a key the central checkpoint lacks raises as in sum_task_vectors; an already merged key passes through: no row
    with pytest.raises(KeyError):
        merge.expert_stats(sd, cfg, central_weight={k: v for k, v in central.items() if "blocks.3.norm1.weight" not in k})
    fewer = {k: v for k, v in sd.items() if "transformer.blocks.0." not in k}
    fewer.update({k: v for k, v in ref.items() if "transformer.blocks.0." in k})
    part = merge.expert_stats(fewer, cfg, central_weight=central)
    assert R.bits(part["tensors"]) == R.bits(want["tensors"][13:])
    torch.cuda.synchronize()
    assert all(torch.equal(v, inputs[k]) for k, v in before.items())  # the experts and the central tensors are inputs only


def test_pairstats_base_size(merge):
    """Base size (the inputs of test_dare_base_size): layers 0 (two sources) and 11 (three) against the restatement, every other
    row finite; the plan's byte counts; and run() returns while its launches are still queued."""
    L = importlib.import_module("vl_merging_amd._lib")
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    cfg = merge_cfg(sum_lambda=0.75)
    plans = []
    got = merge.expert_stats(sd, cfg, central_weight=central, plan_out=plans)
    plan = plans[0]
    assert plan.bytes_written == 0
    assert plan.bytes_read == 4 * sum(int(j.n_elem) * (j.n_src + 1) for j in plan.jobs) == 737058816 + 340180992
    assert len(got["tensors"]) == 12 * 13
    want = restate_state(sd_np, central_np, cfg, layers=(0, 11))
    assert R.bits(got["tensors"][:13] + got["tensors"][-13:]) == R.bits(want["tensors"])
    for t in got["tensors"]:
        vals = list(t["sq"].values()) + [v for p in t["pairs"].values() for v in p.values() if isinstance(v, float)]
        assert all(math.isfinite(v) for v in vals), t["dst"]
        assert all(p["live"] <= t["n"] and p["cosine"] is not None for p in t["pairs"].values())
    # no host synchronisation between upload and the end of run(): the ENQUEUE is timed behind a 0.2 s spin kernel on the same
    # stream, as test_dare_base_size does.  The spin's own length is checked, so the bound cannot pass vacuously.
    import time
    first = plan.report()
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
    print("pairstats enqueue %.6f s behind a spin of %.3f s" % (dt, spin))
    assert spin >= 0.15, "the spin kernel was too short (%.3f s) for the enqueue bound to mean anything" % spin
    assert dt < 0.05, "PairStatsPlan.run() took %.3f s behind a %.3f s spin: it waited for the device" % (dt, spin)
    assert still_queued, "the work of run() was complete when it returned"
    assert R.bits(plan.report()) == R.bits(first)


def test_expert_stats_cli_as_a_child_process(merge, tmp_path, tiny):
    _, _, sd, central = tiny
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}}, tmp_path / "moe.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in central.items()}}, tmp_path / "ufo.ckpt")
    rep = tmp_path / "stats.json"
    cmd = [sys.executable, TOOL, "--ckpt", str(tmp_path / "moe.ckpt"), "--central", str(tmp_path / "ufo.ckpt"), "--trunc-rms", "1.0",
           "--report", str(rep), "with", "vlffn_start_layer_index=10"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = merge.expert_stats(sd, merge_cfg(), central_weight=central, trunc_rms=1.0)
    assert json.load(open(rep)) == want
    assert sorted(os.listdir(tmp_path)) == ["moe.ckpt", "stats.json", "ufo.ckpt"]  # it writes no checkpoint
    rep2 = tmp_path / "raw.json"
    r = subprocess.run([sys.executable, TOOL, "--ckpt", str(tmp_path / "moe.ckpt"), "--raw", "--report", str(rep2), "with",
                        "vlffn_start_layer_index=10"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.load(open(rep2)) == merge.expert_stats(sd, merge_cfg(), raw=True)


def test_model_method_is_the_same_statistics(merge, pkg, tiny):
    """ViLTransformerSS.expert_stats forwards to merge.expert_stats with the model's config."""
    vm = importlib.import_module("vl_merging_amd.vilt.modules.vilt_module")

    class Stub:
        device = torch.device("cuda", torch.cuda.current_device())
        _merge_device = vm.ViLTransformerSS._merge_device

        class hparams:
            config = dict(merge_cfg(sum_lambda=0.75), central_weight=None)

    _, _, sd, central = tiny
    want = merge.expert_stats(sd, Stub.hparams.config, central_weight=central, trunc_rms=0.5)
    import unittest.mock as mock
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    with mock.patch.object(ckpt, "load_file", lambda path: {"state_dict": central}):
        got = vm.ViLTransformerSS.expert_stats(Stub(), sd, trunc_rms=0.5)
    assert R.bits(got) == R.bits(want)
    assert R.bits(vm.ViLTransformerSS.expert_stats(Stub(), sd, raw=True)) == R.bits(merge.expert_stats(sd, Stub.hparams.config, raw=True))
    assert vm.ViLTransformerSS.expert_stats.__defaults__ == (False, None)  # merge.expert_stats' defaults
