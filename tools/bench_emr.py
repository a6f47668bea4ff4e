#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan), the consensus merge with its TALL masks on (the pass whose traffic EMR shares) and EMR-Merging with its
masks off and on, over the same inputs in one process.  `--rounds` alternating blocks of `--reps` stream-timed runs each after
warm-up; per plan the median of the blocks' medians, `ms_vs_taskvec` against the task-vector plan's, and `spread` = (largest -
smallest block median) / median: the same-box repeat spread the comparison has to be read against.  Also times the restore plan
(ufo + masks + rescalers -> every expert, one job per expert and tensor).  The split by kernel is what `rocprofv3 --kernel-trace
--stats -- python tools/bench_emr.py` prints.  Prints ONE JSON line.  `--out FILE` also writes it to FILE
(profiles/emr_merge_base.json holds such a line)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tall-lambda", dest="tall_lambda", type=float, default=0.4)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()

    def first_plan(fn, **kw):
        plans = []
        out = fn(sd, cfg, central_weight=central, plan_out=plans, **kw)
        return plans[0], out

    masks, rescalers = {}, {}
    plans = {"taskvec": first_plan(merge.sum_task_vectors)[0],
             "consensus_masks": first_plan(merge.consensus_merge, tall_lambda=args.tall_lambda, k=args.k, masks_out={})[0],
             "emr": first_plan(merge.emr_merge)[0]}
    plans["emr_masks"], unified = first_plan(merge.emr_merge, lam=1.0, masks_out=masks, rescalers_out=rescalers)
    restore = []
    merge.emr_restore(unified, masks, rescalers, cfg, central_weight=central, plan_out=restore)
    plans["restore"] = restore[0]
    blocks = {name: [] for name in plans}
    fastest = {name: float("inf") for name in plans}
    for _ in range(args.rounds):  # alternating blocks: a drift of the box shows as spread, not as a difference between plans
        for name, plan in plans.items():
            med, lo = bm.timed(plan.run, args.reps)
            blocks[name].append(med)
            fastest[name] = min(fastest[name], lo)
    tv_ms = statistics.median(blocks["taskvec"])
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "rounds": args.rounds, "tall_lambda": args.tall_lambda, "k": args.k}
    for name, plan in plans.items():
        ms = statistics.median(blocks[name])
        nbytes = plan.bytes_read + plan.bytes_written
        res[name] = {"ms_median": ms, "ms_min": fastest[name], "ms_blocks": blocks[name], "spread": (max(blocks[name]) - min(blocks[name])) / ms,
                     "bytes": nbytes, "GBps": nbytes / ms / 1e6, "ms_vs_taskvec": ms / tv_ms, "launches": 1 if name == "taskvec" else 2}
    rep = plans["emr_masks"].report()
    n = sum(r["n"] for r in rep)
    hdr = plans["emr_masks"]._header()
    res["emr_masks"].update(mask_bytes=sum(4 * t.numel() for t in masks.values()), record_bytes=int(hdr.n_chunks) * 8 * 14,
                            kept_fraction=sum(sum(r["kept"]) for r in rep) / sum(r["n"] * len(r["kept"]) for r in rep),
                            zero_fraction=sum(r["zero"] for r in rep) / n, conflict_fraction=sum(r["conflict"] for r in rep) / n,
                            rescale_min=min(min(r["rescale"]) for r in rep), rescale_max=max(max(r["rescale"]) for r in rep))
    res["emr_masks_vs_consensus_masks"] = res["emr_masks"]["ms_median"] / res["consensus_masks"]["ms_median"]
    res["record_bytes_share"] = res["emr_masks"]["record_bytes"] / res["emr_masks"]["bytes"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
