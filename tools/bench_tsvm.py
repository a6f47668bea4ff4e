#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds) through TSV-M: the whole
tsvm_merge -- 48 weight matrices, the Jacobi SVDs of their 104 task vectors and of the 96 concatenated factor matrices, 108 other
tensors through the task-vector job, every blocking read included -- timed on stream events, `--reps` runs after `--warmup` runs.
Reports the wall time, the kernel launches the plans issued, and the sweeps each SVD took per working shape.  There is no
comparison run: nothing comparable exists (profiles/isoc_merge_base.json and profiles/wudi_merge_base.json hold the two other
matrix-aware merges of the same inputs).  Prints ONE JSON line; `--out FILE` also writes it to FILE (profiles/tsvm_merge_base.json
holds such a line, with the share of time in the Jacobi steps added from a separate kernel-stats run)."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    tsvm = importlib.import_module("vl_merging_amd.tsvm")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    plans, rows = [], []

    def merge():
        del plans[:], rows[:]
        return tsvm.tsvm_merge(sd, cfg, central_weight=central, plan_out=plans, report_out=rows)
    ms, lo = bm.timed(merge, args.reps, warmup=args.warmup)
    plan = plans[0]
    sweeps = {}
    for r in rows:
        p, q = min(r["shape"]), max(r["shape"])
        kS = r["k"] * r["S"]
        for key, vals in ((("tau", p, q), r["sweeps"]["tau"]), (("U", kS, p), [r["sweeps"]["U"]]), (("V", kS, q), [r["sweeps"]["V"]])):
            sweeps.setdefault("%s %dx%d" % key, []).extend(vals)
    res = {"workload": "base all_moe -> ufo, 48 matrices + 108 other tensors", "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "ms_median": ms, "ms_min": lo, "launches": plan.launches + len(plans) - 1,
           "scheduled_sweeps": tsvm.SWEEPS, "matrices": len(rows), "svd_groups": plan.groups,
           "sweeps": {k: {"min": min(v), "max": max(v), "svds": len(v)} for k, v in sorted(sweeps.items())},
           "converged": all(all(r["converged"]["tau"]) and r["converged"]["U"] and r["converged"]["V"] for r in rows),
           "dropped_max": max(max(r["dropped"].values()) for r in rows),
           "energy_kept_min": min(min(r["energy_kept"]) for r in rows), "k": sorted({r["k"] for r in rows})}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
