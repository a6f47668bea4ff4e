#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan), the TIES merge (ties_merge's plan) and the SCE merge (sce_merge's plan) over the same inputs in one
process, in that order, then the first two again; 20 stream-timed runs each after 3 warm-ups, medians.
An SCE run reads the inputs five times (three histogram passes over the variance key, the reducer, the apply pass) and writes the
outputs once; a TIES run reads them four times and writes once.  The bound is the traffic: `sce.ms_at_taskvec_rate` is what five
reads and one write cost at the rate the task-vector pass reaches beside it, `sce.ms_vs_bound` the ratio to it, `sce.ms_vs_ties` the
ratio to TIES.  The split by kernel is what `rocprofv3 --kernel-trace --stats -- python tools/bench_sce.py` prints.  Prints ONE JSON
line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    tv, ti, sc, rows = [], [], [], []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    merge.ties_merge(sd, cfg, central_weight=central, density=args.density, plan_out=ti)
    merge.sce_merge(sd, cfg, central_weight=central, density=args.density, plan_out=sc, report_out=rows)
    tv, ti, sc = tv[0], ti[0], sc[0]
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "density": args.density}
    tv_ms, tv_min = bm.timed(tv.run, args.reps)
    ti_ms, ti_min = bm.timed(ti.run, args.reps)
    ms, ms_min = bm.timed(sc.run, args.reps)
    # the yardsticks once more, after the merge: they did not drift while it ran
    tv_ms2, _ = bm.timed(tv.run, args.reps)
    ti_ms2, _ = bm.timed(ti.run, args.reps)
    tv_bytes = tv.bytes_read + tv.bytes_written
    ti_bytes = ti.bytes_read + ti.bytes_written
    res["taskvec"] = {"ms_median": tv_ms, "ms_min": tv_min, "ms_median_after": tv_ms2, "bytes": tv_bytes, "GBps": tv_bytes / tv_ms / 1e6}
    res["ties"] = {"launches": 7, "ms_median": ti_ms, "ms_min": ti_min, "ms_median_after": ti_ms2, "bytes": ti_bytes,
                   "GBps": ti_bytes / ti_ms / 1e6}
    nbytes = sc.bytes_read + sc.bytes_written
    at_rate = nbytes / (tv_bytes / tv_ms)
    res["sce"] = {"launches": 9, "ms_median": ms, "ms_min": ms_min, "bytes": nbytes, "GBps": nbytes / ms / 1e6,
                  "ms_at_taskvec_rate": at_rate, "ms_vs_bound": ms / at_rate, "ms_vs_ties": ms / ti_ms, "ms_vs_taskvec": ms / tv_ms,
                  "bytes_per_pass": sc.bytes_read // sc.PASSES,
                  "kept_share": sum(r["kept"] for r in rows) / sum(r["n"] for r in rows),
                  "conflict_share": sum(r["conflict"] for r in rows) / sum(r["n"] for r in rows)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
