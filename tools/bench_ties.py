#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan) and the TIES merge at density 0.2 in one process, 20 stream-timed runs each, medians; for TIES also the mean per
launch (whole / 7; the split by kernel is what `rocprofv3 --kernel-trace --stats -- python tools/bench_ties.py` prints).
Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    tv, ti = [], []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    merge.ties_merge(sd, cfg, central_weight=central, density=args.density, plan_out=ti)
    tv, ti = tv[0], ti[0]
    tv_ms, tv_min = bm.timed(tv.run, args.reps)
    ti_ms, ti_min = bm.timed(ti.run, args.reps)
    tv_bytes = tv.bytes_read + tv.bytes_written
    ti_bytes = ti.bytes_read + ti.bytes_written
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "taskvec": {"ms_median": tv_ms, "ms_min": tv_min, "bytes": tv_bytes, "GBps": tv_bytes / tv_ms / 1e6},
           "ties": {"density": args.density, "launches": 7, "ms_median": ti_ms, "ms_min": ti_min, "ms_per_launch_mean": ti_ms / 7,
                    "bytes": ti_bytes, "GBps": ti_bytes / ti_ms / 1e6, "ms_vs_taskvec": ti_ms / tv_ms,
                    **bm.report_fractions(ti.report())}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
