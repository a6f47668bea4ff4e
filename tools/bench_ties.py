#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan) and the TIES merge at density 0.2 in one process, 20 stream-timed runs each, medians; for TIES also the mean per
launch (whole / 7; the split by kernel is what `rocprofv3 --kernel-trace --stats -- python tools/bench_ties.py` prints).
Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    from oracle import synth
    from oracle.detweights import det_array
    torch.cuda.set_device(0)
    sd = {k: torch.from_numpy(det_array(k, s)).cuda() for k, (s, dt) in synth.block_shapes(768, 3072, "all_moe").items()}
    central = {k: torch.from_numpy(det_array(k, s, 7)).cuda() for k, (s, dt) in synth.block_shapes(768, 3072, "ufo").items()}
    cfg = dict(vlffn_start_layer_index=10, only_activate_used_experts=False, merge_ratio=0.5, sum_lambda=0.75, loss_names={})
    tv, ti = [], []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    merge.ties_merge(sd, cfg, central_weight=central, density=args.density, plan_out=ti)
    tv, ti = tv[0], ti[0]
    tv_ms, tv_min = timed(tv.run, args.reps)
    ti_ms, ti_min = timed(ti.run, args.reps)
    tv_bytes = tv.bytes_read + tv.bytes_written
    ti_bytes = ti.bytes_read + ti.bytes_written
    rep = ti.report()
    n = sum(r["n"] for r in rep)
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "taskvec": {"ms_median": tv_ms, "ms_min": tv_min, "bytes": tv_bytes, "GBps": tv_bytes / tv_ms / 1e6},
           "ties": {"density": args.density, "launches": 7, "ms_median": ti_ms, "ms_min": ti_min, "ms_per_launch_mean": ti_ms / 7,
                    "bytes": ti_bytes, "GBps": ti_bytes / ti_ms / 1e6, "ms_vs_taskvec": ti_ms / tv_ms,
                    "kept_fraction": sum(sum(r["kept"]) for r in rep) / sum(r["n"] * len(r["kept"]) for r in rep),
                    "conflict_fraction": sum(r["conflict"] for r in rep) / n, "empty_fraction": sum(r["empty"] for r in rep) / n}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
