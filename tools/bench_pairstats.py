#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan) and the expert-pair statistics (expert_stats' plan) over the same inputs in one process, 20 stream-timed
runs each after warm-up, medians; GB/s for both and t_pairstats / t_taskvec.  The statistics read what the merge reads and write
one record per chunk (not counted).  The split by kernel is what `rocprofv3 --kernel-trace --stats -- python
tools/bench_pairstats.py` prints.  Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--raw", action="store_true", help="the weights themselves: no central tensor is read")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    tv = []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    tv = tv[0]
    tv_ms, tv_min = bm.timed(tv.run, args.reps)
    tv_bytes = tv.bytes_read + tv.bytes_written
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "taskvec": {"ms_median": tv_ms, "ms_min": tv_min, "bytes": tv_bytes, "GBps": tv_bytes / tv_ms / 1e6}}
    ps = []
    stats = merge.expert_stats(sd, cfg, central_weight=central, raw=args.raw, plan_out=ps)
    ps = ps[0]
    ms, ms_min = bm.timed(ps.run, args.reps)
    res["pairstats"] = {"raw": args.raw, "launches": 2, "ms_median": ms, "ms_min": ms_min, "bytes": ps.bytes_read,
                        "GBps": ps.bytes_read / ms / 1e6, "ms_vs_taskvec": ms / tv_ms,
                        "summary": {k: {m: v[m] for m in ("l2", "cosine", "ssd", "conflict_rate")} for k, v in stats["summary"].items()}}
    # the task-vector plan once more, after the statistics: the yardstick did not drift while they ran
    tv_ms2, _ = bm.timed(tv.run, args.reps)
    res["taskvec"]["ms_median_after"] = tv_ms2
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
