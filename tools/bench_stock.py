#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge
(sum_task_vectors' plan), the expert-pair statistics (expert_stats' plan) and the Model Stock merge (stock_merge's plan) over the
same inputs in one process, in that order, then the first two again; 20 stream-timed runs each after 3 warm-ups, medians.
A Model Stock run reads the inputs twice (the reducer, then the apply pass) and writes the outputs once.  Its bound is the sum of
the two yardsticks measured beside it: the reducer does strictly less per element than the pair statistics, the apply pass is the
task-vector pass plus one scalar -- `stock.ms_vs_bound` <= 1.  The split by kernel is what `rocprofv3 --kernel-trace --stats --
python tools/bench_stock.py` prints.  Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    tv, ps, st, rows = [], [], [], []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    merge.expert_stats(sd, cfg, central_weight=central, plan_out=ps)
    merge.stock_merge(sd, cfg, central_weight=central, plan_out=st, report_out=rows)
    tv, ps, st = tv[0], ps[0], st[0]
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    tv_ms, tv_min = bm.timed(tv.run, args.reps)
    ps_ms, ps_min = bm.timed(ps.run, args.reps)
    ms, ms_min = bm.timed(st.run, args.reps)
    # the yardsticks once more, after the merge: they did not drift while it ran
    tv_ms2, _ = bm.timed(tv.run, args.reps)
    ps_ms2, _ = bm.timed(ps.run, args.reps)
    tv_bytes = tv.bytes_read + tv.bytes_written
    res["taskvec"] = {"ms_median": tv_ms, "ms_min": tv_min, "ms_median_after": tv_ms2, "bytes": tv_bytes, "GBps": tv_bytes / tv_ms / 1e6}
    res["pairstats"] = {"ms_median": ps_ms, "ms_min": ps_min, "ms_median_after": ps_ms2, "bytes": ps.bytes_read,
                        "GBps": ps.bytes_read / ps_ms / 1e6}
    nbytes = st.bytes_read + st.bytes_written
    ts = [r["t"] for r in rows]
    res["stock"] = {"launches": 3, "ms_median": ms, "ms_min": ms_min, "bytes": nbytes, "GBps": nbytes / ms / 1e6,
                    "ms_vs_taskvec": ms / tv_ms, "ms_vs_bound": ms / (ps_ms + tv_ms), "within_bound": ms <= ps_ms + tv_ms,
                    # what is left for the reducer and the fold if the apply pass costs what the task-vector pass does
                    "reduce_ms_if_apply_is_taskvec": ms - tv_ms, "reduce_bytes": st.bytes_read // 2,
                    "t_min": min(ts), "t_median": sorted(ts)[len(ts) // 2], "t_max": max(ts)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
