#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the spherical merge of the
task vectors of all 156 block tensors, per tensor and per row, with two sources (the v and l experts) and with three (a third
expert of the same shapes is made from the two), beside the task-vector merge (sum_task_vectors' plan), Model Stock (stock_merge's
plan) and DELLA (della_merge's plan) over the same inputs in one process; 20 stream-timed runs each after 3 warm-ups, medians; the
yardsticks are timed again at the end.
A tensor-mode run reads the inputs twice and writes the outputs once, as Model Stock does: `ms_vs_stock` is its ratio to Model Stock
at the same source count where there is one (the yardstick's plan has two sources in ten layers and three in two).  A row-mode run
reads them once, as DELLA does: `ms_vs_della`, and `ms_at_taskvec_rate` = what S + 2 transfers cost at the rate the task-vector pass
reaches beside it.  The split by kernel is what `rocprofv3 --kernel-trace --stats -- python tools/bench_sphere.py` prints.  Prints
ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    tv, st, de = [], [], []
    merge.sum_task_vectors(sd, cfg, central_weight=central, plan_out=tv)
    merge.stock_merge(sd, cfg, central_weight=central, plan_out=st)
    merge.della_merge(sd, cfg, central_weight=central, plan_out=de)
    tv, st, de = tv[0], st[0], de[0]
    # every block tensor with the v and l experts as sources (and a third of the same shape for S = 3), by tensor and by row
    two = dict(cfg, vlffn_start_layer_index=merge.NUM_MERGE_LAYERS)
    plans = {}
    for S in (2, 3):
        for rows in (False, True):
            plan = merge.SpherePlan("cuda")
            for dst, mods, srcs, _ in merge._walk(sd, two, central):
                ts = merge._tensors(srcs)
                if S == 3:
                    ts = ts + [central[dst] + 0.5 * (ts[0] - ts[1])]
                plan.add(ts, central[dst], [1.0 / S] * S, lam=0.75, rows=rows, name=dst)
            plan.run()
            plans[(S, rows)] = plan
    torch.cuda.synchronize()
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    yard = {"taskvec": tv, "stock": st, "della": de}
    first = {k: bm.timed(p.run, args.reps) for k, p in yard.items()}
    timed = {k: bm.timed(p.run, args.reps) for k, p in plans.items()}
    again = {k: bm.timed(p.run, args.reps)[0] for k, p in yard.items()}
    for k, p in yard.items():
        nbytes = p.bytes_read + p.bytes_written
        res[k] = {"ms_median": first[k][0], "ms_min": first[k][1], "ms_median_after": again[k], "bytes": nbytes,
                  "TBps": nbytes / first[k][0] / 1e9}
    tv_rate = res["taskvec"]["bytes"] / res["taskvec"]["ms_median"]
    for (S, rows), p in plans.items():
        ms, ms_min = timed[(S, rows)]
        nbytes = p.bytes_read + p.bytes_written
        rep = p.report()
        row = {"sources": S, "launches": 4, "ms_median": ms, "ms_min": ms_min, "bytes": nbytes, "TBps": nbytes / ms / 1e9,
               "ms_at_taskvec_rate": nbytes / tv_rate, "ms_vs_stock": ms / res["stock"]["ms_median"],
               "ms_vs_della": ms / res["della"]["ms_median"], "ms_vs_taskvec": ms / res["taskvec"]["ms_median"]}
        row["ms_vs_bound"] = ms / row["ms_at_taskvec_rate"]
        if rows:
            row.update(groups=sum(r["rows"] for r in rep), rows_linear=sum(r["rows_linear"] for r in rep),
                       rows_zero=sum(r["rows_zero"] for r in rep), resid_max=max(r["resid_max"] for r in rep))
        else:
            row.update(groups=len(rep), resid_max=max(r["resid"] for r in rep), not_ok=sum(r["status"] != "ok" for r in rep))
        res["sphere_%s_s%d" % ("rows" if rows else "tensor", S)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
