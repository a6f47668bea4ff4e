#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds): the task-vector merge, the
TIES merge at density 0.2 and the band (Model Breadcrumbs) merge at density 0.9 / gamma 0.01 in both modes, in ONE process and in
alternating blocks: every round times each of the four plans once, 20 stream-timed runs after warm-up, and a plan's figure is the
median of its blocks' medians.  A band run moves exactly the bytes of a TIES run, so TIES in the same process is the yardstick:
`ms_vs_ties`, beside the spread of the TIES blocks themselves.  The split by kernel is what
`rocprofv3 --kernel-trace --stats -- python tools/bench_band.py` prints.  Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--ties-density", type=float, default=0.2)
    ap.add_argument("--density", type=float, default=0.9)
    ap.add_argument("--gamma", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    plans = {}
    for name, fn, kw in (("taskvec", merge.sum_task_vectors, {}),
                         ("ties", merge.ties_merge, dict(density=args.ties_density)),
                         ("band_linear", merge.band_merge, dict(density=args.density, gamma=args.gamma, mode="linear")),
                         ("band_ties", merge.band_merge, dict(density=args.density, gamma=args.gamma, mode="ties"))):
        got = []
        fn(sd, cfg, central_weight=central, plan_out=got, **kw)
        plans[name] = got[0]
    blocks = {name: [] for name in plans}
    fastest = {name: float("inf") for name in plans}
    for _ in range(args.rounds):
        for name, plan in plans.items():
            med, lo = bm.timed(plan.run, args.reps)
            blocks[name].append(med)
            fastest[name] = min(fastest[name], lo)
    ms = {name: statistics.median(b) for name, b in blocks.items()}
    res = {"workload": "base all_moe -> ufo, 156 tensors", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "rounds": args.rounds}
    for name, plan in plans.items():
        nbytes = plan.bytes_read + plan.bytes_written
        res[name] = {"ms_median": ms[name], "ms_min": fastest[name], "ms_blocks": blocks[name], "bytes": nbytes,
                     "GBps": nbytes / ms[name] / 1e6}
    res["ties"].update(density=args.ties_density, launches=7, ms_vs_taskvec=ms["ties"] / ms["taskvec"],
                       blocks_spread=(max(blocks["ties"]) - min(blocks["ties"])) / ms["ties"],
                       **bm.report_fractions(plans["ties"].report()))
    for name in ("band_linear", "band_ties"):
        rep = plans[name].report()
        res[name].update(density=args.density, gamma=args.gamma, launches=7, ms_vs_ties=ms[name] / ms["ties"],
                         ms_vs_taskvec=ms[name] / ms["taskvec"],
                         outlier_fraction=sum(sum(r["outlier"]) for r in rep) / sum(r["n"] * len(r["outlier"]) for r in rep),
                         **bm.report_fractions(rep))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
