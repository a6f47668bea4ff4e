#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/helpers/merge_inputs.base_size_state builds and
tests/test_merge_gpu.py::test_merge_base_size_digests pins): the DARE merge at drop = 1 - density and the DELLA merge at
density +- epsilon, each in both modes, in ONE process and in alternating blocks: every round times each of the four plans once,
20 stream-timed runs after warm-up, and a plan's figure is the median of its blocks' medians.  A DELLA run moves exactly the bytes
of a DARE run (one pass: 4 (S + 1) B read and 4 B written per element), so DARE in the same mode and the same process is the
yardstick: `ms_vs_dare`, and the effective rate `GBps` over DARE's byte count.  What DELLA adds is the rank of every entry inside
its row, made in LDS.  Prints ONE JSON line.  `--out FILE` also writes it to FILE."""
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
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    merge = importlib.import_module("vl_merging_amd.merge")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()
    plans = {}
    for mode in ("linear", "ties"):
        for name, fn, kw in (("dare_" + mode, merge.dare_merge, dict(drop=1.0 - args.density)),
                             ("della_" + mode, merge.della_merge, dict(density=args.density, epsilon=args.epsilon))):
            got = []
            fn(sd, cfg, central_weight=central, seed=args.seed, mode=mode, plan_out=got, **kw)
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
           "rounds": args.rounds, "density": args.density, "epsilon": args.epsilon, "seed": args.seed}
    for name, plan in plans.items():
        nbytes = plan.bytes_read + plan.bytes_written
        res[name] = {"ms_median": ms[name], "ms_min": fastest[name], "ms_blocks": blocks[name], "bytes": nbytes,
                     "GBps": nbytes / ms[name] / 1e6, "launches": 2, **bm.report_fractions(plan.report())}
    for mode in ("linear", "ties"):
        dare, della = res["dare_" + mode], res["della_" + mode]
        dare["blocks_spread"] = (max(dare["ms_blocks"]) - min(dare["ms_blocks"])) / dare["ms_median"]
        della["ms_vs_dare"] = della["ms_median"] / dare["ms_median"]
        assert della["bytes"] == dare["bytes"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
