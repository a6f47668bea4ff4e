#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds) through WUDI: the whole
wudi_merge -- 48 weight matrices through `--iters` Adam steps in four lock-step groups, one launch per group and step, 108 other
tensors through the task-vector job, the one read of the heads included -- timed on stream events, `--rounds` blocks of `--reps`
runs each after warm-up; the median of the blocks' medians and `spread` = (largest - smallest block median) / median.  `fp64_flop`
counts the steps' products alone: 2 m n^2 per matrix [m, n] and step (the setup, about 1 / 300 of that at the default step count,
is in the time and not in the count).

For comparison, on the same device and the same G, B and X_0 (the plan's own setup, read back): the same explicit loop in torch
float64 -- per lock-step group one batched `X @ G - B` (rocBLAS) and the elementwise Adam update in torch.optim.Adam's in-place
operations -- timed the same way over the `iters` steps alone (`torch_ms_median`; its setup is NOT in it), how far its X_T lies
from the kernels' (`torch_max_abs_diff`), and that loop's products alone, `iters` times `X_0 @ G - B` per group with no update
(`torch_products_ms_median`: what rocBLAS takes for the flops the step kernel's 64 x 64 tiles do).  Prints ONE JSON line; `--out FILE` also writes it to FILE (profiles/wudi_merge_base.json
holds such a line)."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

FP64_PEAK_TFLOPS = 78.6  # MI355X matrix fp64


def torch_groups(plan):
    """Per lock-step group of the plan the stacked float64 (G, B, X_0) of its matrices, made with torch in the rule's order."""
    out = []
    for g in plan.groups:
        Gs, Bs, Xs = [], [], []
        for j in g["jobs"]:
            _, base, srcs, _, _ = plan.jobs[j]
            taus = [s.double() - base.double() for s in srcs]
            G = torch.zeros(base.shape[1], base.shape[1], dtype=torch.float64, device=base.device)
            B = torch.zeros_like(taus[0])
            X = torch.zeros_like(taus[0])
            for t in taus:
                sq = (t * t).sum()
                Gi = (t.T @ t) * torch.where(sq > 0, 1.0 / sq, torch.zeros_like(sq))
                G, B, X = G + Gi, B + t @ Gi, X + t
            Gs.append(G), Bs.append(B), Xs.append(X)
        out.append((torch.stack(Gs), torch.stack(Bs), torch.stack(Xs)))
    return out


def torch_loop(groups, iters, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The rule's step 4 on every group, batched per group: X @ G - B, then Adam as torch.optim.Adam's single-tensor path writes it."""
    finals = []
    for G, B, X0 in groups:
        X, M, V = X0.clone(), torch.zeros_like(X0), torch.zeros_like(X0)
        for t in range(1, iters + 1):
            g = torch.baddbmm(B, X, G, beta=-1.0).mul_(2.0)
            M.mul_(beta1).add_(g, alpha=1.0 - beta1)
            V.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
            denom = (V.sqrt() / math.sqrt(1.0 - beta2 ** t)).add_(eps)
            X.addcdiv_(M, denom, value=-lr / (1.0 - beta1 ** t))
        finals.append(X)
    return finals


def torch_products(groups, iters):
    """The loop's products alone: `iters` times X_0 @ G - B per group, nothing else."""
    for G, B, X0 in groups:
        for _ in range(iters):
            torch.baddbmm(B, X0, G, beta=-1.0)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-reps", dest="torch_reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    wudi =importlib.import_module("vl_merging_amd.wudi")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    sd, central, cfg = bm.base_size_task_vector_inputs()

    def merge(**kw):
        return wudi.wudi_merge(sd, cfg, central_weight=central, iters=args.iters, lr=args.lr, **kw)
    plans, rows = [], []
    merge(plan_out=plans, report_out=rows)
    plan = plans[0]
    flop = float(sum(args.iters * 2.0 * r["shape"][0] * r["shape"][1] ** 2 for r in rows))
    launches = len(plans) - 1   # the task-vector plan is one launch; per group: 6 S + 1 setup and 2 output launches per source
    for g in plan.groups:      # count S among its matrices, one launch per step (the base size has no group above 64 matrices)
        launches += args.iters * -(-len(g["jobs"]) // 64) + sum(6 * S + 1 + 2 for S in {len(plan.jobs[j][2]) for j in g["jobs"]})
    blocks, fastest = [], float("inf")
    for _ in range(args.rounds):
        med, lo = bm.timed(merge, args.reps, warmup=1)
        blocks.append(med)
        fastest = min(fastest, lo)
    ms = statistics.median(blocks)
    groups = torch_groups(plan)
    finals = torch_loop(groups, args.iters, args.lr)
    torch.cuda.synchronize()
    diff = max(float((torch.stack([plan.state(j) for j in g["jobs"]]) - X).abs().max()) for g, X in zip(plan.groups, finals))
    del finals
    tblocks = [bm.timed(lambda: torch_loop(groups, args.iters, args.lr), args.torch_reps, warmup=1)[0] for _ in range(args.rounds)]
    tms = statistics.median(tblocks)
    pblocks = [bm.timed(lambda: torch_products(groups, args.iters), args.torch_reps, warmup=1)[0] for _ in range(args.rounds)]
    pms = statistics.median(pblocks)
    res = {"workload": "base all_moe -> ufo, 48 matrices + 108 other tensors", "device": torch.cuda.get_device_name(0),
           "iters": args.iters, "lr": args.lr, "reps": args.reps, "rounds": args.rounds, "ms_median": ms, "ms_min": fastest,
           "ms_blocks": blocks, "spread": (max(blocks) - min(blocks)) / ms, "ms_per_step": ms / args.iters,
           "launches_estimated": launches, "matrices": len(rows),
           "groups": [{"shape": list(g["shape"]), "matrices": len(g["jobs"])} for g in plan.groups],
           "loss_first_sum": sum(r["loss_first"] for r in rows), "loss_last_sum": sum(r["loss_last"] for r in rows),
           "fp64_flop": flop, "fp64_tflops": flop / ms / 1e9, "fp64_peak_fraction": flop / ms / 1e9 / FP64_PEAK_TFLOPS,
           "torch_ms_median": tms, "torch_ms_blocks": tblocks, "torch_reps": args.torch_reps,
           "torch_spread": (max(tblocks) - min(tblocks)) / tms, "torch_fp64_tflops": flop / tms / 1e9,
           "torch_over_wudi": tms / ms, "torch_max_abs_diff": diff,
           "torch_products_ms_median": pms, "torch_products_ms_blocks": pblocks, "torch_products_fp64_tflops": flop / pms / 1e9}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
