#!/usr/bin/env python
"""Base-size all_moe -> ufo (the inputs tests/test_merge_gpu.py::test_merge_base_size_digests builds) through Iso-C: the whole
isoc_merge -- 48 weight matrices through the fp64 polar iteration in three lock-step groups, 108 other tensors through the
task-vector job, the one read of the verdicts included -- timed on stream events, `--rounds` blocks of `--reps` runs each after
warm-up; the median of the blocks' medians and `spread` = (largest - smallest block median) / median.  `fp64_flop` counts, per
matrix [rows >= cols] and step, the SYRK (rows cols^2), the factorisation (cols^3 / 3) and the two triangular solves (2 rows cols^2);
`launches_estimated` is NOT counted from the run: it mirrors the block-column loops of the drivers in csrc/f64ops.hip as they stand
(cholesky_launches, solve_launches below) and leaves out the few launches torch makes itself (clears, the heads' gather).  For
comparison: torch.linalg.svd on the device over the same 48 float64 task-vector sums, batched per shape (what the rule's definition
would cost).  Prints ONE JSON line; `--out FILE` also writes it to FILE (profiles/isoc_merge_base.json holds such a line).

`--syrk` measures the choice inside a step instead: Z = I + c X^T X for each lock-step group of the base size as the SYRK
(ops.iso_gram) and as a general transposed product (vlm_gemm_f64_batched, ta = 1) over the same operands, one launch each,
alternating blocks, and the largest difference between the two results (profiles/isoc_syrk_vs_gemm.json holds such a line)."""
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

FP64_PEAK_TFLOPS = 78.6  # MI355X matrix fp64


def _blocks(n, big=256):
    for J0 in range(0, n, big):
        yield J0, min(J0 + big, n)


def cholesky_launches(n):
    """vlm_cholesky_f64_batched: per 64-wide block column a left-looking update (not the first of its 256), the block factor, the
    panel solve (not the last column); per 256 columns the trailing update (not the last)."""
    k = 0
    for J0, J1 in _blocks(n):
        for c in range(J0, J1, 64):
            k += (c > J0) + 1 + (min(c + 64, n) < n)
        k += J1 < n
    return k


def solve_launches(n):
    """vlm_solve_spd_right_f64_batched: both sweeps."""
    k = 0
    for J0, J1 in _blocks(n):
        for c in range(J0, J1, 64):
            k += (c > J0) + 1
        k += J1 < n
        for c in range(J0, J1, 64):
            k += (min(c + 64, n) < J1) + 1
        k += J0 > 0
    return k


def step_launches(cols):
    """One step of one lock-step group of at most 64 matrices: the SYRK, the verdicts' memset, factorisation, solve, combine, fold."""
    return 1 + 1 + cholesky_launches(cols) + solve_launches(cols) + 2


def syrk_vs_gemm(reps, rounds):
    L = importlib.import_module("vl_merging_amd._lib")
    ops = importlib.import_module("vl_merging_amd.ops")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "rounds": rounds}
    for rows, cols, count in ((3072, 768, 24), (2304, 768, 12), (768, 768, 12)):
        N = rows * cols
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        buf = torch.zeros(count, L.ISO_HEAD + 3 * N, dtype=torch.float64, device="cuda")
        buf[:, L.ISO_HEAD + N: L.ISO_HEAD + 2 * N] = torch.randn(count, N, dtype=torch.float64, device="cuda", generator=gen) / rows ** 0.5
        work = [buf[i] for i in range(count)]
        xs = [buf[i, L.ISO_HEAD + N: L.ISO_HEAD + 2 * N].view(rows, cols) for i in range(count)]
        z1 = torch.empty(count, cols, cols, dtype=torch.float64, device="cuda")
        z2 = torch.empty_like(z1)
        z1l, z2l = [z1[i] for i in range(count)], [z2[i] for i in range(count)]

        def syrk():
            ops.iso_gram(work, rows, cols, z1l, 1.0, False)

        def gemm():
            L.check(L.get_lib().vlm_gemm_f64_batched(1, 0, cols, cols, rows, 1.0, ops._ptr_list(xs), cols, 0, ops._ptr_list(xs), cols,
                                                     0.0, ops._ptr_list(z2l), cols, count, L.stream_ptr()), "vlm_gemm_f64_batched")
        blocks = {"syrk": [], "gemm": []}
        for _ in range(rounds):
            for name, fn in (("syrk", syrk), ("gemm", gemm)):
                blocks[name].append(bm.timed(fn, reps)[0])
        torch.cuda.synchronize()
        diff = float((z1 - torch.eye(cols, dtype=torch.float64, device="cuda") - z2).abs().max())
        ms = {name: statistics.median(b) for name, b in blocks.items()}
        tiles = -(-cols // 64)
        res["%d of %dx%d" % (count, rows, cols)] = {
            "syrk_ms": ms["syrk"], "gemm_ms": ms["gemm"], "syrk_over_gemm": ms["syrk"] / ms["gemm"], "syrk_blocks": blocks["syrk"],
            "gemm_blocks": blocks["gemm"], "max_abs_diff": diff,
            "syrk_tflops": count * 2.0 * rows * 64 * 64 * (tiles * (tiles + 1) // 2) / ms["syrk"] / 1e9}   # the tiles it computes
    return res


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--syrk", action="store_true", help="measure the SYRK against the general transposed GEMM instead")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--svd-reps", dest="svd_reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    ge.import_package()
    isoc = importlib.import_module("vl_merging_amd.isoc")
    bm = importlib.import_module("vl_merging_amd.bench_merge")
    torch.cuda.set_device(0)
    if args.syrk:
        line = json.dumps(syrk_vs_gemm(2 * args.reps, args.rounds))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return 0
    sd, central, cfg = bm.base_size_task_vector_inputs()
    plans, rows = [], []
    isoc.isoc_merge(sd, cfg, central_weight=central, plan_out=plans, report_out=rows)
    plan = plans[0]
    K = len(plan.schedule)
    flop, launches = 0.0, len(plans) - 1   # the task-vector plan is one launch
    for g in plan.groups:
        r, c = g["shape"]
        chunks = -(-len(g["jobs"]) // 64)
        steps = [rows[j]["steps"] for j in g["jobs"]]
        flop += sum(steps) * (r * c * c + c ** 3 / 3 + 2 * r * c * c)
        shapes = len({tuple(plan.jobs[j][1].shape) for j in g["jobs"]})
        # D (kernel + fold per original shape), the steps, finish (dot, fold, apply per original shape)
        launches += 2 * shapes + max(steps) * chunks * step_launches(c) + 3 * shapes
    blocks, fastest = [], float("inf")
    for _ in range(args.rounds):
        med, lo = bm.timed(lambda: isoc.isoc_merge(sd, cfg, central_weight=central), args.reps, warmup=1)
        blocks.append(med)
        fastest = min(fastest, lo)
    ms = statistics.median(blocks)
    # the definition's cost: one batched SVD per working shape over the same float64 sums
    deltas = [torch.stack([plan.delta(j) for j in g["jobs"]]) for g in plan.groups]
    svd_ms, _ = bm.timed(lambda: [torch.linalg.svd(d, full_matrices=False) for d in deltas], args.svd_reps, warmup=1)
    res = {"workload": "base all_moe -> ufo, 48 matrices + 108 other tensors", "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "rounds": args.rounds, "ms_median": ms, "ms_min": fastest, "ms_blocks": blocks,
           "spread": (max(blocks) - min(blocks)) / ms, "launches_estimated": launches, "scheduled_steps": K,
           "extra_steps": sum(max(0, r["steps"] - K) for r in rows), "matrices": len(rows),
           "groups": [{"shape": list(g["shape"]), "matrices": len(g["jobs"])} for g in plan.groups],
           "converged": all(r["converged"] for r in rows), "last_step_max": max(r["last_step"] for r in rows),
           "fp64_flop": flop, "fp64_tflops": flop / ms / 1e9, "fp64_peak_fraction": flop / ms / 1e9 / FP64_PEAK_TFLOPS,
           "svd_ms_median": svd_ms, "svd_reps": args.svd_reps, "svd_over_isoc": svd_ms / ms}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
