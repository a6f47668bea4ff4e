"""The four weight gradients of a base-width block (fc2, fc1, proj, qkv) alone on the chip: four plain wgrad calls (each with its
reduce launch) against one ops.gemm_wgrad_batch, at the token counts of the flagship step's two passes (T = 54 296 and 13 574).
Median of 20 device-event timings after 3 warm-ups; one JSON file (default profiles/wgrad_batch_harness.json).

Alone on the chip the batch may lose at T = 54 296: it fills 216 of 256 CUs, the plain calls 243-252.  What it saves -- workspace bytes
and CU-time -- pays on the side stream, next to the main stream's kernels; the step A/B is the figure that counts."""
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
ops = importlib.import_module("vl_merging_amd.ops")
L = importlib.import_module("vl_merging_amd._lib")

D, F = 768, 3072
SHAPES = [("fc2", D, F), ("fc1", F, D), ("proj", D, D), ("qkv", 3 * D, D)]  # dW [M, N] = dy[T, M]^T x[T, N]


def median_us(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wgrad_batch_harness.json")
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "cus": L.get_lib().vlm_device_cus(), "method": "median of 20 device-event timings after 3 warm-ups, us",
           "cases": []}
    for T in (54296, 13574):
        probs = []
        for _, M, N in SHAPES:
            dy = torch.randn(T, M, device="cuda", generator=gen).to(torch.bfloat16)
            x = torch.randn(T, N, device="cuda", generator=gen).to(torch.bfloat16)
            probs.append((dy, x, torch.zeros(M, N, device="cuda")))

        def plain():
            for dy, x, w in probs:
                ops.gemm(dy, x, w, ta=True, tb=True, accumulate=True)

        def batch():
            ops.gemm_wgrad_batch(probs)

        assert ops.wgrad_batch_serves(T, [(M, N) for _, M, N in SHAPES])
        # same sums, other order: the two forms agree to the wgrad tolerance
        for _, _, w in probs:
            w.zero_()
        plain()
        a = [w.clone() for _, _, w in probs]
        for _, _, w in probs:
            w.zero_()
        batch()
        err = max(float((w - r).abs().max()) for (_, _, w), r in zip(probs, a))
        p, b = median_us(plain), median_us(batch)
        per = {name: median_us(lambda dy=dy, x=x, w=w: ops.gemm(dy, x, w, ta=True, tb=True, accumulate=True))[0]
               for (name, _, _), (dy, x, w) in zip(SHAPES, probs)}
        case = {"T": T, "plain_4_calls_us": {"median": p[0], "min": p[1], "max": p[2]}, "plain_each_us": per,
                "batch_1_call_us": {"median": b[0], "min": b[1], "max": b[2]}, "batch_over_plain": b[0] / p[0],
                "max_abs_diff_batch_vs_plain": err}
        res["cases"].append(case)
        print(json.dumps(case))
        del probs
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
