"""csrc/wgrad_plan.h, the slice plan shared by vlm_gemm_wgrad_batch and vlm_gemm_wgrad_grouped, checked without HIP and without a
GPU: tests/helpers/wgrad_plan_check.cpp is compiled with the host compiler under AddressSanitizer + UBSan and run as a child
process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_plan_cover_budget_and_workspace(tmp_path):
    """The base block (36, 36, 9, 27 tiles) at T = 54 296 and 13 574, one to four problems of 1..36 tiles, T from 33 to 60 000 and CU
    budgets 256 / 248 / 128 / 64: every (problem, tile, K step) belongs to exactly one item, items <= budget, kps even and >= 4,
    the problems' workspace blocks are disjoint and sum to the total, refusal when the tiles exceed the budget or the workspace is
    one float short; and the row-range form keeps the slice counts of the rule vlm_gemm_wgrad_grouped had before."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "wgrad_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "wgrad_plan_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "wgrad plan ok" in r.stdout
