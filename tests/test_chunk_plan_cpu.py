"""The host part of csrc/chunk_plan.h -- the chunk plan the merge family shares (della.hip: its checks and its run), the counter plan of
dare.hip and tall.hip, the record plan of pairstats.hip and stock.hip (sphere.hip: its parts) and chunk_first_fill -- checked without HIP and without a GPU:
tests/helpers/chunk_plan_check.cpp is compiled with the host compiler under AddressSanitizer + UBSan and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_table_count_cover_and_tail_owner(tmp_path):
    """For the ragged sizes {1, 3, 5, 4095, 4096, 4097, 8195, 12289} and for the 156 tensor lengths of a base-size merge: the
    chunk count, every (job, start4), the chunks of a job cover [0, n4) exactly once, exactly one chunk per job owns the tail,
    and the offsets and bytes of the host image built around the table.  The per-job checks under each overlap policy: equal,
    16-byte offset, adjacent and disjoint ranges, misaligned and null pointers, the length limit and its precedence.  What the
    methods share whole, for both sets of lengths: chunk_first_fill (every first[i], the count, a plan some of whose jobs have no
    chunks), chunk_jobs_check's precedence, and the counter and record layouts -- 256-aligned offsets, disjoint parts in the order
    taken, totals equal to the formulas the methods' own layout functions had."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "chunk_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "chunk_plan_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "chunk plan ok" in r.stdout
