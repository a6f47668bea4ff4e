"""The host part of csrc/chunk_plan.h, the chunk plan merge.hip, ties.hip, dare.hip, pairstats.hip and band.hip share (della.hip: its checks), checked without HIP and without a GPU:
tests/helpers/chunk_plan_check.cpp is compiled with the host compiler under AddressSanitizer + UBSan and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_table_count_cover_and_tail_owner(tmp_path):
    """For the ragged sizes {1, 3, 5, 4095, 4096, 4097, 8195, 12289} and for the 156 tensor lengths of a base-size merge: the
    chunk count, every (job, start4), the chunks of a job cover [0, n4) exactly once, exactly one chunk per job owns the tail,
    and the offsets and bytes of the host image built around the table.  The per-job checks under each overlap policy: equal,
    16-byte offset, adjacent and disjoint ranges, misaligned and null pointers, the length limit and its precedence."""
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
