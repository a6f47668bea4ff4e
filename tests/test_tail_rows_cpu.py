"""Kept rows without a GPU: csrc/attention_keep.h (which query tiles and streamed blocks a per-segment query prefix keeps) as
plain C++ under AddressSanitizer + UBSan against a brute-force walk, and engine.KeepRows (which rows of a segment-major pass a
block evaluation keeps, and how the plan's expert ranges map onto them) against index arithmetic."""
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attention_keep_units_match_brute_force(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "attn_keep_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "vl-merging_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "attn_keep_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "attention keep ok" in r.stdout


@pytest.fixture()
def eng(pkg):
    return importlib.import_module("vl_merging_amd.engine"), importlib.import_module("vl_merging_amd.ops")


def _rows(seq, k0, k1):
    return ([seq.base0 + b * seq.n0 + t for b in range(seq.B) for t in range(k0)]
            + [seq.base1 + b * seq.n1 + i for b in range(seq.B) for i in range(k1)])


@pytest.mark.parametrize("B,n0,n1", [(3, 5, 7), (1, 40, 145), (9, 40, 0), (4, 0, 6)])
def test_keep_rows_are_the_prefix_rows(eng, B, n0, n1):
    import torch
    engine, ops = eng
    seq = ops.Seq(B, n0, n1)
    M = seq.rows
    t = torch.arange(M * 2, dtype=torch.float32).view(M, 2)
    for keep in [(n0, 0), (0, n1), (1, 1), (1, 0), (0, 1), (n0 + 3, 0)]:
        k0, k1 = min(keep[0], n0), min(keep[1], n1)
        kr = engine.KeepRows.of(seq, keep)
        if k0 + k1 == 0:
            assert kr is None
            continue
        served = (k1 == 0 and k0 == n0) or (k0 == 0 and k1 == n1) or (k0 <= 1 and k1 <= 1)
        assert (kr is not None) == served, keep
        want = _rows(seq, k0, k1)
        assert kr.count == len(want) and kr.q == (k0, k1)
        assert kr.take(t)[:, 0].tolist() == [2.0 * r for r in want]
        assert (kr.span is not None) == (want == list(range(want[0], want[0] + len(want))) and (k0 == n0 or k1 == n1) and k0 * k1 == 0)
        # expert ranges in kept-row coordinates: every kept row lands in the range of the expert that owns it
        e0, e1 = object(), object()
        for ranges in ([(0, M, e0)], [r for r in [(0, B * n0, e0), (B * n0, M, e1)] if r[0] < r[1]]):
            got = kr.ranges(ranges)
            owner = [None] * kr.count
            for a, b, e in got:
                for i in range(a, b):
                    assert owner[i] is None
                    owner[i] = e
            assert owner == [next(e for r0, r1, e in ranges if r0 <= r < r1) for r in want]
        if kr.span is not None:
            for r0, r1 in [(0, M), (0, B * n0), (B * n0, M), (1, M - 1)]:
                if r0 >= r1:
                    continue
                pieces = kr.pieces(r0, r1)
                assert [p[0] for p in pieces] + [r1] == [r0] + [p[1] for p in pieces]  # a partition, in order
                for a, b, at in pieces:
                    inside = [r in want for r in range(a, b)]
                    assert all(inside) if at is not None else not any(inside)
                    if at is not None:
                        assert want[at] == a


def test_keep_rows_refuses_other_prefixes(eng):
    engine, ops = eng
    seq = ops.Seq(4, 8, 10)
    for keep in [(3, 0), (8, 1), (2, 2), (0, 5)]:
        assert engine.KeepRows.of(seq, keep) is None
    assert engine.KeepRows.of(seq, (0, 0)) is None
