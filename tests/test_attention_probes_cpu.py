"""Power check of the attention probes (tests/helpers/attn_probes.py), on the CPU: before any kernel runs, the probe inputs and
the derived bounds tau must be able to SEE the errors a kernel could make.  For every geometry, mode and probe the clean float64
evaluation is within tau of itself and of the autograd reference (1e-12), and every mutation -- applied to the evaluation, never
to a kernel -- moves at least one compared entry beyond POWER = 4 tau.  The factor is a condition on the inputs: a case that
misses it has the wrong inputs (denser or sparser integers, a sharper table), not the wrong factor."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_probes as ap  # noqa: E402

SMALL = ("G1", "G2", "G3", "G4", "G5", "G6")
_CACHE = {}


@pytest.fixture(autouse=True, scope="module")
def few_threads():
    """float64 products of matrices this small get slower with many threads (minutes instead of seconds on a small host)."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


def clean(gid, sep, probe, with_bias=True):
    key = (gid, sep, probe, with_bias)
    if key not in _CACHE:
        c = ap.case_for(gid, probe, with_bias=with_bias)
        qkv, dout = ap.probe_inputs(c, probe, sep)
        _CACHE[key] = (c, qkv, dout, ap.evaluate(c, qkv, dout, sep))
    return _CACHE[key]


def test_geometries_are_the_pinned_ones():
    assert ap.GEOMS == {"G1": (9, 40, 145, 2, 300), "G2": (3, 64, 64, 1, 300), "G3": (3, 57, 71, 1, 300), "G4": (3, 72, 65, 2, 300),
                        "G5": (2, 0, 130, 1, 300), "G6": (3, 40, 0, 1, 300), "G7": (2, 40, 728, 1, 300), "G8": (2, 40, 729, 1, 300),
                        "G9": (2, 40, 984, 1, 300), "G10": (2, 40, 985, 1, 300), "G11": (2, 40, 696, 1, 8191),
                        "G12": (2, 40, 728, 1, 8191)}
    assert ap.U == 2.0 ** -9 and ap.POWER == 4.0
    for gid, NP in (("G1", 185), ("G2", 128), ("G3", 135), ("G4", 137), ("G7", 768), ("G8", 769), ("G9", 1024), ("G10", 1025),
                    ("G11", 736), ("G12", 768)):
        assert ap.Case(gid).NP == NP


def test_probe_inputs_are_exact_in_bf16_and_coded():
    for probe in ap.PROBES:
        c = ap.case_for("G3", probe)
        qkv, dout = ap.probe_inputs(c, probe, False)
        q, k, v = (c.heads(qkv[:, i * c.D:(i + 1) * c.D].double()) for i in range(3))
        cd = ap.code(c.pos).double()
        coded = dict(F=v, BV=c.heads(dout.double()), BQ=k, BK=q, T=k)[probe]
        assert torch.equal(coded, cd[None, None].expand_as(coded))
        assert float((q @ k.transpose(-1, -2)).abs().max()) == 0.0          # the scores are the bias alone
        if probe != "F":
            assert torch.equal(qkv.double(), qkv.double().round()) and float(qkv.double().abs().max()) <= 3
    assert float(cd[57].argmax()) == 0 and float(cd[56].argmax()) == 56     # slot 57 = position 64 (the gap is skipped)


@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("gid", SMALL)
@pytest.mark.parametrize("with_bias", [True, False])
def test_written_out_evaluation_is_the_autograd_reference(gid, sep, with_bias):
    for probe in ap.PROBES:
        c, qkv, dout, ev = clean(gid, sep, probe, with_bias)
        ref = ap.reference(c, qkv, dout, sep)
        D = c.D
        pairs = [(ev["out"], ref["out"]), (ev["lse"], ref["lse"]), (ev["dq"], ref["dqkv"][:, :D]), (ev["dk"], ref["dqkv"][:, D:2 * D]),
                 (ev["dv"], ref["dqkv"][:, 2 * D:])]
        if with_bias:
            pairs.append((ev["dbias"], ref["dbias"]))
        for a, b in pairs:
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def power(gid, sep, probe):
    c, qkv, dout, ev = clean(gid, sep, probe)
    assert all(v <= 1.0 for v in ap.worst_ratio(ev, ev).values())            # (trivially)
    assert all(bool(torch.isfinite(ev[n]).all()) for n in ap.OUTPUTS)
    # (f), one pair left out of its table bin, is stated on the sparse probe T alone (the helper's docstring says why)
    muts = [(name, m) for name, m in ap.mutations(c, sep) if probe == "T" or not name.startswith("f ")]
    kinds = {name.split(":")[0].split(" ")[0] for name, _ in muts}
    want = {"a", "b", "c", "e"} | ({"f"} if probe == "T" else set()) | ({"d"} if c.n0 else set())
    if probe in ("BQ", "BK"):   # every pair reaches dQ / dK / its bin: no query row has dS identically 0
        assert ev["zero_dS_rows"] == 0
    assert kinds == want, (kinds, want)
    missed = []
    for name, mut in muts:
        ratio, where = ap.exceeds(ap.evaluate(c, qkv, dout, sep, mut=mut, bounds=False), ev)
        if not ratio > ap.POWER:
            missed.append((name, round(ratio, 3), where))
    assert not missed, missed


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("gid", sorted(ap.GEOMS, key=lambda g: int(g[1:])))
def test_every_mutation_exceeds_four_tau(gid, sep, probe):
    power(gid, sep, probe)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("q_keep", [(None, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("gid", ["G1", "G4"])
def test_a_prefix_longer_by_one_exceeds_four_tau(gid, q_keep, sep, probe):
    """(g): the reference of a kept-row call has dO zero outside the prefixes; a kernel that takes one more row is caught."""
    c, qkv, dout, _ = clean(gid, sep, probe)
    q_keep = (c.n0 if q_keep[0] is None else q_keep[0], q_keep[1])
    kept, longer = c.kept_rows(q_keep), ap.prefix_longer(c, q_keep)
    assert int(longer.sum()) == int(kept.sum()) + c.B
    zero = torch.zeros_like(dout)
    ref = ap.evaluate(c, qkv, torch.where(kept[:, None], dout, zero), sep)
    assert float(ref["dq"][~kept].abs().max()) == 0.0 and float(ref["tau"]["dq"][~kept].abs().max()) == 0.0
    ratio, where = ap.exceeds(ap.evaluate(c, qkv, torch.where(longer[:, None], dout, zero), sep, bounds=False), ref)
    assert ratio > ap.POWER, (ratio, where)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
def test_a_dead_sample_computed_as_live_exceeds_four_tau(sep, probe):
    """(h): sample 1 is dead (JOINT: both segments, SEPARATE: its text segment); its dqkv rows are 0 with a bound of 0."""
    c, qkv, dout, _ = clean("G1", sep, probe)
    dead = c.sample_rows(1, (0,) if sep else (0, 1))
    ref = ap.evaluate(c, qkv, torch.where(dead[:, None], torch.zeros_like(dout), dout), sep)
    assert float(ref["dq"][dead].abs().max()) == 0.0 and float(ref["tau"]["dq"][dead].abs().max()) == 0.0
    ratio, where = ap.exceeds(ap.evaluate(c, qkv, dout, sep, bounds=False), ref)
    assert ratio > ap.POWER, (ratio, where)
