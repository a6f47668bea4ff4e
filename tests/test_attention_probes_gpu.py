"""The attention kernels on the probes of tests/helpers/attn_probes.py, against its float64 reference and derived bounds tau.

Every case runs one forward and one backward, compares out, lse, dQ, dK, dV, the four column sums and the bias-table gradient
entry by entry with tau, prints the largest err / tau per output and asserts that none exceeds 1.  Where tau is 0 (a dQ row
outside a kept prefix, the dqkv rows of a dead sample, dK with Q = 0) the kernel's value must be exactly 0.  No tolerance is
stated here: all of them come from the helper, and tests/test_attention_probes_cpu.py shows what they can see.

Plans (JOINT mode), rechecked against att_handplaced_covers (attention_common.h:142: a dense bias, no image keep mask,
pos1 <= 64) and dkvb_lds_bytes (attention_bwd_dkvb.h:428: ceil(NP / 32) * 4096 + max(W * 8192, 8 R + 16) <= 163 840):
  G1 185 -> 6 blocks, G2 128 -> 4, G3 135 -> 5, G5 130 -> 5, G6 40 -> 2: hand-placed forward / dQ, W = 8
  G4 pos1 = 72 > 64: generic forward / dQ; 137 -> 5 blocks, W = 8
  G7 768 -> 24 blocks: 98 304 + 65 536 = 163 840, W = 8;  G8 769 -> 25: 102 400 + 65 536 > limit, + 32 768 fits: W = 4
  G9 1 024 -> 32 blocks: 131 072 + 32 768 = 163 840, W = 4;  G10 1 025 -> 33: 135 168 + 32 768 > limit: the fallback pair
  G11 R = 8 191: 8 R + 16 = 65 544 > 65 536; 736 -> 23 blocks: 94 208 + 65 544 = 159 752, W = 8
  G12 768 -> 24 blocks: 98 304 + 65 544 = 163 848 > limit for W = 8 and for W = 4 (the histogram is the larger tail): fallback
In SEPARATE mode the panel is the larger PART's (ceil(max(n0, n1) / 32) blocks), so G10 (31 blocks, W = 4) and G12 (23 blocks,
W = 8) run the fused kernel there; `plan` restates the two rules and every case asserts what the ABI shows of them."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_probes as ap  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER = sorted(ap.GEOMS, key=lambda g: int(g[1:]))
# JOINT mode: (hand-placed forward / dQ, waves of the fused dK / dV / bias-gradient kernel or 0 = the fallback pair)
JOINT_PLANS = {"G1": (True, 8), "G2": (True, 8), "G3": (True, 8), "G4": (False, 8), "G5": (True, 8), "G6": (True, 8), "G7": (True, 8),
               "G8": (True, 4), "G9": (True, 4), "G10": (True, 0), "G11": (True, 8), "G12": (True, 0)}


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("vl_merging_amd.ops")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("vl_merging_amd._lib")


def plan(c, sep):
    """(hand-placed, W) by the two rules of the module docstring."""
    hand = c.with_bias and c.keep1 is None and c.pos1 <= 64
    blocks = max((c.n0 + 31) // 32, (c.n1 + 31) // 32) if sep else (c.NP + 31) // 32
    W = 0
    for w in (8, 4):
        if c.with_bias and not W and blocks * 4096 + max(w * 8192, 8 * c.R + 16) <= 160 * 1024:
            W = w
    return hand, W


_REF = {}


def reference(key, c, qkv, dout_counted, sep):
    """One float64 reference per case, kept for the module (the parametrised cases do not share gradients: dO differs).  It is
    computed on the HOST, where tests/test_attention_probes_cpu.py has checked it: a reference must not depend on the card
    under test (docs/experiments.md)."""
    if key not in _REF:
        host = ap.Case(c.gid, device="cpu", with_bias=c.with_bias, image_mask=c.keep1 is not None, sharp=c.sharp)
        ref = ap.reference_with_bounds(host, qkv.cpu(), dout_counted.cpu(), sep)
        tau = {k: v.cuda() for k, v in ref.pop("tau").items()}
        _REF[key] = {k: v.cuda() for k, v in ref.items() if torch.is_tensor(v)}
        _REF[key]["tau"] = tau
    return _REF[key]


def run_case(ops, L, gid, probe, sep, *, with_bias=True, image_mask=False, q_keep=None, dead=False):
    c = ap.case_for(gid, probe, device="cuda", with_bias=with_bias, image_mask=image_mask)
    qkv, dout = ap.probe_inputs(c, probe, sep)
    seq = ops.Seq(c.B, c.n0, c.n1)
    assert seq.pos1 == c.pos1 and seq.rows == c.rows
    H, D, rows = c.H, c.D, c.rows
    mode = L.ATTN_SEPARATE if sep else L.ATTN_JOINT
    kw = dict(keep0=c.keep0, keep1=c.keep1, mode=mode)
    bias_t = None
    if with_bias:
        bias_t = c.table.t().contiguous()
        idx4 = (c.idx * 4).contiguous()
        idx_t = torch.zeros_like(idx4)
        idx_t[:, :c.NP] = idx4[:, :c.NP].t()
        kw.update(bias_t=bias_t, head_row0=ap.LAYER * H, rel_index=idx4, rel_index_t=idx_t,
                  bias_dense=ops.bias_dense(bias_t, idx4, seq, mode))      # ops.attention_fwd's own path, built once per case
    # ---- what the ABI shows of the plan ----
    hand, W = plan(c, sep)
    if not sep and with_bias and not image_mask:
        assert (hand, W) == JOINT_PLANS[gid]
    served = ops.attention_qkeep_served(qkv, seq, H, **kw)
    assert served == (W != 0)
    desc = ops._attn_desc(qkv, seq, H, bias_t, kw.get("head_row0", 0), kw.get("rel_index"), kw.get("rel_index_t"), c.keep0, c.keep1, mode,
                          0.125, kw.get("bias_dense"))
    ws = L.get_lib().vlm_attention_bwd_ws_floats(ctypes.byref(desc), 0)
    assert ws == (H * rows if (W or not with_bias) else 3 * H * rows)
    # ---- the gradient that counts ----
    counted = torch.ones(rows, dtype=torch.bool, device="cuda")
    kept = None
    if q_keep is not None:
        q_keep = (c.n0 if q_keep[0] is None else q_keep[0], q_keep[1])
        kept = c.kept_rows(q_keep)
        counted &= kept
    live = None
    if dead:  # sample 1: both segments in JOINT mode (one draw), its text segment in SEPARATE mode
        dead_rows = c.sample_rows(1, (0,) if sep else (0, 1))
        counted &= ~dead_rows
        live = torch.full((rows,), 1.0 / 0.9, device="cuda")
        live[dead_rows] = 0.0
    do_counted = torch.where(counted[:, None], dout, torch.zeros_like(dout))
    ref = reference((gid, probe, sep, with_bias, image_mask, q_keep, dead), c, qkv, do_counted, sep)
    # ---- the kernels ----
    out = torch.full((rows, D), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full((H, rows), float("nan"), device="cuda")
    do_gpu = do_counted.clone()
    limit = q_keep if (q_keep is not None and served) else None
    if limit is not None:
        do_gpu[~kept] = float("nan")        # honoured limit: rows outside the prefixes are not read
    # (a plan that ignores the limit reads every row: its forward runs unlimited and dO holds zeros there, include/vlm_hip.h)
    ops.attention_fwd(qkv, out, lse, seq, H, q_keep=limit, **kw)
    dqkv = torch.full((rows, 3 * D), float("nan"), device="cuda", dtype=torch.bfloat16)
    dbias_t = torch.zeros_like(bias_t) if with_bias else None
    # (zeros: tests/test_attention_gpu.py checks that the sums are ADDED to what is there; a start value's own fp32 rounding
    # would need a term of its own in tau)
    csq = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
    csv = [torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")]
    ops.attention_bwd(qkv, out, do_gpu, lse, dqkv, seq, H, dbias_t=dbias_t, dq_colsum=csq, dv_colsum=csv, row_live=live, q_keep=q_keep, **kw)
    torch.cuda.synchronize()
    got = dict(out=out, lse=lse, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:],
               csq=torch.stack(csq), csv=torch.stack(csv))
    if with_bias:
        got["dbias"] = dbias_t[ap.LAYER * H:(ap.LAYER + 1) * H]
        assert float(dbias_t[:H].abs().max()) == 0.0       # the other layer's rows untouched
    ratios = ap.worst_ratio(got, ref, rows=kept if limit is not None else None)
    print("probe-ratio %s %s %s%s%s%s%s | plan %s W=%d | %s" % (
        gid, "SEPARATE" if sep else "JOINT", probe, "" if with_bias else " nobias", " keep1" if image_mask else "",
        " q_keep=%s" % (q_keep,) if q_keep else "", " dead" if dead else "", "hand" if hand else "generic", W,
        " ".join("%s=%.3f" % (k, v) for k, v in ratios.items())))
    if limit is not None:   # rows of tiles that hold no kept position were not written (a launched tile writes all its rows)
        assert not bool(torch.isnan(out[kept].float()).any()) and not bool(torch.isnan(lse[:, kept]).any())
    assert sorted(ratios) == sorted(n for n in ap.OUTPUTS if n != "dbias" or with_bias)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
    return ratios


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("gid", ORDER)
def test_probe(ops, L, gid, sep, probe):
    run_case(ops, L, gid, probe, sep)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
def test_probe_with_an_image_keep_mask(ops, L, sep, probe):
    """keep1 at a hand-placed geometry: the generic forward and dQ kernels."""
    run_case(ops, L, "G1", probe, sep, image_mask=True)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("q_keep", [(None, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("gid", ["G1", "G4"])
def test_probe_with_kept_query_prefixes(ops, L, gid, q_keep, sep, probe):
    """q_keep = (n0, 0), (1, 1), (1, 0): dO outside the prefixes is NaN, out / lse start as NaN; dQ outside must be exactly 0."""
    run_case(ops, L, gid, probe, sep, q_keep=q_keep)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("q_keep", [None, (None, 0)])
def test_probe_with_a_dead_sample(ops, L, q_keep, sep, probe):
    """row_live with sample 1 dead, alone and together with the text prefix: its dqkv rows must be exactly 0."""
    run_case(ops, L, "G1", probe, sep, q_keep=q_keep, dead=True)


@pytest.mark.parametrize("probe", ap.PROBES)
@pytest.mark.parametrize("sep", [False, True])
def test_probe_with_a_prefix_the_plan_may_ignore(ops, L, sep, probe):
    """G10: in JOINT mode no panel fits, attention_qkeep_served is 0 (asserted in run_case against the plan rule), the forward
    runs unlimited and dO holds zeros outside the prefix; in SEPARATE mode the image part's 31 blocks fit and the limit is served."""
    run_case(ops, L, "G10", probe, sep, q_keep=(None, 0))


@pytest.mark.parametrize("probe", ["F", "BV"])
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("gid", ["G1", "G4", "G5"])
def test_probe_without_a_bias(ops, L, gid, sep, probe):
    """bias_t = None: the scores are all zero, P is uniform over the kept keys (the HAS_BIAS == false kernels)."""
    run_case(ops, L, gid, probe, sep, with_bias=False)
