"""HIP merge kernel (through the C ABI) vs the oracle and the reference's golden vectors: bit-exact."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from test_oracle_merge import CASES, merge_cfg, tiny_state

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from merge_inputs import base_size_state  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def merge(pkg):
    return importlib.import_module("vl_merging_amd.merge")


def to_dev(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sd.items()}


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c][0] != "regmean"])
def test_merge_matches_reference_tiny(case, merge, golden_dir):
    gold = np.load(os.path.join(golden_dir, "merge_tiny.npz"))
    fn, over = CASES[case]
    cfg = merge_cfg(**over)
    sd = to_dev(tiny_state("ufo" if case == "interp_already_ufo" else "all_moe"))
    if fn == "merge_weights":
        res = merge.merge_weights(sd, cfg)
    else:
        res = merge.sum_task_vectors(sd, cfg, central_weight={"state_dict": to_dev(tiny_state("ufo", salt=7))})
    torch.cuda.synchronize()
    keys = json.loads(str(gold[case + "/__keys__"]))
    assert sorted(res.keys()) == keys
    for k in keys:
        if "transformer.blocks." in k and "gamma" not in k:
            assert res[k].cpu().numpy().tobytes() == gold[case + "/" + k].tobytes(), k
        else:
            assert res[k] is sd[k]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4096, 4097, 8191, 12289, 1 << 20])
@pytest.mark.parametrize("mode", ["lerp2", "lerp3", "taskvec3", "mean3", "lerp1"])
def test_merge_ragged_sizes(n, mode, merge):
    """Edge sizes: empty, < one float4, chunk boundaries +-1."""
    if n == 0:
        pytest.skip("empty tensors never reach the kernel (no such key in a checkpoint)")
    L = importlib.import_module("vl_merging_amd._lib")
    rng = np.random.default_rng(n)
    srcs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    srcs[0][: min(n, 2)] = -0.0
    base = rng.standard_normal(n).astype(np.float32)
    plan = merge.MergePlan("cuda")
    d = [torch.from_numpy(s).cuda() for s in srcs]
    if mode == "lerp2":
        out = plan.add(L.MERGE_LERP, d[:2], [0.3, 0.7]); ref = mo.lerp(srcs[:2], [0.3, 0.7])
    elif mode == "lerp3":
        r = [(2 / 3) * 0.3, (2 / 3) * 0.7, 1 / 3]
        out = plan.add(L.MERGE_LERP, d, r); ref = mo.lerp(srcs, r)
    elif mode == "lerp1":
        out = plan.add(L.MERGE_LERP, d[:1], [1]); ref = mo.lerp(srcs[:1], [1])
    elif mode == "taskvec3":
        out = plan.add(L.MERGE_TASKVEC, d, [0.75] * 3, base=torch.from_numpy(base).cuda())
        ref = mo.taskvec(base, srcs, [0.75] * 3)
    else:
        out = plan.add(L.MERGE_MEAN, d, None); ref = mo.mean(srcs)
    plan.run()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == ref.tobytes()


def test_merge_mixed_jobs_in_one_plan(merge):
    """Eight jobs of mixed mode and source count (LERP with 1-4 sources, TASKVEC with 1 and 4, MEAN with 2 and 4) in ONE plan,
    one per size at which tail ownership and the chunk boundary can go wrong; every output bit-equal to the oracle, and a second
    run() of the same plan gives the same bytes."""
    L = importlib.import_module("vl_merging_amd._lib")
    sizes = [1, 3, 5, 4095, 4096, 4097, 8195, 12289]
    kinds = [("lerp", 1), ("lerp", 2), ("lerp", 3), ("lerp", 4), ("taskvec", 1), ("taskvec", 4), ("mean", 2), ("mean", 4)]
    ratios = [0.3, 0.45, 0.15, 0.1]
    plan = merge.MergePlan("cuda")
    outs, refs = [], []
    for k, ((kind, s), n) in enumerate(zip(kinds, sizes[3:] + sizes[:3])):  # the four-source jobs meet 8195, 1 and 5
        rng = np.random.default_rng(100 + k)
        srcs = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
        srcs[0][: min(n, 2)] = -0.0
        base = rng.standard_normal(n).astype(np.float32)
        d = [torch.from_numpy(a).cuda() for a in srcs]
        if kind == "lerp":
            outs.append(plan.add(L.MERGE_LERP, d[:s], ratios[:s])); refs.append(mo.lerp(srcs[:s], ratios[:s]))
        elif kind == "taskvec":
            outs.append(plan.add(L.MERGE_TASKVEC, d[:s], [0.75] * s, base=torch.from_numpy(base).cuda()))
            refs.append(mo.taskvec(base, srcs[:s], [0.75] * s))
        else:
            outs.append(plan.add(L.MERGE_MEAN, d[:s], None)); refs.append(mo.mean(srcs[:s]))
    assert len(plan.jobs) == 8
    plan.run()
    torch.cuda.synchronize()
    first = [o.cpu().numpy().tobytes() for o in outs]
    for k, (got, ref) in enumerate(zip(first, refs)):
        assert got == ref.tobytes(), (kinds[k], len(ref))
    plan.run()
    torch.cuda.synchronize()
    assert [o.cpu().numpy().tobytes() for o in outs] == first


def test_merge_base_size_digests(merge, golden_dir):
    """BASELINE config 4: base-size all_moe -> ufo (1 077 239 808 algorithmic bytes), sha256 == reference."""
    dig = json.load(open(os.path.join(golden_dir, "merge_base_digests.json")))
    sd_np, central_np = base_size_state()
    sd, central = to_dev(sd_np), to_dev(central_np)
    for name, ratio in (("interp_r0.5", 0.5), ("interp_r0.3", 0.3)):
        plans = []
        res = merge.merge_weights(sd, merge_cfg(merge_ratio=ratio), plan_out=plans)
        torch.cuda.synchronize()
        assert plans[0].bytes_read + plans[0].bytes_written == 1077239808
        bad = [k for k, d in dig[name].items() if hashlib.sha256(res[k].cpu().numpy().tobytes()).hexdigest() != d]
        assert not bad, bad[:5]
    res = merge.sum_task_vectors(sd, merge_cfg(sum_lambda=0.75), central_weight=central)
    torch.cuda.synchronize()
    bad = [k for k, d in dig["taskvec_l0.75"].items()
           if hashlib.sha256(res[k].cpu().numpy().tobytes()).hexdigest() != d]
    assert not bad, bad[:5]


def test_merge_properties_full_size(merge):
    """Size-independent properties at full size: merging identical experts is the identity for 2-way r+(1-r)
    only up to rounding, but exactly idempotent for the 1-way case; linearity in the sources for ratio 0.5."""
    n = 7087104
    a = torch.randn(n, device="cuda")
    L = importlib.import_module("vl_merging_amd._lib")
    plan = merge.MergePlan("cuda")
    o1 = plan.add(L.MERGE_LERP, [a], [1])
    o2 = plan.add(L.MERGE_LERP, [a, a], [0.5, 0.5])
    o3 = plan.add(L.MERGE_TASKVEC, [a], [1.0], base=a)
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(o1, a + 0.0)
    assert torch.equal(o2, a + 0.0)  # 0.5a + 0.5a is exact
    assert torch.equal(o3, a)


def test_missing_library_is_loud(pkg, monkeypatch):
    L = importlib.import_module("vl_merging_amd._lib")
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libvlm_hip.so")
    with pytest.raises(L.VlmError):
        L.get_lib()
