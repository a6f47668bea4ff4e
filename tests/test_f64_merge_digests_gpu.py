"""Iso-C, WUDI and TSV-M give the bytes, the report values and the launch count they gave before their scaffolding was shared
(matrix_plan.py, csrc/f64_sum.h, csrc/f32_io.h): tests/golden/f64_merge_digests.json was recorded at the commit it names, with
record() below, and is compared for equality.  Per method: the tiny synthetic merge of the *_merge_tiny_* tests (every block
tensor, 48 matrices) and one matrix past a fold limit (65 partials for Iso-C and WUDI, p > 256 for TSV-M's SVD).  A mismatch is a
change of behaviour -- a sum order, a store or a launch moved -- and is found in the diff, never by recording again."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import torch

from test_oracle_merge import merge_cfg, tiny_state
from test_ties_gpu import CASES, to_dev
import isoc_restatement
import tsvm_restatement
import wudi_restatement

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f64_merge_digests.json")
LAM = 0.75
ITERS = 40   # test_wudi_gpu.ITERS
METHODS = ("isoc", "tsvm", "wudi")
# one matrix past a fold limit: isoc_restatement.BOUNDARY_SHAPES[0], tsvm_restatement.BOUNDARY_TALL[0] as a merge of two,
# wudi_restatement.BOUNDARY_CASES[2]
SINGLE = {"isoc": (363, 362, 3), "tsvm": (257, 300, 2), "wudi": (363, 362, 2)}


def hexed(x):
    """A report with every float as float.hex(): equality is equality of bits."""
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {k: hexed(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [hexed(v) for v in x]
    return x


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def tiny(method, mod):
    """The tiny merge: the outputs in key order, the report and, where the plan counts them, its launches."""
    cfg = merge_cfg(sum_lambda=LAM, **CASES["all"])
    sd, central = to_dev(tiny_state("all_moe")), to_dev(tiny_state("ufo", salt=7))
    rows, plans = [], []
    kw = dict(iters=ITERS) if method == "wudi" else {}
    res = getattr(mod, method + "_merge")(sd, cfg, central_weight={"state_dict": central}, report_out=rows, plan_out=plans, **kw)
    torch.cuda.synchronize()
    out = {"keys": len(res), "sha256": sha(res[k] for k in res), "report": hexed(rows)}
    if hasattr(plans[0], "launches"):
        out["launches"] = plans[0].launches
    return out


def single(method, mod):
    """One matrix through the method's plan: its output, the plan's float64 result and its report row."""
    m, n, S = SINGLE[method]
    if method == "isoc":
        (c, srcs), plan, result = isoc_restatement.case(m, n, S), mod.IsoPlan("cuda"), "factor"
    elif method == "wudi":
        (c, srcs), plan, result = wudi_restatement.case(m, n, S), mod.WudiPlan("cuda", iters=ITERS), "state"
    else:
        (c, srcs), plan, result = tsvm_restatement.planted(m, n, S), mod.TsvPlan("cuda"), "task_vector"
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = plan.add([dev(s) for s in srcs], dev(c), lam=LAM, name="0")
    plan.run()
    torch.cuda.synchronize()
    got = {"shape": [m, n, S], "sha256": sha([out, getattr(plan, result)(0)]), "report": hexed(plan.report())}
    if hasattr(plan, "launches"):
        got["launches"] = plan.launches
    return got


def record(commit):
    """What the fixture holds, from the code that is imported: run at the commit to compare against, by hand."""
    out = {"commit": commit}
    for method in METHODS:
        mod = importlib.import_module("vl_merging_amd." + method)
        out[method] = {"tiny": tiny(method, mod), "single": single(method, mod)}
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("which", ["tiny", "single"])
@pytest.mark.parametrize("method", METHODS)
def test_same_bytes_report_and_launches_as_recorded(method, which, recorded, pkg):
    mod = importlib.import_module("vl_merging_amd." + method)
    got = json.loads(json.dumps({"tiny": tiny, "single": single}[which](method, mod)))
    want = recorded[method][which]
    assert len(recorded["commit"]) == 40
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (method, which, key)
