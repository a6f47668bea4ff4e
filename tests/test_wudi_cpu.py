"""WUDI without a GPU: the numpy restatement of the rule (wudi_restatement.py) against autograd and torch.optim.Adam on the paper's
loss, the constant of its loss, the C ABI and the command line."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import wudi_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
WUDI_SYMBOLS = ("vlm_wudi_parts", "vlm_wudi_work_doubles", "vlm_wudi_state_offset", "vlm_wudi_prepare", "vlm_wudi_step",
                "vlm_wudi_finish")


def merge_ckpt():
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        return importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)


def test_restatement_is_adam_on_the_papers_loss():
    """Autograd on sum_i sum(square((X - tau_i) @ tau_i^T)) / n_i with torch.optim.Adam(lr=1e-5) in float64, 50 steps."""
    c, srcs = R.inputs(20, 12, 3)
    ref = R.wudi(c, srcs, 1.0, 50)
    ts = [torch.from_numpy(t) for t in R.taus(c, srcs)]
    X = torch.nn.Parameter(sum(ts).clone())
    assert X.detach().numpy().tobytes() == ref["X0"].tobytes()
    opt = torch.optim.Adam([X], lr=1e-5)
    losses = []
    for _ in range(50):
        opt.zero_grad()
        loss = sum(torch.sum(torch.square((X - t) @ t.T)) / torch.sum(t * t) for t in ts)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    diff = float(np.abs(X.detach().numpy() - ref["X"]).max())
    rel = max(abs(a - b) / abs(b) for a, b in zip(ref["losses"], losses))
    print("wudi restatement vs torch Adam: max |diff| %.3e, losses rel %.3e" % (diff, rel))
    assert diff <= 1e-15
    assert rel <= 1e-12
    assert ref["losses"][-1] < ref["losses"][0]


@pytest.mark.parametrize("m,n,S", R.SHAPES)
def test_loss_constant(m, n, S):
    """loss_0 = <X_0, X_0 G - 2 B> + K against L(X_0) from its definition: the constant K."""
    c, srcs = R.case(m, n, S)
    ref = R.wudi(c, srcs, 1.0, 1)
    want = R.loss_by_definition(c, srcs, ref["X0"])
    assert abs(ref["loss_first"] - want) <= 1e-12 * want, (ref["loss_first"], want)
    assert ref["loss_first"] == ref["loss_last"]   # one step: the iterate the last step started from is X_0


@pytest.mark.parametrize("case,iters", R.BOUNDARY_CASES)
def test_the_boundary_inputs_are_well_posed(case, iters):
    """The condition of the GPU suite's rules at the shapes past the kernels' limits (test_wudi_gpu.py): the restatement's two
    summation orders differ by far less than the tolerance made from them, and in no fp32 output."""
    m, n, S = case
    c, srcs = R.inputs(m, n, S)
    a, b = R.wudi(c, srcs, 0.75, iters), R.wudi(c, srcs, 0.75, iters, permute=True)
    x0 = np.abs(a["X0"]).max()
    spread = np.abs(a["X"] - b["X"]).max()
    tol = min(2.0 ** -30 * x0, max(16 * spread, (n + iters) * 2.0 ** -52 * x0))
    assert 16 * spread <= tol and tol == (n + iters) * 2.0 ** -52 * x0   # the rounding term decides, not the spread
    assert a["out"].tobytes() == b["out"].tobytes()
    assert a["loss_last"] < a["loss_first"]


def test_restatement_edges():
    c, srcs = R.inputs(16, 24, 2)
    ref = R.wudi(c, [c.copy(), c.copy()], 0.75, 5)                            # zero task vectors: c itself, nothing NaN
    assert ref["out"].tobytes() == c.tobytes() and not ref["X"].any() and ref["losses"] == [0.0] * 5 and ref["sq"] == [0.0, 0.0]
    a, b = R.wudi(c, srcs, 1.0, 7), R.wudi(c, srcs, 1.0, 7, permute=True)     # the second mode is the same rule
    assert 0 < np.abs(a["X"] - b["X"]).max() <= 1e-12 * np.abs(a["X0"]).max()
    assert a["X0"].tobytes() == ((0.0 + (srcs[0].astype("f8") - c)) + (srcs[1].astype("f8") - c)).tobytes()
    g, gs = R.grid_inputs(8, 8, 2)
    assert all(np.array_equal(t * 1024, np.round(t * 1024)) and np.abs(t).max() < 4 for t in [g] + gs)


def test_abi_exports_the_wudi_entries(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    header = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    for s in WUDI_SYMBOLS:
        assert hasattr(lib, s) and s in L.SIGNATURES and ("%s(" % s) in header, s
    assert sorted(s for s in L.SIGNATURES if s.startswith("vlm_wudi_")) == sorted(WUDI_SYMBOLS)
    assert lib.vlm_abi_version() == 11 and "#define VLM_ABI_VERSION 11" in header
    assert "#define VLM_WUDI_HEAD %d\n" % L.WUDI_HEAD in header
    # host-side functions of the shape alone (no device is touched)
    assert lib.vlm_wudi_work_doubles(3, 2) == L.WUDI_HEAD + 2 * 4 + 5 * 6 and lib.vlm_wudi_work_doubles(0, 2) == 0
    assert lib.vlm_wudi_state_offset(3, 2, 0) == L.WUDI_HEAD + 8 + 6 and lib.vlm_wudi_state_offset(3, 2, 2) == L.WUDI_HEAD + 8 + 6
    assert lib.vlm_wudi_state_offset(3, 2, 301) == L.WUDI_HEAD + 8 + 12
    assert lib.vlm_wudi_parts(64, 64) == 2 + 2 and lib.vlm_wudi_parts(130, 70) == 5 + 2 * 6 and lib.vlm_wudi_parts(0, 1) == 0
    # the boundary shapes cross the limits they are there for: the capped 256 partials and 144 tiles; a 65th partial
    assert [lib.vlm_wudi_parts(*case[:2]) for case, _ in R.BOUNDARY_CASES] == [256 + 2 * 144, 256 + 2 * 144, 65 + 2 * 36]
    wudi = importlib.import_module("vl_merging_amd.wudi")
    with pytest.raises(L.VlmError):
        wudi.WudiPlan("cpu")
    step, bc2s = wudi.adam_scalars(3, 1e-5)
    assert step == 1e-5 / (1.0 - 0.9 ** 3) and bc2s == float(np.sqrt(np.float64(1.0 - 0.999 ** 3)))


def test_merge_ckpt_parses_wudi(pkg):
    mc = merge_ckpt()
    assert mc.METHODS[-1] == "wudi" and mc.METHODS[12] == "isoc"
    args, cfg = mc.parse_args(["--method", "wudi", "--wudi-iters", "40", "--wudi-lr", "2e-5", "--ckpt", "a.ckpt", "--out", "b.ckpt",
                               "--central", "c.ckpt", "--lambda", "0.75", "--report", "r.json", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.wudi_iters, args.wudi_lr, args.central) == ("wudi", 40, 2e-5, "c.ckpt") and cfg["sum_lambda"] == 0.75
    args, _ = mc.parse_args(["--method", "wudi", "--ckpt", "a", "--out", "b"])
    assert (args.wudi_iters, args.wudi_lr) == (300, 1e-5)
    for bad in (["--wudi-iters", "0"], ["--wudi-lr", "0"], ["--wudi-lr", "-1"], ["--masks-out", "m.pt"]):
        with pytest.raises(ValueError):
            mc.parse_args(["--method", "wudi", "--ckpt", "a", "--out", "b"] + bad)
    assert "--method wudi" in mc.__doc__ and "wudi_merge" in mc.__doc__ and ",wudi}" in mc.__doc__
