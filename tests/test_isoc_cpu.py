"""Iso-C without a GPU: the schedule of the polar iteration, the numpy iteration against the SVD definition of the rule
(isoc_restatement.py), the C ABI and the command line."""
import importlib
import os
import sys

import numpy as np
import pytest

import isoc_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "vl-merging_amd", "merge_ckpt.py")
ISO_SYMBOLS = ("vlm_iso_parts", "vlm_iso_delta", "vlm_iso_gram", "vlm_iso_step", "vlm_iso_finish")


@pytest.fixture(scope="module")
def isoc(pkg):
    return importlib.import_module("vl_merging_amd.isoc")


def test_schedule_matches_the_formulas(isoc):
    got = isoc.iso_schedule()
    want = R.schedule(1e-6, 8)
    assert len(got) == 8 and all(isinstance(v, float) for abc in got for v in abc)
    l0 = np.float64(1e-6)
    d = np.cbrt(4 * (1 - l0 ** 2) / l0 ** 4)
    a = np.sqrt(1 + d) + 0.5 * np.sqrt(8 - 4 * d + 8 * (2 - l0 ** 2) / (l0 ** 2 * np.sqrt(1 + d)))
    c0 = a + (a - 1) ** 2 / 4 - 1
    assert abs(got[0][2] - c0) <= 1e-12 * c0
    for g, w in zip(got, want):
        assert all(abs(x - y) <= 1e-12 * abs(y) for x, y in zip(g, w)), (g, w)
    # the lower bound the coefficients are made for never falls and reaches 1; from there on the step is Halley's
    l, ls = 1e-6, []
    for a, b, c in got:
        ls.append(l)
        l = min(1.0, l * (a + b * l * l) / (1 + c * l * l))
    ls.append(l)
    assert all(y >= x for x, y in zip(ls, ls[1:])) and ls[-1] == 1.0
    first_one = ls.index(1.0)
    assert first_one < 8 and all(abc == (3.0, 1.0, 3.0) for abc in got[first_one:])
    assert got[-1] == (3.0, 1.0, 3.0)
    long = isoc.iso_schedule(steps=20)
    assert long[:8] == got and all(abc == (3.0, 1.0, 3.0) for abc in long[8:])
    assert isoc.iso_schedule(l0=1.0, steps=3) == [(3.0, 1.0, 3.0)] * 3
    for bad in (dict(l0=0.0), dict(l0=1.5), dict(steps=0), dict(l0=float("nan"))):
        with pytest.raises(ValueError):
            isoc.iso_schedule(**bad)


@pytest.mark.parametrize("m,n,S", R.SHAPES)
def test_iteration_meets_the_svd_definition(m, n, S):
    """fp32 outputs of the iteration and of the SVD differ by at most 1 ulp, in at most max(2, 1e-4 n) elements (n = the matrix's
    element count); the polar factors agree and the steps have died out."""
    c, srcs = R.case(m, n, S)
    for lam in (1.0, 0.75):
        want, q, nuc = R.iso_svd(c, srcs, lam)
        got, X, nuc2, norms = R.iso_qdwh(c, srcs, lam)
        u = R.ulp_diff(got, want)
        assert u.max() <= 1 and int((u > 0).sum()) <= max(2, 1e-4 * m * n), (u.max(), int((u > 0).sum()))
        assert abs(nuc - nuc2) <= 1e-13 * nuc
        assert np.abs(X - q).max() <= 1e-10 and norms[-1] <= 1e-10 * np.sqrt(min(m, n))
    if (m, n) == (130, 70):   # the planted zero columns: exact zeros of D, of X and of Q; the output there is c
        assert not R.delta(c, srcs)[:, 5:9].any() and not X[:, 5:9].any() and np.abs(q[:, 5:9]).max() < 1e-15
        assert got[:, 5:9].tobytes() == c[:, 5:9].tobytes()


@pytest.mark.parametrize("m,n,S", R.BOUNDARY_SHAPES)
def test_the_boundary_inputs_are_well_posed(m, n, S):
    """The condition of the GPU suite's rules at the shapes past the kernels' limits (test_isoc_gpu.py), at its lam: the numpy
    iteration alone meets them with room to spare -- its error against the SVD leaves tol = min(1e-8, max(8 err, r eps)) far below
    1e-8, X^T X = I to 1e-14, the last step a hundredth of its bound, and no fp32 output differs from the SVD definition's."""
    c, srcs = R.inputs(m, n, S)
    r = min(m, n)
    want, q, nuc = R.iso_svd(c, srcs, 0.75)
    got, X, nuc2, norms = R.iso_qdwh(c, srcs, 0.75)
    assert np.abs(X - q).max() <= 1e-12 and abs(nuc - nuc2) <= 1e-13 * nuc
    Xw = R.working(X)
    assert np.abs(Xw.T @ Xw - np.eye(r)).max() <= 1e-14
    assert norms[-1] <= 1e-12 * np.sqrt(r)
    assert got.tobytes() == want.tobytes()


def test_restatement_edges():
    c, srcs = R.inputs(16, 32, 2)
    out, X, nuc, norms = R.iso_qdwh(c, [c.copy(), c.copy()], 0.75)          # D = 0: c itself
    assert out.tobytes() == c.tobytes() and nuc == 0.0 and not X.any() and norms == []
    assert R.iso_svd(c, [c.copy()], 1.0)[0].tobytes() == c.tobytes()
    d = R.delta(c, srcs)
    assert d.dtype == np.float64 and d.tobytes() == ((0.0 + (srcs[0].astype("f8") - c)) + (srcs[1].astype("f8") - c)).tobytes()
    assert R.working(d).shape == (32, 16) and R.working(d.T) is not None and R.working(d.T).shape == (32, 16)
    # S = 1: the polar factor of one task vector; lam scales the step, not the factor
    o1 = R.iso_svd(c, srcs[:1], 1.0)
    o2 = R.iso_svd(c, srcs[:1], 0.5)
    assert np.array_equal(o1[1], o2[1]) and o1[2] == o2[2] and not np.array_equal(o1[0], o2[0])
    assert list(R.ulp_diff(np.float32([1.0, -0.0, 1.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0, 1.0]))) == [1, 0, 0]


def test_abi_exports_the_iso_entries(pkg):
    import __graft_entry__ as ge
    L = importlib.import_module("vl_merging_amd._lib")
    if not os.path.exists(L.LIB_PATH):
        ge.build()
    lib = L.get_lib()
    header = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    for s in ISO_SYMBOLS:
        assert hasattr(lib, s) and s in L.SIGNATURES and ("int %s(" % s) in header, s
    assert lib.vlm_abi_version() == 11 and "#define VLM_ABI_VERSION 11" in header
    assert "#define VLM_ISO_HEAD %d\n" % L.ISO_HEAD in header and "#define VLM_ISO_MAX_STEPS %d\n" % L.ISO_MAX_STEPS in header
    # host-side functions of the shape alone (no device is touched)
    assert lib.vlm_iso_parts(16, 16) == 1 and lib.vlm_iso_parts(0, 5) == 0
    assert lib.vlm_iso_parts(64, 33) == 2 and lib.vlm_iso_parts(3072, 768) == 256
    # the boundary shapes cross the limits they are there for: a 65th partial; the cap with more than 2048 elements a workgroup
    assert [lib.vlm_iso_parts(m, n) for m, n, _ in R.BOUNDARY_SHAPES] == [65, 65, 256, 256] and 727 * 723 > 256 * 2048
    isoc = importlib.import_module("vl_merging_amd.isoc")
    assert 8 + isoc.EXTRA_MAX <= L.ISO_MAX_STEPS and 2 + L.ISO_MAX_STEPS <= L.ISO_HEAD
    with pytest.raises(L.VlmError):
        isoc.IsoPlan("cpu")


def test_merge_ckpt_parses_isoc(pkg):
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        mc = importlib.import_module("merge_ckpt")
    finally:
        sys.path.pop(0)
    assert "isoc" in mc.METHODS and mc.METHODS[:12] == ("interp", "taskvec", "ties", "dare", "breadcrumbs", "della", "stock", "sce",
                                                        "slerp", "karcher", "consensus", "emr")
    args, cfg = mc.parse_args(["--method", "isoc", "--ckpt", "a.ckpt", "--out", "b.ckpt", "--central", "c.ckpt", "--lambda", "0.75",
                               "--report", "r.json", "with", "vlffn_start_layer_index=10"])
    assert (args.method, args.central, args.report) == ("isoc", "c.ckpt", "r.json") and cfg["sum_lambda"] == 0.75
    with pytest.raises(ValueError):
        mc.parse_args(["--method", "isoc", "--ckpt", "a", "--out", "b", "--masks-out", "m.pt"])
    assert "--method isoc" in mc.__doc__ and "isoc_merge" in mc.__doc__
