"""matrix_plan.py without a GPU: the cut of a list of matrices into kernel-argument tables (batches), and the messages of the plan
that Iso-C, WUDI and TSV-M share (MatrixPlan.add, report, the refusal of a device that is not a GPU), word for word what each
method's own copy said."""
import importlib

import pytest
import torch

NAMES = {"isoc": ("IsoPlan", "an Iso-C", "Iso-C"), "wudi": ("WudiPlan", "a WUDI", "WUDI"), "tsvm": ("TsvPlan", "a TSV-M", "SVD")}
COUNTS = (0, 1, 64, 65, 129)


@pytest.fixture(scope="module")
def mp(pkg):
    return importlib.import_module("vl_merging_amd.matrix_plan")


@pytest.mark.parametrize("n", COUNTS)
def test_batches_of_one_key(n, mp):
    ops = importlib.import_module("vl_merging_amd.ops")
    assert ops.F64_MAX_BATCH == 64
    ids = [3 * i + 1 for i in range(n)]
    for got in (list(mp.batches(ids)), list(mp.batches(iter(ids), key=lambda i: "k"))):
        assert [len(part) for _, part in got] == [64] * (n // 64) + [n % 64] * (n % 64 > 0)
        assert {k for k, _ in got} <= {None, "k"} and len({k for k, _ in got}) <= 1
        assert [i for _, part in got for i in part] == ids          # the given order, every id exactly once


@pytest.mark.parametrize("n", COUNTS)
def test_batches_of_two_interleaved_keys(n, mp):
    ids = list(range(100, 100 + n))
    got = list(mp.batches(ids, key=lambda i: ("b", 2) if i % 2 == 0 else ("a", 10)))   # `a` sorts first, its ids are the odd ones
    odd, even = [i for i in ids if i % 2], [i for i in ids if i % 2 == 0]
    want = []
    for key, js in ((("a", 10), odd), (("b", 2), even)):
        want += [(key, js[i0:i0 + 64]) for i0 in range(0, len(js), 64)]
    assert got == want
    assert all(1 <= len(part) <= 64 for _, part in got)
    assert [k for k, _ in got] == sorted(k for k, _ in got)          # keys in sorted order, a key's parts together
    assert sorted(i for _, part in got for i in part) == ids         # every id exactly once
    for key in {k for k, _ in got}:
        mine = [i for k, part in got if k == key for i in part]
        assert mine == sorted(mine)                                  # the given order within a key


@pytest.mark.parametrize("method", sorted(NAMES))
def test_plan_messages_are_each_method_s_own(method, mp, pkg):
    L = importlib.import_module("vl_merging_amd._lib")
    cls_name, name, kernels = NAMES[method]
    cls = getattr(importlib.import_module("vl_merging_amd." + method), cls_name)
    assert issubclass(cls, mp.MatrixPlan) and (cls.NAME, cls.KERNELS) == (name, kernels)
    with pytest.raises(L.VlmError) as e:
        cls("cpu")
    assert str(e.value) == "the %s kernels run on the GPU only (got device cpu)" % kernels
    # add() and report() as far as a CPU device allows: a plan that skipped its constructor
    plan = cls.__new__(cls)
    plan.device, plan.jobs, plan.keep, plan.rows = torch.device("cpu"), [], [], None
    c = torch.zeros(4, 4)
    with pytest.raises(L.VlmError) as e:
        plan.add([c] * 5, c)
    assert str(e.value) == "%s job takes 1 .. 4 sources, got 5" % name
    with pytest.raises(L.VlmError) as e:
        plan.add([], c)
    assert str(e.value) == "%s job takes 1 .. 4 sources, got 0" % name
    for base, src in ((c, torch.zeros(4, 3)), (torch.zeros(16), torch.zeros(16)), (torch.zeros(0, 4), torch.zeros(0, 4))):
        with pytest.raises(L.VlmError) as e:
            plan.add([src], base)
        assert str(e.value) == "%s job takes non-empty matrices of one shape, got %s" % (name, [tuple(base.shape), tuple(src.shape)])
    with pytest.raises(L.VlmError, match="merge expects float32 checkpoints, got torch.float64"):
        plan.add([c.double()], c)
    for out in (torch.zeros(4, 3), torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 8)[:, ::2], torch.zeros(17)[1:].view(4, 4)):
        with pytest.raises(L.VlmError) as e:
            plan.add([c], c, out=out)
        assert str(e.value) == "%s output must be a contiguous, 16-byte aligned float32 tensor of the sources' shape on cpu" % name
    wide = torch.zeros(1, L.SVD_MAX_Q + 1)
    if method == "tsvm":                                             # the one extra bound
        with pytest.raises(L.VlmError) as e:
            plan.add([wide], wide)
        assert str(e.value) == "the Jacobi SVD holds rows of at most %d doubles, got a (1, %d) matrix" % (L.SVD_MAX_Q, L.SVD_MAX_Q + 1)
    else:
        assert plan.add([wide], wide).shape == wide.shape and len(plan.jobs) == 1
        del plan.jobs[:]
    assert not plan.jobs
    with pytest.raises(L.VlmError) as e:
        plan.report()
    assert str(e.value) == "%s.report() needs a plan that has run" % cls_name
    out = torch.empty(4, 4)
    assert plan.add([c, c], c, lam=1, out=out, name="w") is out
    (job,) = plan.jobs
    assert job[0] == "w" and job[3] is out and job[4] == 1.0 and isinstance(job[4], float) and len(job[2]) == 2


def test_svd_plan_shares_the_device_check_and_the_report_guard(mp, pkg):
    L = importlib.import_module("vl_merging_amd._lib")
    tsvm = importlib.import_module("vl_merging_amd.tsvm")
    assert not issubclass(tsvm.SvdPlan, mp.MatrixPlan)
    with pytest.raises(L.VlmError) as e:
        tsvm.SvdPlan("cpu")
    assert str(e.value) == "the SVD kernels run on the GPU only (got device cpu)"
    plan = tsvm.SvdPlan.__new__(tsvm.SvdPlan)
    plan.rows = None
    with pytest.raises(L.VlmError) as e:
        plan.report()
    assert str(e.value) == "SvdPlan.report() needs a plan that has run"
    plan.rows = [{"rotations": [1, 0], "off": [0.5, 0.0]}]
    got = plan.report()
    assert got == plan.rows and got[0] is not plan.rows[0] and got[0]["off"] is not plan.rows[0]["off"]   # a copy, lists included
