"""What the per-matrix float64 merge methods (isoc.py, wudi.py, tsvm.py) and RegMean's solves (regmean.py) share on the host: the
plan a method's matrices are added to (MatrixPlan), the lock-step groups of one shape and the streams they run on (shape_groups,
run_groups), the cut of a list of matrices into kernel-argument tables (batches), and the walk over a state dict that hands the
2-D tensors to a method's plan and everything else to the task-vector job (matrix_merge)."""
import copy

import torch

from . import _lib as L
from . import merge as M
from . import ops


def cuda_device(device, kernels):
    """torch.device(device), "cuda" resolved to the current device's index; the `kernels` kernels run nowhere else."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.VlmError("the %s kernels run on the GPU only (got device %s)" % (kernels, device))
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def report(plan):
    """A copy of the rows of a plan that has run."""
    if plan.rows is None:
        raise L.VlmError("%s.report() needs a plan that has run" % type(plan).__name__)
    return copy.deepcopy(plan.rows)


class MatrixPlan:
    """The matrices of a merge: add() them, a subclass's run() merges them and leaves self.rows for report().  A subclass names
    itself for the messages (NAME: "an Iso-C") and its kernels (KERNELS), and may refuse a shape in _check_shape."""

    NAME = KERNELS = None
    report = report

    def __init__(self, device):
        self.device = cuda_device(device, self.KERNELS)
        self.jobs = []   # (name, central, sources, out, lam)
        self.keep = []
        self.rows = None

    _dev = M._Plan._dev   # float32, on the device, contiguous, 16-byte aligned: staged and kept alive where it is not

    def _check_shape(self, shape):
        pass

    def add(self, srcs, base, lam=1.0, out=None, name=None):
        """One output matrix.  `out` may be `base` or one of `srcs` (they are read before it is written) or any tensor that meets
        none of them."""
        if not 1 <= len(srcs) <= L.MERGE_MAX_SRC:
            raise L.VlmError("%s job takes 1 .. %d sources, got %d" % (self.NAME, L.MERGE_MAX_SRC, len(srcs)))
        base = self._dev(base)
        srcs = [self._dev(s) for s in srcs]
        if base.dim() != 2 or base.numel() == 0 or any(s.shape != base.shape for s in srcs):
            raise L.VlmError("%s job takes non-empty matrices of one shape, got %s" % (self.NAME, [tuple(t.shape) for t in [base] + srcs]))
        self._check_shape(base.shape)
        if out is None:
            out = torch.empty_like(base)
        elif out.shape != base.shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() \
                or (out.data_ptr() & 15):
            raise L.VlmError("%s output must be a contiguous, 16-byte aligned float32 tensor of the sources' shape on %s"
                             % (self.NAME, self.device))
        self.jobs.append((name, base, srcs, out, float(lam)))
        return out


def batches(ids, key=None):
    """(key, part) for `ids` grouped by key(i): the keys in sorted order, a key's ids in their given order and at most
    ops.F64_MAX_BATCH -- one kernel-argument table -- a part.  Without `key`: one group, key None."""
    by = {}
    for i in ids:
        by.setdefault(key(i) if key else None, []).append(i)
    for k in sorted(by):
        for i0 in range(0, len(by[k]), ops.F64_MAX_BATCH):
            yield k, by[k][i0:i0 + ops.F64_MAX_BATCH]


def shape_groups(n, shape, cost):
    """The lock-step groups of matrices 0 .. n - 1, [dict(shape=, jobs=[indices])]: one per shape(j), the one with the largest
    cost(shape) * matrices first."""
    by = {}
    for j in range(n):
        by.setdefault(shape(j), []).append(j)
    return [dict(shape=key, jobs=js) for key, js in sorted(by.items(), key=lambda kv: -cost(kv[0]) * len(kv[1]))]


_SIDE = {}


def _side_streams(device, n):
    pool = _SIDE.setdefault(torch.device(device).index, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool


def run_groups(device, groups, enqueue, ready=None):
    """enqueue(g) for independent groups, largest first: the first stays on the caller's stream, every other runs on a side stream
    of its own that first waits for the caller's stream -- or for the event ready(g), where that is given and not None -- and that
    the caller's stream waits for at the end.  Launch order is the groups' order.  What a group works in is allocated by the
    caller, on the caller's stream, before this."""
    main = torch.cuda.current_stream(device)
    side = _side_streams(device, len(groups) - 1)
    for n_, g in enumerate(groups):
        st = main if n_ == 0 else side[n_ - 1]
        if st is not main:
            event = ready(g) if ready is not None else None
            if event is not None:
                st.wait_event(event)
            else:
                st.wait_stream(main)
        with torch.cuda.stream(st):
            enqueue(g)
    for st in side[:len(groups) - 1]:
        main.wait_stream(st)


def matrix_merge(mat, state_dict, config, central_weight=None, lam=None, plan_out=None, report_out=None):
    """The merge of the modality experts' task vectors `W_i - central` around the empty MatrixPlan `mat`: a 2-D tensor with several
    sources is added to `mat`, any other tensor with several sources takes the MEAN task vector, a layer with ONE source the
    task-vector job with ratio 1.  Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors; `lam=None` takes
    config["sum_lambda"].  `plan_out` receives `mat` FIRST if it has jobs, then the MergePlan of everything else if it has jobs;
    `report_out` one row per matrix."""
    if lam is None:
        lam = config["sum_lambda"]
    plan = M.MergePlan(mat.device)
    out = M._passthrough(state_dict)
    central = M._central(central_weight, config)
    for dst, mods, srcs, through in M._walk(state_dict, config, central):
        if srcs is None:
            out[dst] = through
        elif len(mods) == 1:
            out[dst] = plan.add(L.MERGE_TASKVEC, M._tensors(srcs), [1], base=central[dst])
        elif central[dst].dim() == 2:
            out[dst] = mat.add(M._tensors(srcs), central[dst], lam=lam, name=dst)
        else:
            out[dst] = plan.add(L.MERGE_TASKVEC, M._tensors(srcs), [lam / len(srcs)] * len(srcs), base=central[dst])
    if plan.jobs:
        plan.run()   # (enqueued first: the streaming pass runs under the matrix plan's launch chain)
    if mat.jobs:
        mat.run()
    if plan_out is not None:
        plan_out.extend(p for p in (mat, plan) if p.jobs)
    if report_out is not None:
        report_out.extend(mat.report() if mat.jobs else [])
    return out
