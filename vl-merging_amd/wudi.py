"""WUDI-Merging (Cheng et al., ICML 2025, "Whoever Started the Interference Should End It: Guiding Data-Free Model Merging via Task
Vectors") of the modality experts on the GPU.  No reference site; the rule and the order of its operations: include/vlm_hip.h,
held to the numpy restatement tests/wudi_restatement.py.

Per destination tensor with central tensor c, sources W_0 .. W_{S-1} and lam:
  not 2-D (biases, q_bias, v_bias, the norms): the MEAN task vector, dst = c + sum_i (lam / S)(W_i - c) -- the MergePlan task-vector
    job with ratios [lam / S] * S;
  2-D [m, n] (qkv.weight as one [3D, D] matrix, proj, fc1, fc2), in float64 with tau_i = W_i - c: Adam (iters steps at lr, betas
    0.9 / 0.999, eps 1e-8) on  L(X) = sum_i (1 / ||tau_i||_F^2) ||(X - tau_i) tau_i^T||_F^2  from X_0 = sum_i tau_i, then
    dst = fl32(c + lam * X_T);
  a layer with ONE source: the task-vector job with ratio 1, as in the rest of the family.

grad L = 2 (X G - B) with G = sum_i w_i tau_i^T tau_i and B = sum_i w_i tau_i (tau_i^T tau_i): RegMean's normal equation with the
task vectors' own Gram matrices in place of data.  A step is ONE launch per lock-step group: the fp64 product X G on the MFMA tiles
of csrc/f64ops.hip with the Adam update in its epilogue (csrc/wudi.hip).  The bias corrections depend on the step number alone, so
a merge enqueues everything and reads the device once, for the report.
"""
import math

import torch

from . import _lib as L
from . import ops
from .matrix_plan import MatrixPlan, matrix_merge, run_groups, shape_groups

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8   # torch.optim.Adam's defaults, as the paper's code runs it


def adam_scalars(t, lr, beta1=BETA1, beta2=BETA2):
    """(lr / (1 - beta1^t), sqrt(1 - beta2^t)) in python doubles: what step t of the rule multiplies and divides by."""
    return lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)


class WudiPlan(MatrixPlan):
    """The matrices of a WUDI merge: add() them, run() enqueues everything -- the setup, `iters` step launches per lock-step group,
    the outputs -- and synchronises ONCE at its end, reading the heads for report().  Matrices are grouped by their exact shape
    [m, n] (G is [n, n]: orientation matters) and walk the steps in lock step, a step of a group one launch over all of it (64 at
    a time); independent groups run side by side on side streams.  After run(): self.rows (report()), self.state(j): the device's
    float64 X_T of matrix j."""

    NAME, KERNELS = "a WUDI", "WUDI"

    def __init__(self, device, iters=300, lr=1e-5):
        super().__init__(device)
        if int(iters) != iters or iters < 1:
            raise ValueError("WUDI takes iters >= 1 Adam steps, got %r" % (iters,))
        if not (lr > 0.0 and math.isfinite(lr)):
            raise ValueError("WUDI takes a finite lr > 0, got %r" % (lr,))
        self.iters, self.lr = int(iters), float(lr)
        self._where = {}

    def _chunks(self, g):
        """The calls of a group.  A step does not look at a matrix's source count or lam: it runs the group 64 matrices at a time,
        each such chunk with its own scratch.  The setup and the output do: inside a chunk the matrices are ordered by (S, lam),
        and each run of equal (S, lam) is one setup and one output call on its slice of the chunk's scratch."""
        m, n = g["shape"]
        per = L.get_lib().vlm_wudi_parts(m, n)

        def key(i):
            return len(self.jobs[g["jobs"][i]][2]), self.jobs[g["jobs"][i]][4]
        order = sorted(range(len(g["jobs"])), key=lambda i: (key(i), i))
        for c0 in range(0, len(order), ops.F64_MAX_BATCH):
            ids = order[c0:c0 + ops.F64_MAX_BATCH]
            partials = ops.wudi_partials(m, n, len(ids), self.device)
            runs, a = [], 0
            while a < len(ids):
                b = a
                while b < len(ids) and key(ids[b]) == key(ids[a]):
                    b += 1
                S, lam = key(ids[a])
                runs.append(dict(S=S, lam=lam, work=[g["work"][i] for i in ids[a:b]], jobs=[self.jobs[g["jobs"][i]] for i in ids[a:b]],
                                 partials=partials[a * per:]))
                a = b
            yield dict(work=[g["work"][i] for i in ids], partials=partials, runs=runs)

    def _enqueue(self, g):
        m, n = g["shape"]
        chunks = g["chunks"]
        for ch in chunks:
            for r in ch["runs"]:
                js = r["jobs"]
                ops.wudi_prepare([j[1] for j in js], [[j[2][k] for j in js] for k in range(r["S"])], r["work"], r["partials"])
        for t in range(1, self.iters + 1):
            step, bc2s = adam_scalars(t, self.lr)
            for ch in chunks:
                ops.wudi_step(ch["work"], m, n, t, step, bc2s, ch["partials"], BETA1, BETA2, EPS)
        for ch in chunks:
            for r in ch["runs"]:
                js = r["jobs"]
                ops.wudi_finish(r["work"], [j[1] for j in js], [j[3] for j in js], r["S"], self.iters, r["lam"], r["partials"])

    def run(self):
        if not self.jobs:
            self.rows = []
            return self
        groups = shape_groups(len(self.jobs), lambda j: tuple(self.jobs[j][1].shape), lambda shape: shape[0] * shape[1] ** 2)
        with torch.cuda.device(self.device):
            for g in groups:   # buffers on the CALLER's stream, whose allocator pool they belong to (state() outlives the run)
                m, n = g["shape"]
                g["buf"] = torch.empty(len(g["jobs"]), ops.wudi_work_doubles(m, n), dtype=torch.float64, device=self.device)
                g["work"] = [g["buf"][i] for i in range(len(g["jobs"]))]
                g["chunks"] = list(self._chunks(g))
            run_groups(self.device, groups, self._enqueue)
            heads = torch.cat([g["buf"][:, :L.WUDI_HEAD].reshape(-1) for g in groups]).cpu().tolist()   # the one synchronisation
        rows, k0 = [None] * len(self.jobs), 0
        for g in groups:
            for i, j in enumerate(g["jobs"]):
                name, base, srcs, _, _ = self.jobs[j]
                h = heads[k0 + i * L.WUDI_HEAD: k0 + (i + 1) * L.WUDI_HEAD]
                rows[j] = {"dst": name, "n": base.numel(), "shape": list(base.shape), "S": len(srcs), "iters": self.iters, "lr": self.lr,
                           "sq": h[:len(srcs)], "loss_first": h[9], "loss_last": h[10]}
                self._where[j] = (g, i)
            k0 += len(g["jobs"]) * L.WUDI_HEAD
            del g["chunks"]   # (the scratch and the job lists; the working sets stay for state())
        self.rows = rows
        self.groups = groups
        return self

    def state(self, j):
        """The device's float64 X_T of job j, [m, n] as the tensor is stored."""
        g, i = self._where[j]
        return ops.wudi_state(g["work"][i], g["shape"][0], g["shape"][1], self.iters)


def wudi_merge(state_dict, config, central_weight=None, lam=None, device="cuda", plan_out=None, report_out=None, states_out=None,
               iters=300, lr=1e-5):
    """WUDI merge of the modality experts' task vectors `W_i - central` (the rule: the module docstring).  Same inputs, keys,
    pass-through and KeyError behaviour as sum_task_vectors; `lam=None` takes config["sum_lambda"]; the central tensors are inputs
    only.  `plan_out` receives the WudiPlan FIRST whenever a matrix has several sources, then the MergePlan of everything else if it
    has jobs; `report_out` receives one row per matrix (dst, n, shape, S, iters, lr, sq per source, loss_first = L(X_0), loss_last =
    L(X_{iters-1})); `states_out[dst]` the device's float64 X_iters."""
    wudi = WudiPlan(device, iters=iters, lr=lr)
    out = matrix_merge(wudi, state_dict, config, central_weight, lam, plan_out, report_out)
    if states_out is not None:
        for j, job in enumerate(wudi.jobs):
            states_out[job[0]] = wudi.state(j)
    return out
