"""Iso-C: isotropic merging (Marczak et al. 2025, "No Task Left Behind: Isotropic Model Merging with Common and Task-Specific
Subspaces") of the modality experts on the GPU.  No reference site; the rule and the order of its operations: include/vlm_hip.h,
held to the numpy restatement tests/isoc_restatement.py.

Per destination tensor with central tensor c, sources W_0 .. W_{S-1} and lam:
  not 2-D (biases, q_bias, v_bias, the norms): the MEAN task vector, dst = c + sum_m (lam / S)(W_m - c) -- the MergePlan task-vector
    job with ratios [lam / S] * S;
  2-D (qkv.weight as one [3D, D] matrix, proj, fc1, fc2): D = sum_m (W_m - c) in float64, dst = fl32(c + ((lam * sum sigma) / r) U V^T)
    with D = U diag(sigma) V^T and r = min(m, n) -- the SUM of the task vectors with its spectrum flattened to its mean;
  a layer with ONE source: the task-vector job with ratio 1, as in the rest of the family.

U V^T is the polar factor of D and sum sigma = <U V^T, D>, so no SVD is taken: a Cholesky-based QDWH iteration (Nakatsukasa, Bai &
Gygi 2010) needs products, SPD factorisations and right-solves only -- RegMean's float64 leg (csrc/f64ops.hip, regmean._Solves'
lock-step batching).  Its coefficients (iso_schedule) depend on a lower bound chosen up front, not on the data, so a merge runs
without a host synchronisation until its verdicts are read ONCE; a matrix whose last step is not small then (singular values
far below l0) takes further Halley steps (3, 1, 3) in rounds of 4, one read per round.
"""
import math
import warnings

import torch

from . import _lib as L
from . import ops
from .matrix_plan import MatrixPlan, batches, matrix_merge, run_groups, shape_groups

EXTRA_ROUND = 4    # further steps per round for what the schedule left unconverged
EXTRA_MAX = 32     # and at most this many
STEP_TOL = 1e-10   # converged: ||X_{k+1} - X_k||_F <= STEP_TOL * sqrt(r); cubic convergence leaves about its cube


def iso_schedule(l0=1e-6, steps=8):
    """The (a, b, c) of every QDWH step for singular values of X_0 in [l0, 1], in python doubles: a function of (l0, steps) alone.
    (3, 1, 3) -- Halley's iteration -- once the lower bound has reached 1."""
    if not (0.0 < l0 <= 1.0) or steps < 1:
        raise ValueError("iso_schedule needs 0 < l0 <= 1 and steps >= 1, got %r, %r" % (l0, steps))
    out, l = [], float(l0)
    for _ in range(steps):
        if l >= 1.0:
            a, b, c = 3.0, 1.0, 3.0
        else:
            l2 = l * l
            d = (4.0 * (1.0 - l2) / (l2 * l2)) ** (1.0 / 3.0)
            a = math.sqrt(1.0 + d) + 0.5 * math.sqrt(8.0 - 4.0 * d + 8.0 * (2.0 - l2) / (l2 * math.sqrt(1.0 + d)))
            b = (a - 1.0) ** 2 / 4.0
            c = a + b - 1.0
        out.append((a, b, c))
        l = min(1.0, l * (a + b * l * l) / (1.0 + c * l * l))
    return out


class IsoPlan(MatrixPlan):
    """The matrices of an Iso-C merge: add() them, run() enqueues everything and reads the verdicts (the outputs' apply pass is
    enqueued behind that read: run() does not end synchronised).  Matrices are grouped by working shape [rows >= cols] (fc1 and
    the transposed fc2 are one group) and walk the iteration in lock step, every step of a group one launch over all of it (64 at
    a time); independent groups run side by side on side streams.  After run(): self.rows (report()), self.factor(i): the
    device's float64 X of matrix i in working orientation."""

    NAME, KERNELS = "an Iso-C", "Iso-C"

    def __init__(self, device, l0=1e-6, steps=8):
        super().__init__(device)
        if not 1 <= steps <= L.ISO_MAX_STEPS - EXTRA_MAX:
            raise ValueError("Iso-C takes 1 .. %d scheduled steps, got %r" % (L.ISO_MAX_STEPS - EXTRA_MAX, steps))
        self.schedule = iso_schedule(l0, steps)
        self._where = {}

    # ------------------------------------------------------------------------------------------------ the device side
    def _step(self, g, idx, k, abc):
        """Step k with coefficients abc for the matrices idx of group g, 64 at a time."""
        a, b, c = abc
        rows, cols = g["shape"]
        for _, part in batches(idx):
            work, zs = [g["work"][i] for i in part], [g["z"][i] for i in part]
            ys = [g["y"][i] for i in part]
            ops.iso_gram(work, rows, cols, zs, c, first=k == 0)
            st = torch.zeros(len(part), dtype=torch.int32, device=self.device)  # zero on entry; read with the heads
            g["status"].append(st)
            ops.cholesky_batched_(zs, st)
            ops.solve_spd_right_batched_(ys, zs)
            ops.iso_step(work, rows, cols, b / c, a - b / c, k, k == 0, g["partials"])

    def _finish(self, g, idx, phases):
        """The phases of ops.iso_finish for the matrices idx of group g: one call per original shape (the two orientations of a
        group), lam and 64 matrices."""
        def key(i):
            job = self.jobs[g["jobs"][i]]
            return tuple(job[1].shape), job[4]
        for (shape, lam), part in batches(idx, key):
            js = [self.jobs[g["jobs"][i]] for i in part]
            ops.iso_finish([g["work"][i] for i in part], [j[1] for j in js], [j[3] for j in js], lam, g["partials"], phases)

    def _allocate(self, g):
        """The group's buffers, on the CALLER's stream: the group's side stream works in them between its wait for the caller's
        stream and the caller's wait for it; the extra rounds, the apply pass and whoever holds a factor() afterwards use them on
        the caller's stream, whose allocator pool they belong to."""
        rows, cols = g["shape"]
        n = len(g["jobs"])
        N = rows * cols
        buf = torch.empty(n, L.ISO_HEAD + 3 * N, dtype=torch.float64, device=self.device)
        buf[:, :L.ISO_HEAD].zero_()
        g["buf"] = buf
        g["work"] = [buf[i] for i in range(n)]
        g["y"] = [buf[i, L.ISO_HEAD + 2 * N:].view(rows, cols) for i in range(n)]
        zbuf = torch.empty(n, cols, cols, dtype=torch.float64, device=self.device)
        g["z"] = [zbuf[i] for i in range(n)]
        g["status"] = []   # (allocated by _step under the group's stream; read and dropped by the next _heads, which synchronises)
        g["partials"] = ops.iso_partials(rows, cols, min(n, ops.F64_MAX_BATCH), self.device)

    def _delta(self, g):
        """D of every matrix of the group: one call per original shape, source count and 64 matrices."""
        def key(i):
            job = self.jobs[g["jobs"][i]]
            return tuple(job[1].shape), len(job[2])
        for (shape, S), part in batches(range(len(g["jobs"])), key):
            js = [self.jobs[g["jobs"][i]] for i in part]
            ops.iso_delta([j[1] for j in js], [[j[2][k] for j in js] for k in range(S)], [g["work"][i] for i in part], g["partials"])

    def _heads(self, groups):
        """Every head and Cholesky verdict of the groups in ONE blocking copy: the merge's one synchronisation (and one more per
        extra round)."""
        heads = [g["buf"][:, :L.ISO_HEAD].reshape(-1) for g in groups]
        status = [st.double() for g in groups for st in g["status"]]
        flat = torch.cat(heads + status).cpu().tolist()
        n_head = sum(h.numel() for h in heads)
        if any(flat[n_head:]):
            raise L.VlmError("Iso-C: I + c X^T X has no Cholesky factor (verdicts %s): the iteration met a non-finite value"
                             % ([int(v) for v in flat[n_head:]],))
        out, k0 = [], 0
        for g in groups:
            g["status"] = []
            n = len(g["jobs"])
            out.append([flat[k0 + i * L.ISO_HEAD: k0 + (i + 1) * L.ISO_HEAD] for i in range(n)])
            k0 += n * L.ISO_HEAD
        return out

    def run(self):
        if not self.jobs:
            self.rows = []
            return self
        groups = shape_groups(len(self.jobs), lambda j: (max(self.jobs[j][1].shape), min(self.jobs[j][1].shape)),
                              lambda shape: shape[0] * shape[1] ** 2)
        K = len(self.schedule)

        def scheduled(g):
            self._delta(g)
            every = list(range(len(g["jobs"])))
            for k, abc in enumerate(self.schedule):
                self._step(g, every, k, abc)
            self._finish(g, every, L.ISO_PHASE_NUCLEAR)
        with torch.cuda.device(self.device):
            for g in groups:
                self._allocate(g)
            run_groups(self.device, groups, scheduled)
            # A matrix's output is written ONCE, after its verdict: the apply pass reads the central tensor, which the output may be.
            # Before the read only <X, D> is made, so the common case is still one synchronisation, with the apply pass enqueued behind it.
            heads = self._heads(groups)
            steps = [[K] * len(g["jobs"]) for g in groups]

            def pending(n_, i):
                return steps[n_][i] < K + EXTRA_MAX and not self._converged(heads[n_][i], steps[n_][i], groups[n_]["shape"][1])
            todo = [[i for i in range(len(g["jobs"])) if pending(n_, i)] for n_, g in enumerate(groups)]
            for n_, g in enumerate(groups):
                self._finish(g, [i for i in range(len(g["jobs"])) if i not in todo[n_]], L.ISO_PHASE_APPLY)
            while any(todo):
                for n_, g in enumerate(groups):  # (the matrices of a group that are still at it have taken the same number of steps)
                    for _ in range(EXTRA_ROUND if todo[n_] else 0):
                        self._step(g, todo[n_], steps[n_][todo[n_][0]], (3.0, 1.0, 3.0))
                        for i in todo[n_]:
                            steps[n_][i] += 1
                    self._finish(g, todo[n_], L.ISO_PHASE_NUCLEAR)
                heads = self._heads(groups)
                for n_, g in enumerate(groups):
                    done = [i for i in todo[n_] if not pending(n_, i)]
                    self._finish(g, done, L.ISO_PHASE_APPLY)
                    todo[n_] = [i for i in todo[n_] if i not in done]
        rows = [None] * len(self.jobs)
        for n_, g in enumerate(groups):
            r = g["shape"][1]
            for i, j in enumerate(g["jobs"]):
                name, base, srcs, _, _ = self.jobs[j]
                h, k = heads[n_][i], steps[n_][i]
                ok = self._converged(h, k, r)
                if not ok:
                    warnings.warn("Iso-C: the polar iteration of %s has not converged after %d steps (last step %.3e); the matrix "
                                  "is written as it stands" % (name, k, math.sqrt(h[1 + k])))
                rows[j] = {"dst": name, "n": base.numel(), "shape": list(base.shape), "transposed": base.shape[0] < base.shape[1],
                           "S": len(srcs), "fro": math.sqrt(h[0]), "nuclear": h[1], "sigma_mean": h[1] / r, "steps": k,
                           "last_step": math.sqrt(h[1 + k]), "converged": ok}
                self._where[j] = (g, i)
        self.rows = rows
        self.groups = groups
        return self

    @staticmethod
    def _converged(head, k, r):
        return math.sqrt(head[1 + k]) <= STEP_TOL * math.sqrt(r)   # head[2 + (k - 1)]: the last step taken

    def factor(self, j):
        """The device's float64 X of job j, [rows >= cols] (the transpose of the polar factor when the matrix is wide)."""
        g, i = self._where[j]
        rows, cols = g["shape"]
        N = rows * cols
        return g["buf"][i, L.ISO_HEAD + N: L.ISO_HEAD + 2 * N].view(rows, cols)

    def delta(self, j):
        """The device's float64 D of job j in working orientation."""
        g, i = self._where[j]
        rows, cols = g["shape"]
        return g["buf"][i, L.ISO_HEAD: L.ISO_HEAD + rows * cols].view(rows, cols)


def isoc_merge(state_dict, config, central_weight=None, lam=None, device="cuda", plan_out=None, report_out=None, factors_out=None,
               l0=1e-6, steps=8):
    """Iso-C merge of the modality experts' task vectors `W_m - central` (the rule: the module docstring).  Same inputs, keys,
    pass-through and KeyError behaviour as sum_task_vectors; `lam=None` takes config["sum_lambda"]; the central tensors are inputs
    only.  `plan_out` receives the IsoPlan FIRST whenever a matrix has several sources, then the MergePlan of everything else if it
    has jobs; `report_out` receives one row per matrix (dst, n, shape, transposed, S, fro, nuclear, sigma_mean, steps, last_step,
    converged); `factors_out[dst]` the device's float64 X in working orientation.  A matrix that has not converged after the extra
    rounds is written as it stands, reported with converged = False, and warned about."""
    iso = IsoPlan(device, l0=l0, steps=steps)
    out = matrix_merge(iso, state_dict, config, central_weight, lam, plan_out, report_out)
    if factors_out is not None:
        for j, job in enumerate(iso.jobs):
            factors_out[job[0]] = iso.factor(j)
    return out
