"""TSV-M: task singular vectors merging (Gargiulo et al., CVPR 2025, "Task Singular Vectors: Reducing Task Interference in Model
Merging") of the modality experts on the GPU, and the batched float64 SVD it stands on.  No reference site; the rule and the order
of its operations: include/vlm_hip.h, held to the numpy restatement tests/tsvm_restatement.py.

Per destination tensor with central tensor c, sources W_0 .. W_{S-1} and lam:
  not 2-D (biases, q_bias, v_bias, the norms): the MEAN task vector, dst = c + sum_i (lam / S)(W_i - c) -- the MergePlan task-vector
    job with ratios [lam / S] * S;
  2-D [m, n] (qkv.weight as one [3D, D] matrix, proj, fc1, fc2), in float64 with tau_i = W_i - c = U_i diag(s_i) V_i^T, r = min(m, n)
    and k = r // S: every expert's k leading triplets side by side in Ucat [m, kS], scat [kS], Vcat [n, kS] (zero columns for
    singular values that are exactly zero), Uo = polar(Ucat), Vo = polar(Vcat) over the singular values above 2^-40 of the
    largest, dst = fl32(c + lam * Uo diag(scat) Vo^T); k = 0: dst = c;
  a layer with ONE source: the task-vector job with ratio 1, as in the rest of the family.

The SVD is one-sided Jacobi on rows (csrc/jacobi.hip): a sweep is p - 1 launches per lock-step group, each a tournament step over
every matrix of the group.  A matrix whose last sweep rotated nothing is done and later sweeps skip it on the device, so a plan
enqueues SWEEPS of them without a host synchronisation, reads every head in ONE blocking copy, and gives what still rotates
further sweeps in rounds of EXTRA_ROUND up to the head's VLM_SVD_MAX_SWEEPS.  polar(B)^T comes from the same SVD of B^T: R^T times
the unit rows; the recombination is one MFMA-f64 product with the output in its epilogue (csrc/tsvm.hip).
"""
import warnings

import torch

from . import _lib as L
from . import ops
from .matrix_plan import MatrixPlan, batches, cuda_device, matrix_merge, report, run_groups, shape_groups

SWEEPS = 18        # scheduled: the base-size merge needs at most 16 (docs/experiments.md, "TSV-M"); the restated sweep 15 at 768 x 768
EXTRA_ROUND = 2    # further sweeps per round for what the schedule left rotating
POLAR_FLOOR = 2.0 ** -40


class SvdPlan:
    """Batched float64 SVDs: add() matrices (or adopt() loaded working sets), run() enqueues the scheduled sweeps of every
    lock-step group (one working shape [p <= q] each, 64 matrices a launch; independent groups on side streams), reads the heads
    once, sweeps on what still rotates, and finishes (singular values, ranks, unit rows).  After run(): rows[j] = {p, q, transposed,
    sweeps, converged, rotations (per sweep), off (per sweep)}; s(j), order(j), rank(j), vt(j) (unit rows, zero where dropped), rt(j)
    (U^T), head(j): views of the device's working set.  matrix = rt^T diag(s) vt in working orientation (its transpose when
    `transposed`)."""

    def __init__(self, device, sweeps=SWEEPS, floor_rel=0.0):
        self.device = cuda_device(device, "SVD")
        if int(sweeps) != sweeps or not 1 <= sweeps <= L.SVD_MAX_SWEEPS:
            raise ValueError("an SVD plan schedules 1 .. %d sweeps, got %r" % (L.SVD_MAX_SWEEPS, sweeps))
        if not 0.0 <= floor_rel < 1.0:
            raise ValueError("floor_rel lies in [0, 1), got %r" % (floor_rel,))
        self.sweeps, self.floor_rel = int(sweeps), float(floor_rel)
        self.sets = []   # (work, p, q, transposed)
        self.rows = None
        self.launches = 0   # kernel launches run() issued through the library

    def add(self, a):
        """One float64 matrix [m, n] on the device; it is copied (transposed when m > n) into a working set of its own."""
        if a.dtype != torch.float64 or a.dim() != 2 or a.numel() == 0 or a.device != self.device:
            raise L.VlmError("an SVD job takes a non-empty float64 matrix on %s" % self.device)
        m, n = a.shape
        p, q = min(m, n), max(m, n)
        if q > L.SVD_MAX_Q:
            raise L.VlmError("the Jacobi SVD holds rows of at most %d doubles, got a [%d, %d] matrix" % (L.SVD_MAX_Q, m, n))
        work = torch.empty(ops.svd_work_doubles(p, q), dtype=torch.float64, device=self.device)
        ops.svd_views(work, p, q)[1].copy_(a.t() if m > n else a)
        return self.adopt(work, p, q, transposed=m > n)

    def adopt(self, work, p, q, transposed=False):
        """A working set whose A the caller has filled (run() resets its R and head).  Returns its index."""
        self.sets.append((work, p, q, bool(transposed)))
        return len(self.sets) - 1

    def _sweep(self, g, idx, sweep):
        p, q = g["shape"]
        for _, part in batches(idx):
            ops.svd_sweep([self.sets[j][0] for j in part], p, q, sweep)
            self.launches += L.get_lib().vlm_svd_steps(p)

    def _heads(self):
        """Every head in ONE blocking copy."""
        return torch.stack([w[:L.SVD_HEAD] for w, _, _, _ in self.sets]).cpu().tolist()

    @staticmethod
    def _verdict(head, p, ran):
        """(sweeps taken, converged) from a head after `ran` sweeps were issued."""
        if p < 2:
            return 0, True
        for k in range(ran):
            if head[2 + k] == 0.0:
                return k + 1, True
        return ran, False

    def run(self):
        if not self.sets:
            self.rows = []
            return self
        groups = shape_groups(len(self.sets), lambda j: self.sets[j][1:3], lambda shape: shape[0] ** 2 * shape[1])

        def scheduled(g):
            p, q = g["shape"]
            for _, part in batches(g["jobs"]):
                ops.svd_reset([self.sets[j][0] for j in part], p, q)
                self.launches += 1
            for sweep in range(self.sweeps if p > 1 else 0):
                self._sweep(g, g["jobs"], sweep)
        with torch.cuda.device(self.device):
            run_groups(self.device, groups, scheduled)
            ran = self.sweeps
            heads = self._heads()   # the one synchronisation (and one more per extra round)

            def rotating():
                return [[j for j in g["jobs"] if not self._verdict(heads[j], g["shape"][0], ran)[1]] for g in groups]
            todo = rotating()
            while any(todo) and ran < L.SVD_MAX_SWEEPS:
                more = min(EXTRA_ROUND, L.SVD_MAX_SWEEPS - ran)
                for g, idx in zip(groups, todo):
                    for sweep in range(ran, ran + more if idx else ran):
                        self._sweep(g, idx, sweep)
                ran += more
                heads = self._heads()
                todo = rotating()
            for g in groups:
                p, q = g["shape"]
                for _, part in batches(g["jobs"]):
                    ops.svd_finish([self.sets[j][0] for j in part], p, q, self.floor_rel)
                    self.launches += 3
        rows = []
        for j, (_, p, q, transposed) in enumerate(self.sets):
            k, ok = self._verdict(heads[j], p, ran)
            if not ok:
                warnings.warn("Jacobi SVD: matrix %d [%d, %d] still rotates after %d sweeps (%d rotations, largest |gamma| / "
                              "sqrt(alpha beta) %.3e); it is used as it stands" % (j, p, q, k, heads[j][2 + k - 1], heads[j][32 + k - 1]))
            rows.append({"p": p, "q": q, "transposed": transposed, "sweeps": k, "converged": ok,
                         "rotations": [int(v) for v in heads[j][2:2 + k]], "off": heads[j][32:32 + k]})
        self.rows = rows
        self.groups = groups
        return self

    report = report

    def _view(self, j, which):
        work, p, q, _ = self.sets[j]
        return ops.svd_views(work, p, q)[which]

    def head(self, j):
        return self._view(j, 0)

    def vt(self, j):
        return self._view(j, 1)

    def rt(self, j):
        return self._view(j, 2)

    def s(self, j):
        return self._view(j, 3)

    def rank(self, j):
        return self._view(j, 4)

    def order(self, j):
        return self._view(j, 5)


class TsvPlan(MatrixPlan):
    """The matrices of a TSV-M merge: add() them, run() takes the SVDs of every task vector in one SvdPlan, gathers Ucat^T and
    Vcat^T, takes their SVDs in a second SvdPlan, and enqueues the polar products and the outputs (run() does not end
    synchronised).  After run(): self.rows (report()), self.task_vector(j): the device's float64 merged task vector of matrix j in
    the tensor's own orientation."""

    NAME, KERNELS = "a TSV-M", "SVD"

    def __init__(self, device, sweeps=SWEEPS):
        super().__init__(device)
        self.svd = [SvdPlan(self.device, sweeps), SvdPlan(self.device, sweeps, floor_rel=POLAR_FLOOR)]
        self.launches = 0   # kernel launches run() issued through the library, the SVD plans' included
        self._t = {}

    def _check_shape(self, shape):
        if max(shape) > L.SVD_MAX_Q:
            raise L.VlmError("the Jacobi SVD holds rows of at most %d doubles, got a %s matrix" % (L.SVD_MAX_Q, tuple(shape)))

    def run(self):
        if not self.jobs:
            self.rows = []
            return self
        jobs, dev = self.jobs, self.device
        dims = [self._dims(j) for j in range(len(jobs))]
        live = [j for j, d in enumerate(dims) if d["k"] > 0]
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            # ---- the SVDs of the task vectors
            first = {}   # job -> the indices of its S working sets in svd[0]
            sets = {}
            for (p, q), js in self._group(live, lambda d: (d["p"], d["q"])):
                buf = torch.empty(sum(dims[j]["S"] for j in js), ops.svd_work_doubles(p, q), **f64)
                at = 0
                for j in js:
                    sets[j] = [buf[at + i] for i in range(dims[j]["S"])]
                    at += dims[j]["S"]
            for i in range(L.MERGE_MAX_SRC):
                for _, part in batches([j for j in live if dims[j]["S"] > i], lambda j: tuple(jobs[j][1].shape)):
                    ops.tsv_delta([jobs[j][1] for j in part], [jobs[j][2][i] for j in part], [sets[j][i] for j in part])
                    self.launches += 1
            for j in live:
                first[j] = [self.svd[0].adopt(w, dims[j]["p"], dims[j]["q"], dims[j]["m"] > dims[j]["n"]) for w in sets[j]]
            self.svd[0].run()
            # ---- Ucat^T [kS, p] and Vcat^T [kS, q], their SVDs
            second, cat, scat = {}, {}, {}
            for (kS, p, q), js in self._group(live, lambda d: (d["k"] * d["S"], d["p"], d["q"])):
                ub = torch.empty(len(js), ops.svd_work_doubles(kS, p), **f64)
                vb = torch.empty(len(js), ops.svd_work_doubles(kS, q), **f64)
                sb = torch.empty(len(js), kS, **f64)
                for i, j in enumerate(js):
                    cat[j], scat[j] = (ub[i], vb[i]), sb[i]
            for (p, q, S, k), part in batches(live, lambda j: (dims[j]["p"], dims[j]["q"], dims[j]["S"], dims[j]["k"])):
                src = [[sets[j][i] for j in part] for i in range(S)]
                ops.tsv_gather(src, p, q, k, 0, [cat[j][0] for j in part])
                ops.tsv_gather(src, p, q, k, 1, [cat[j][1] for j in part], [scat[j] for j in part])
                self.launches += 2
            for j in live:
                d = dims[j]
                second[j] = (self.svd[1].adopt(cat[j][0], d["k"] * d["S"], d["p"]), self.svd[1].adopt(cat[j][1], d["k"] * d["S"], d["q"]))
            # the spectra of the task vectors, for the report: enqueued before the second plan's blocking read, fetched after it
            spectra = torch.cat([torch.cat([self.svd[0].s(i), self.svd[0].order(i).double()]) for j in live for i in first[j]]) if live else None
            self.svd[1].run()
            # ---- the transposed polar factors R^T (unit rows), T = PU^T diag(scat) PV and the outputs
            pol = {}
            for side in (0, 1):
                for (kS, ln), part in batches(live, lambda j: (dims[j]["k"] * dims[j]["S"], dims[j]["q" if side else "p"])):
                    outb = torch.empty(len(part), kS, ln, **f64)
                    for i, j in enumerate(part):
                        pol.setdefault(j, [None, None])[side] = outb[i]
                    ops.gemm_f64_batched([self.svd[1].rt(second[j][side]) for j in part], [self.svd[1].vt(second[j][side]) for j in part],
                                         [pol[j][side] for j in part], ta=True)
                    self.launches += 1
            for (shape, kS, lam), part in batches(range(len(jobs)), lambda j: (tuple(jobs[j][1].shape), dims[j]["k"] * dims[j]["S"], jobs[j][4])):
                tb = torch.empty(len(part), min(shape), max(shape), **f64)
                for i, j in enumerate(part):
                    self._t[j] = tb[i]
                dummy = [tb[i] for i in range(len(part))]
                ops.tsv_apply([pol[j][0] for j in part] if kS else dummy, [pol[j][1] for j in part] if kS else dummy,
                              [scat[j] for j in part] if kS else dummy, [jobs[j][1] for j in part], [jobs[j][3] for j in part],
                              dummy, kS, lam)
                self.launches += 1
            spectra = spectra.cpu().tolist() if live else []
            heads2 = {j: [self.svd[1].head(i)[:2] for i in second[j]] for j in live}
            dropped = torch.stack([h for j in live for h in heads2[j]]).cpu().tolist() if live else []
        rows, at, dr = [], 0, 0
        for j, (name, base, srcs, _, _) in enumerate(jobs):
            d = dims[j]
            row = {"dst": name, "n": base.numel(), "shape": list(base.shape), "transposed": d["m"] > d["n"], "S": d["S"], "k": d["k"],
                   "sweeps": {"tau": [], "U": None, "V": None}, "converged": {"tau": [], "U": None, "V": None},
                   "s_max": [], "s_kept_min": [], "s_dropped_max": [], "energy_kept": [], "dropped": {"U": 0, "V": 0}}
            if d["k"] > 0:
                p, k = d["p"], d["k"]
                for i in first[j]:
                    s, order = spectra[at:at + p], spectra[at + p:at + 2 * p]
                    at += 2 * p
                    s = [s[int(o)] for o in order]   # descending
                    total = sum(v * v for v in s)
                    row["s_max"].append(s[0])
                    row["s_kept_min"].append(s[k - 1])
                    row["s_dropped_max"].append(s[k] if k < p else 0.0)
                    row["energy_kept"].append(sum(v * v for v in s[:k]) / total if total > 0 else 1.0)
                    row["sweeps"]["tau"].append(self.svd[0].rows[i]["sweeps"])
                    row["converged"]["tau"].append(self.svd[0].rows[i]["converged"])
                for side, i in zip("UV", second[j]):
                    row["sweeps"][side] = self.svd[1].rows[i]["sweeps"]
                    row["converged"][side] = self.svd[1].rows[i]["converged"]
                    row["dropped"][side] = int(dropped[dr][1])
                    dr += 1
                if not (all(row["converged"]["tau"]) and row["converged"]["U"] and row["converged"]["V"]):
                    warnings.warn("TSV-M: an SVD of %s has not converged (%s); the matrix is written as it stands" % (name, row["converged"]))
            rows.append(row)
        self.rows = rows
        self.launches += self.svd[0].launches + self.svd[1].launches
        self.groups = [[dict(shape=list(g["shape"]), matrices=len(g["jobs"])) for g in getattr(s, "groups", [])] for s in self.svd]
        self.svd = None   # (the working sets: only the merged task vectors stay)
        return self

    def _group(self, ids, key):
        by = {}
        for j in ids:
            by.setdefault(key(self._dims(j)), []).append(j)
        return sorted(by.items())

    def _dims(self, j):
        _, base, srcs, _, _ = self.jobs[j]
        m, n = base.shape
        return dict(m=m, n=n, p=min(m, n), q=max(m, n), S=len(srcs), k=min(m, n) // len(srcs))

    def task_vector(self, j):
        """The device's float64 merged task vector of job j, [m, n] as the tensor is stored (a transposed view when m > n)."""
        m, n = self.jobs[j][1].shape
        return self._t[j].t() if m > n else self._t[j]


def tsvm_merge(state_dict, config, central_weight=None, lam=None, device="cuda", plan_out=None, report_out=None):
    """TSV-M merge of the modality experts' task vectors `W_i - central` (the rule: the module docstring).  Same inputs, keys,
    pass-through and KeyError behaviour as sum_task_vectors; `lam=None` takes config["sum_lambda"]; the central tensors are inputs
    only.  `plan_out` receives the TsvPlan FIRST whenever a matrix has several sources, then the MergePlan of everything else if it
    has jobs; `report_out` receives one row per matrix: dst, n, shape, transposed, S, k, sweeps and converged ({tau: per source, U,
    V}: every SVD taken), s_max, s_kept_min, s_dropped_max (the gap at the cut) and energy_kept per source, dropped ({U, V}: polar
    directions below 2^-40 of the largest).  An SVD that still rotates after VLM_SVD_MAX_SWEEPS sweeps is used as it stands,
    reported with converged = False, and warned about."""
    return matrix_merge(TsvPlan(device), state_dict, config, central_weight, lam, plan_out, report_out)
