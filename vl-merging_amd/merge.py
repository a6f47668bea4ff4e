"""Checkpoint merging on the GPU: interpolation, task-vector arithmetic, RegMean, TIES, DARE, Breadcrumbs, DELLA, Model Stock, SCE,
SLERP / Karcher mean, Consensus merging with TALL masks (and the restore of the experts from them) -- and the expert-pair statistics
(expert_stats) that say how far apart the experts are before any of them is tried.

Drop-in for ViLTransformerSS.merge_weights / sum_task_vectors / regmean
(reference src/vilt/modules/vilt_module.py:533-638, :640-746, :366-531): same `state_dict -> state_dict`
contract, same key grammar, same pass-through-by-identity of non-block keys, same "already merged key
passes through" and KeyError behaviour; the per-element arithmetic of all 156 output tensors runs in ONE
launch of the HIP merge kernel (csrc/merge.hip) and is bit-exact with the reference's CPU result.

ties_merge (TIES-merging, Yadav et al. 2023) has NO reference site: the reference has no TIES.  It takes what sum_task_vectors
takes and follows its dictionary logic; its arithmetic (include/vlm_hip.h, csrc/ties.hip) is pinned to a numpy restatement of
the rule (tests/ties_restatement.py), not to the reference.  dare_merge (DARE, Yu et al. 2023) likewise: no reference site, the
rule in include/vlm_hip.h, csrc/dare.hip held to tests/dare_restatement.py.  expert_stats likewise: the rule (with the order of
its sums) in include/vlm_hip.h, csrc/pairstats.hip held to tests/pairstats_restatement.py.  band_merge (Model Breadcrumbs,
Davari & Belilovsky 2023) likewise: the rule in include/vlm_hip.h, csrc/band.hip held to tests/band_restatement.py.  della_merge
(DELLA, Deep et al. 2024) likewise: the rule in include/vlm_hip.h, csrc/della.hip held to tests/della_restatement.py.

stock_merge (Model Stock, Jang, Yun & Han 2024) likewise: no reference site, csrc/stock.hip held to tests/stock_restatement.py.
Its rule (include/vlm_hip.h), per tensor with central tensor c and sources W_0 .. W_{S-1}; fp32 rounds once, no FMA; f64 = the
operand widened exactly, the operation in double:
  1. x_m = W_m - c (fp32)
  2. sq[m] = sum f64(x_m) f64(x_m);  dot[(a, b)] = sum f64(x_a) f64(x_b) -- the pair statistics' sums, in their order
  3. in f64, on the device: cos_p = dot_p / sqrt(sq_a sq_b) (+0.0 where that root is not > 0);  cos = their mean;
     cc = cos clamped to [0, 1] by comparison;  t = S cc / (1 + (S - 1) cc) (S = 1: t = 1);  scale = float32(t / S)
  4. d = ((0 + x_0) + x_1) + ... (fp32);  dst = c + scale * d
It has no hyper-parameter; the apply pass reads a scalar the reduction over the same tensor made, ordered by the stream alone.

sce_merge (SCE, Wan et al. 2024) likewise: no reference site, the rule in include/vlm_hip.h, csrc/sce.hip held to
tests/sce_restatement.py: a select on the variance across the experts, a reduction that depends on its threshold, an apply pass
that reads both.

sphere_merge (SLERP and the Karcher mean; mergekit's nuslerp / karcher) likewise: no reference site, the rule in include/vlm_hip.h,
csrc/sphere.hip held to tests/sphere_restatement.py: one coefficient per source and per group (a tensor or a row), made by an
iterative solve on the device from the group's Gram matrix.

consensus_merge (Consensus merging with TALL masks, Wang et al. 2024) likewise: no reference site, csrc/tall.hip held to
tests/tall_restatement.py.  Its rule (include/vlm_hip.h), per tensor with central tensor c, sources W_0 .. W_{S-1}, tall_lambda >= 0,
an integer k in [0, S] and lam; fp32 rounds once, no FMA:
  1. x_m = W_m - c
  2. d = ((0 + x_0) + x_1) + ...
  3. keep_m = |x_m| >= tall_lambda * |d - x_m|
  4. sel = (sum_m keep_m) >= k
  5. dst = c + lam * (sel ? d : +0.0)
  6. the keep_m, packed 32 to a word (bit 0 first), are the TALL masks
It is the first method that decides per element by comparing an expert with the others, and the first whose streaming pass has a
bit-packed side output.  tall_restore is the reverse direction: ufo + masks -> all_moe, dst = bit ? unified : central per expert.

emr_merge (EMR-Merging: elect, mask, rescale; Huang et al. 2024) likewise: no reference site, csrc/emr.hip held to
tests/emr_restatement.py.  Its rule (include/vlm_hip.h), per tensor with central tensor c, sources W_0 .. W_{S-1} and lam:
  1. x_m = W_m - c
  2. s = ((0 + x_0) + x_1) + ...; its sign by comparison
  3. agree_m = x_m has the sign of s;  e = max over the agreeing m of |x_m|;  u = sign(s) * e
  4. dst = c + lam * u
  5. the agree_m, packed as the TALL masks are
  6. a[m] = sum f64(|x_m|), b[m] = sum (agree_m ? f64(e) : 0) in the family's pinned order;  rescale[m] = f32(a[m] / b[m])
emr_restore is the way back: dst = central + rescale * (bit ? unified - central : 0) per expert.  Rescalers are per tensor, not per
model, and an element with s == 0 contributes nothing: the two departures from the paper's code.

isoc.isoc_merge (Iso-C, isotropic merging; Marczak et al. 2025) lives in isoc.py beside regmean.py, whose float64 leg it runs on: no
reference site, csrc/isoc.hip and the SYRK of csrc/f64ops.hip held to tests/isoc_restatement.py.  It is the one method here that
looks at a weight as a matrix.  Its rule (include/vlm_hip.h), per 2-D tensor [m, n] with central tensor c, sources W_0 .. W_{S-1}, lam
and r = min(m, n), in float64:
  1. D = ((0 + (W_0 - c)) + (W_1 - c)) + ...      (the sum, not the mean)
  2. D = U diag(sigma) V^T;  Q = U V^T over the non-zero sigma
  3. dst = fl32(c + ((lam * sum sigma) / r) * Q);  D = 0: dst = c
Q is the polar factor of D and sum sigma = <Q, D>: a Cholesky-based QDWH iteration makes them from products, SPD factorisations and
right-solves, with coefficients that depend on a lower bound chosen up front and not on the data.  Every other tensor takes the
mean task vector through the task-vector job of this module (ratios lam / S), a layer with one source the ratio-1 job.

wudi.wudi_merge (WUDI-Merging; Cheng et al. 2025) lives in wudi.py: the second matrix-aware method and the one ITERATED one, no
reference site, csrc/wudi.hip and the products of csrc/f64ops.hip held to tests/wudi_restatement.py.  Its rule (include/vlm_hip.h),
per 2-D tensor [m, n] with central tensor c, sources W_0 .. W_{S-1} and lam, in float64 with tau_i = W_i - c:
  1. n_i = ||tau_i||_F^2;  G = sum_i tau_i^T tau_i / n_i;  B = sum_i tau_i (tau_i^T tau_i) / n_i
  2. X_0 = sum_i tau_i;  `iters` steps of Adam (lr, 0.9, 0.999, 1e-8) with the gradient 2 (X G - B)
  3. dst = fl32(c + lam * X_iters)
Every other tensor and a layer with one source are treated as for Iso-C.
"""
import ctypes
import math
import struct
from typing import Dict, List, Optional

import torch

from . import _lib as L

# (source template, destination template): vilt_module.py:543-551
_LAYERS = [
    ("transformer.blocks.{i}.attn.{m}.qkv.weight", "transformer.blocks.{i}.attn.qkv.weight", (None,)),
    ("transformer.blocks.{i}.attn.{m}.proj.{n}", "transformer.blocks.{i}.attn.proj.{n}", ("weight", "bias")),
    ("transformer.blocks.{i}.attn.{m}.{n}", "transformer.blocks.{i}.attn.{n}", ("q_bias", "v_bias")),
    ("transformer.blocks.{i}.mlp.{m}.fc1.{n}", "transformer.blocks.{i}.mlp.fc1.{n}", ("weight", "bias")),
    ("transformer.blocks.{i}.mlp.{m}.fc2.{n}", "transformer.blocks.{i}.mlp.fc2.{n}", ("weight", "bias")),
    ("transformer.blocks.{i}.norm1.{m}.{n}", "transformer.blocks.{i}.norm1.{n}", ("weight", "bias")),
    ("transformer.blocks.{i}.norm2.{m}.{n}", "transformer.blocks.{i}.norm2.{n}", ("weight", "bias")),
]
NUM_MERGE_LAYERS = 12  # the reference hard-codes range(12) (:395, :553, :665)


def _tensor_names(i):
    for src_t, dst_t, leaves in _LAYERS:
        for n in leaves:
            yield (lambda m, s=src_t, n=n: s.format(i=i, m=m, n=n)), dst_t.format(i=i, n=n)


def modalities_for_layer(config, i, honour_only_used=True):
    """Which experts feed layer i (vilt_module.py:557-567; regmean's variant :397-404)."""
    loss = config["loss_names"]
    if i < config["vlffn_start_layer_index"]:
        return ["v", "l"]
    if honour_only_used:
        if config["only_activate_used_experts"]:
            if loss.get("irtr", 0) > 0:
                return ["v", "l"]
            if loss.get("vqa", 0) > 0 or loss.get("nlvr2", 0) > 0:
                return ["vl"]
            # the reference leaves modalities=None and dies at len(None) (:569); same error class
            raise TypeError("object of type 'NoneType' has no len()")
        return ["v", "l", "vl"]
    if loss.get("irtr", 0) > 0:
        return ["v", "l"]
    if loss.get("vqa", 0) > 0:
        return ["vl"]
    return ["v", "l", "vl"]


def interpolation_ratios(modalities, merge_ratio):
    """vilt_module.py:569-584 (python doubles; rounded to fp32 when they meet the tensor)."""
    if len(modalities) == 1:
        return {modalities[0]: 1}
    if len(modalities) == 3:
        return {"v": (2 / 3) * merge_ratio, "l": (2 / 3) * (1 - merge_ratio), "vl": 1 / 3}
    return {"v": merge_ratio, "l": 1 - merge_ratio}


class _Plan:
    """A device-resident job table of the merge family (csrc/chunk_plan.h): build with add(), upload once, run() enqueues the
    kernels.  A subclass gives its ctypes job type, its three entry points and how often a run streams the inputs, and writes
    an add() that hands _add() a `fill(job)` for the fields of its own."""

    KIND = GPU_ONLY = JOB = BYTES = UPLOAD = RUN = HEADER = STATE = None
    GROUPS = ("kept",)  # a job's counters: MERGE_MAX_SRC per group, in this order, then `conflict` and `empty`
    PASSES = 1  # how often a run reads every source and the base
    HAS_DST = True  # a job writes one tensor (PairStatsPlan: none)

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.VlmError("%s (got device %s)" % (self.GPU_ONLY, device))
        if self.device.index is None:  # "cuda" names the current device; _dev compares devices, and cuda:0 != cuda would stage a
            self.device = torch.device("cuda", torch.cuda.current_device())  # copy of every tensor that is already there
        self.jobs = []
        self.names: List[Optional[str]] = []
        self.keep = []  # keeps staged tensors alive
        self.total = 0
        self.bytes_read = 0
        self.bytes_written = 0
        self.ws = None

    def _dev(self, t):
        t = t.detach()
        if t.dtype != torch.float32:
            raise L.VlmError("merge expects float32 checkpoints, got %s" % t.dtype)
        if t.device != self.device or not t.is_contiguous() or (t.data_ptr() & 15):
            t = t.to(self.device, copy=True).contiguous()
        self.keep.append(t)
        return t

    def _same_shape(self, tensors):
        for t in tensors:
            if t.shape != tensors[0].shape:
                raise L.VlmError("merge sources disagree in shape: %s vs %s" % (t.shape, tensors[0].shape))

    def _add(self, fill, srcs, base=None, out=None, name=None):
        """The part of add() every method shares: stages the sources and the base, checks their count and shapes, allocates
        `out` or checks the one given, fills the job's dst / base / src / n_src / n_elem, has `fill(job)` set the method's own
        fields (if it raises, the plan has no new job) and appends the job.  Returns `out`.  A plan without HAS_DST has no
        output: nothing is allocated, the job has no dst, nothing is counted as written, and None is returned."""
        srcs = [self._dev(s) for s in srcs]
        if not 1 <= len(srcs) <= L.MERGE_MAX_SRC:
            raise L.VlmError("a %s job takes 1 .. %d sources, got %d" % (self.KIND, L.MERGE_MAX_SRC, len(srcs)))
        ins = srcs if base is None else srcs + [self._dev(base)]
        self._same_shape(ins)
        if not self.HAS_DST:
            out = None
        elif out is None:
            out = torch.empty_like(srcs[0])
        else:
            self._same_shape([srcs[0], out])
            if out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() or (out.data_ptr() & 15):
                raise L.VlmError("a %s output must be a contiguous, 16-byte aligned float32 tensor on %s" % (self.KIND, self.device))
        if self.HAS_DST:
            self.keep.append(out)
        n = srcs[0].numel()
        job = self.JOB()
        if self.HAS_DST:
            job.dst = out.data_ptr()
        job.base = 0 if base is None else ins[-1].data_ptr()
        for k, s in enumerate(srcs):
            job.src[k] = s.data_ptr()
        job.n_src = len(srcs)
        job.n_elem = n
        fill(job)
        self.jobs.append(job)
        self.names.append(name)
        self.total += n
        # what the passes move: each reads every source and the base once (TIES never stores the task vectors; its histograms,
        # thresholds and counters, 16 KiB per source and tensor, are not counted; DARE's mask costs nothing)
        self.bytes_read += self.PASSES * 4 * n * len(ins)
        self.bytes_written += 4 * n if self.HAS_DST else 0
        return out

    def upload(self):
        lib = L.get_lib()
        n = len(self.jobs)
        arr = (self.JOB * n)(*self.jobs)
        nbytes = getattr(lib, self.BYTES)(n, self.total)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.check(getattr(lib, self.UPLOAD)(arr, n, L.ptr(self.ws), nbytes, L.stream_ptr()), self.UPLOAD)
        return self

    def run(self):
        if self.ws is None:
            self.upload()
        with torch.cuda.device(self.device):
            L.check(getattr(L.get_lib(), self.RUN)(L.ptr(self.ws), L.stream_ptr()), self.RUN)

    def _header(self):
        """The workspace header after a run (this synchronises)."""
        if self.ws is None:
            raise L.VlmError("%s.report() needs a plan that has run" % type(self).__name__)
        return self.HEADER.from_buffer_copy(self.ws[: ctypes.sizeof(self.HEADER)].cpu().numpy().tobytes())

    def _structs(self, TYPE, offset, count):
        """`count` structs of the ctypes TYPE at `offset` of the workspace, as the device left them (this synchronises)."""
        size = ctypes.sizeof(TYPE)
        raw = self.ws[offset: offset + size * count].cpu().numpy().tobytes()
        return [TYPE.from_buffer_copy(raw[i * size: (i + 1) * size]) for i in range(count)]

    def _read(self):
        """The workspace header after a run (this synchronises) and, per job, the start of its report row and the counters TIES,
        DARE, DELLA and the band merge share: per group of GROUPS one count per source (how many entries each source kept; band
        merge: how many it lost as outliers), then the elements whose kept entries disagree in sign and the elements nothing
        contributes to."""
        hdr = self._header()
        width = len(self.GROUPS) * L.MERGE_MAX_SRC + 2
        counters = self.ws[hdr.counters_off: hdr.counters_off + 8 * width * hdr.n_jobs].cpu().numpy().view("<u8").reshape(-1, width)
        rows = []
        for i, job in enumerate(self.jobs):
            counts = {g: [int(counters[i, k * L.MERGE_MAX_SRC + m]) for m in range(job.n_src)] for k, g in enumerate(self.GROUPS)}
            counts.update(conflict=int(counters[i, width - 2]), empty=int(counters[i, width - 1]))
            rows.append(({"dst": self.names[i], "n": int(job.n_elem)}, counts))
        return hdr, rows

    def _state(self, hdr):
        """The selection state after a run, per job: one row of STATE's 32-bit words per source (TIES, band merge)."""
        size = ctypes.sizeof(self.STATE)
        state = self.ws[hdr.state_off: hdr.state_off + size * hdr.n_units].cpu().numpy().view("<u4").reshape(-1, size // 4)
        first = 0
        for job in self.jobs:
            yield state[first: first + job.n_src]
            first += job.n_src


class MergePlan(_Plan):
    """The job table of csrc/merge.hip; run() launches one kernel."""

    KIND, GPU_ONLY, JOB = "merge", "the merge kernel runs on the GPU only", L.MergeJob
    BYTES, UPLOAD, RUN = "vlm_merge_plan_bytes", "vlm_merge_plan_upload", "vlm_merge_run"

    def add(self, mode, srcs, ratios, base=None, out=None):
        def fill(job):
            for k in range(job.n_src):
                job.ratio[k] = float(ratios[k]) if ratios is not None else 1.0
            job.mode = mode
        return self._add(fill, srcs, base if mode == L.MERGE_TASKVEC else None, out)


def _passthrough(state_dict):
    # vilt_module.py:537-541: same tensor objects, not copies
    return {k: v for k, v in state_dict.items() if "transformer.blocks." not in k or "gamma" in k}


def _collect(state_dict, src, dst, modalities):
    """Return (list of present sources | None, passthrough tensor | None) with the reference's break rule."""
    srcs = []
    for m in modalities:
        name = src(m)
        if name in state_dict:
            srcs.append((m, state_dict[name]))
        else:
            return None, state_dict[dst]  # KeyError if neither exists, as in the reference (:597-599)
    return srcs, None


def _walk(state_dict, config, central=None, honour_only_used=True, want=None):
    """The one walk over layers and tensor names: yields (dst, mods, srcs | None, through) in the reference's key order, `srcs`
    as _collect returns them.  `central[dst]` is read BEFORE _collect, so a key the central checkpoint lacks raises before a
    pass-through.  `want(dst)` = False skips a name."""
    for i in range(NUM_MERGE_LAYERS):
        mods = modalities_for_layer(config, i, honour_only_used)
        for src, dst in _tensor_names(i):
            if want is not None and not want(dst):
                continue
            if central is not None:
                central[dst]
            srcs, through = _collect(state_dict, src, dst, mods)
            yield dst, mods, srcs, through


def _central(central_weight, config):
    """The central checkpoint: the argument, or torch.load(config["central_weight"]); unwrapped from "state_dict"."""
    if central_weight is None:
        from . import checkpoint
        central_weight = checkpoint.load_file(config["central_weight"])
    return central_weight["state_dict"] if "state_dict" in central_weight else central_weight


def _tensors(srcs):
    return [t for _, t in srcs]


def _finish(plan, plan_out, always=False):
    """The tail of every merge: run the plan if it has jobs; `plan_out` receives it then -- `always`: even without jobs."""
    if plan.jobs:
        plan.run()
    if plan_out is not None and (always or plan.jobs):
        plan_out.append(plan)


def merge_weights(state_dict: Dict[str, torch.Tensor], config, device="cuda", plan_out: Optional[list] = None):
    """Interpolation merge (vilt_module.py:533-638)."""
    out = _passthrough(state_dict)
    plan = MergePlan(device)
    for dst, mods, srcs, through in _walk(state_dict, config):
        ratios = interpolation_ratios(mods, config["merge_ratio"])
        if srcs is None:
            out[dst] = through
        else:
            out[dst] = plan.add(L.MERGE_LERP, _tensors(srcs), [ratios[m] for m, _ in srcs])
    _finish(plan, plan_out, always=True)
    return out


def sum_task_vectors(state_dict, config, central_weight=None, device="cuda", plan_out: Optional[list] = None):
    """Task-vector merge (vilt_module.py:640-746).  `central_weight` defaults to torch.load(config[...])."""
    out = _passthrough(state_dict)
    central = _central(central_weight, config)
    plan = MergePlan(device)
    lam = config["sum_lambda"]
    for dst, mods, srcs, through in _walk(state_dict, config, central):
        if srcs is None:
            out[dst] = through
        else:
            r = [1 if len(mods) == 1 else lam] * len(srcs)
            out[dst] = plan.add(L.MERGE_TASKVEC, _tensors(srcs), r, base=central[dst])
    _finish(plan, plan_out, always=True)
    return out


def ties_keep_count(density, n):
    """K of the trim step: max(1, min(n, ceil(density * n))) in python doubles."""
    if not (0.0 < density <= 1.0):  # also rejects NaN
        raise ValueError("TIES density must lie in (0, 1], got %r" % (density,))
    return max(1, min(n, math.ceil(density * n)))


def _key_float(key):
    return struct.unpack("<f", struct.pack("<I", key))[0]


class TiesPlan(_Plan):
    """The job table of csrc/ties.hip; run() enqueues the seven launches of a TIES merge (three histogram passes of the radix
    select, a bin pick after each, the apply pass) without a host synchronisation."""

    KIND, GPU_ONLY, JOB = "TIES", "the TIES kernels run on the GPU only", L.TiesJob
    BYTES, UPLOAD, RUN = "vlm_ties_plan_bytes", "vlm_ties_plan_upload", "vlm_ties_run"
    HEADER, STATE = L.TiesHeader, L.TiesState
    PASSES = 4  # three selection passes + the apply pass: each streams every source and the central tensor once

    def add(self, srcs, base, density=None, lam=1.0, keep=None, name=None):
        """One output tensor.  `density` gives K for every source (ties_keep_count); `keep` = explicit K per source instead."""
        def fill(job):
            ks = [ties_keep_count(density, int(job.n_elem))] * job.n_src if keep is None else keep
            for k in range(job.n_src):
                job.k[k] = int(ks[k])
            job.lam = float(lam)
        return self._add(fill, srcs, base, name=name)

    def report(self):
        """Per job, read back after a run (this synchronises): the threshold per source as a float and as its key, how many
        entries each source kept, the elements whose kept entries disagree in sign, the elements no source contributes to."""
        hdr, rows = self._read()
        out = []
        for (head, counts), job, state in zip(rows, self.jobs, self._state(hdr)):
            keys = [int(k) for k in state[:, 0]]
            out.append({**head, "K": [int(job.k[m]) for m in range(job.n_src)],
                        "threshold": [_key_float(k) for k in keys], "threshold_bits": keys, **counts})
        return out


def _task_vector_merge(plan_type, add, state_dict, config, central_weight, lam, device, plan_out, report_out, delta=True):
    """The driver every method after sum_task_vectors shares: sum_task_vectors' dictionary logic,
    `add(plan, dst, tensors, central, lam, mods)` into a `plan_type(device)` for a tensor with several sources (`lam=None` takes
    config["sum_lambda"]; `mods`: the sources' modality names), the task-vector job with ratio 1 for a layer with ONE source.
    `delta=False` (sphere_merge on the weights) is merge_weights' logic instead: no central checkpoint is read, `add` gets None
    for it, and a layer with ONE source is the LERP job with ratio 1.  `plan_out` receives the plan first, then the MergePlan of
    the single-source layers (each only if it has jobs); `report_out` receives the plan's report()."""
    if lam is None:
        lam = config["sum_lambda"]
    plan = plan_type(device)
    single = MergePlan(plan.device)
    out = _passthrough(state_dict)
    central = _central(central_weight, config) if delta else None
    for dst, mods, srcs, through in _walk(state_dict, config, central):
        if srcs is None:
            out[dst] = through
        elif len(mods) == 1:
            out[dst] = single.add(L.MERGE_TASKVEC if delta else L.MERGE_LERP, _tensors(srcs), [1], base=central[dst] if delta else None)
        else:
            out[dst] = add(plan, dst, _tensors(srcs), central[dst] if delta else None, lam, [m for m, _ in srcs])
    for p in (plan, single):
        _finish(p, plan_out)
    if report_out is not None:
        report_out.extend(plan.report() if plan.jobs else [])
    return out


def ties_merge(state_dict, config, central_weight=None, density=0.2, lam=None, device="cuda", plan_out: Optional[list] = None,
               report_out: Optional[list] = None):
    """TIES merge of the modality experts' task vectors `W_m - central` (no reference site; the rule: include/vlm_hip.h).
    Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors; `lam=None` takes config["sum_lambda"].
    Trimming is per tensor.  A layer with ONE source is not trimmed: it is the task-vector job with ratio 1 that
    sum_task_vectors issues for it.  `plan_out` receives the TiesPlan FIRST whenever a layer has several sources, then the MergePlan of the single-source layers if
    there are any (the order is part of the contract: callers index [0] for the TiesPlan);
    `report_out` receives TiesPlan.report() (reading it back synchronises)."""
    ties_keep_count(density, 1)  # ValueError before any device work
    return _task_vector_merge(TiesPlan, lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, density=density, lam=lam, name=dst),
                              state_dict, config, central_weight, lam, device, plan_out, report_out)


def dare_keep_below(drop):
    """keep_below of the DARE rule: a draw u (32 bits) keeps its entry iff u < floor((1 - drop) * 2**32), in python doubles."""
    if not (0.0 <= drop < 1.0):  # also rejects NaN
        raise ValueError("DARE drop probability must lie in [0, 1), got %r" % (drop,))
    kb = math.floor((1.0 - drop) * 2 ** 32)
    if kb < 1:
        raise ValueError("DARE drop probability %r keeps nothing" % (drop,))
    return kb


def dare_rescale(drop, rescale=True):
    """float32(1 / (1 - drop)): computed in double, rounded once; 1.0 without rescaling."""
    if not rescale:
        return 1.0
    return struct.unpack("<f", struct.pack("<f", 1.0 / (1.0 - drop)))[0]


# how the trimmed entries are combined: DARE's, the band merge's and DELLA's LINEAR / TIES are one pair of values
assert L.DARE_LINEAR == L.BAND_LINEAR == L.DELLA_LINEAR and L.DARE_TIES == L.BAND_TIES == L.DELLA_TIES
_MODES = {"linear": L.DARE_LINEAR, "ties": L.DARE_TIES, L.DARE_LINEAR: L.DARE_LINEAR, L.DARE_TIES: L.DARE_TIES}


def _mode(kind, mode):
    if isinstance(mode, bool) or mode not in _MODES:
        raise L.VlmError("%s mode must be 'linear' or 'ties', got %r" % (kind, mode))
    return _MODES[mode]


def _seed_stream(kind, seed, stream):
    """The Philox key and stream of a DARE or DELLA job."""
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(stream) < 2 ** 32:
        raise L.VlmError("%s seed must fit 64 bits and stream 32 bits, got %r, %r" % (kind, seed, stream))
    return int(seed), int(stream)


class DarePlan(_Plan):
    """The job table of csrc/dare.hip; run() enqueues the counter reset and the one streaming launch of a DARE merge without a
    host synchronisation.  The mask is a function of (seed, stream, source, element) and is never stored."""

    KIND, GPU_ONLY, JOB = "DARE", "the DARE kernel runs on the GPU only", L.DareJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_dare_plan_bytes", "vlm_dare_plan_upload", "vlm_dare_run", L.DareHeader

    def add(self, srcs, base, drop, lam, seed, stream, mode, rescale=True, out=None, name=None):
        """One output tensor.  `out` may be `base` or one of `srcs` (the pass is elementwise) or any tensor that meets none of them."""
        mode = _mode(self.KIND, mode)
        keep_below = dare_keep_below(drop)
        seed, stream = _seed_stream(self.KIND, seed, stream)

        def fill(job):
            job.keep_below = keep_below
            job.seed = seed
            job.mode = mode
            job.lam = float(lam)
            job.rescale = dare_rescale(drop, rescale)
            job.stream = stream
        return self._add(fill, srcs, base, out, name)

    def report(self):
        """Per job, read back after a run (this synchronises): how many entries each source kept, the elements whose kept entries
        disagree in sign, the elements nothing contributes to."""
        _, rows = self._read()
        return [{**head, "keep_below": int(job.keep_below), **counts} for (head, counts), job in zip(rows, self.jobs)]


DARE_STREAMS_PER_LAYER = 13  # the tensor names of a layer (_tensor_names)


def dare_stream(dst):
    """The Philox stream of an output tensor: 13 * layer + its position among the layer's names -- a function of the name alone, so
    a tensor's mask does not depend on which other keys a checkpoint holds."""
    return _DARE_STREAM[dst]


_DARE_STREAM = {dst: DARE_STREAMS_PER_LAYER * i + slot for i in range(NUM_MERGE_LAYERS)
                for slot, (_, dst) in enumerate(_tensor_names(i))}


def dare_merge(state_dict, config, central_weight=None, drop=0.9, lam=None, seed=0, mode="linear", rescale=True, device="cuda",
               plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """DARE merge of the modality experts' task vectors `W_m - central` (no reference site; the rule: include/vlm_hip.h): every
    entry is dropped with probability `drop`, the survivors are scaled by 1 / (1 - drop), then summed (mode "linear") or sign-elected
    and averaged as in TIES (mode "ties").  Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors and ties_merge;
    `lam=None` takes config["sum_lambda"].  A layer with ONE source is not dropped: it is the task-vector job with ratio 1 that
    sum_task_vectors issues for it.  `plan_out` receives the DarePlan FIRST whenever a layer has several sources, then the MergePlan
    of the single-source layers if there are any; `report_out` receives DarePlan.report() (reading it back synchronises)."""
    dare_keep_below(drop)  # ValueError before any device work
    mode = _mode(DarePlan.KIND, mode)
    return _task_vector_merge(
        DarePlan, lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, drop, lam, seed, dare_stream(dst), mode, rescale=rescale, name=dst),
        state_dict, config, central_weight, lam, device, plan_out, report_out)


def band_ranks(n, density, gamma):
    """(k_hi, k_lo) of the band trim, in python doubles: the k_hi = min(n - 1, floor(gamma * n)) largest entries are outliers, the
    band reaches down to the k_lo = min(n, k_hi + max(1, ceil(density * n)))-th largest.  `density` is the fraction kept, `gamma`
    the fraction of largest entries dropped; where the two overlap, the band is whatever lies below the outliers."""
    if not (0.0 < density <= 1.0):  # also rejects NaN
        raise ValueError("band density must lie in (0, 1], got %r" % (density,))
    if not (0.0 <= gamma < 1.0):
        raise ValueError("band gamma must lie in [0, 1), got %r" % (gamma,))
    k_hi = min(n - 1, math.floor(gamma * n))
    return k_hi, min(n, k_hi + max(1, math.ceil(density * n)))


class BandPlan(_Plan):
    """The job table of csrc/band.hip; run() enqueues the seven launches of a band merge (three histogram passes of ONE radix
    select for both ranks of every source, a pick of both bins after each, the apply pass) without a host synchronisation."""

    KIND, GPU_ONLY, JOB = "band", "the band kernels run on the GPU only", L.BandJob
    BYTES, UPLOAD, RUN = "vlm_band_plan_bytes", "vlm_band_plan_upload", "vlm_band_run"
    HEADER, STATE, GROUPS = L.BandHeader, L.BandState, ("kept", "outlier")
    PASSES = 4  # three selection passes + the apply pass, as TIES: the second rank costs no pass of its own

    def add(self, srcs, base, density=None, gamma=0.0, lam=1.0, mode="linear", ranks=None, name=None):
        """One output tensor.  `density` and `gamma` give (k_hi, k_lo) for every source (band_ranks); `ranks` = an explicit
        (k_hi, k_lo) per source instead."""
        mode = _mode(self.KIND, mode)

        def fill(job):
            rs = [band_ranks(int(job.n_elem), density, gamma)] * job.n_src if ranks is None else ranks
            for k in range(job.n_src):
                job.k_hi[k], job.k_lo[k] = int(rs[k][0]), int(rs[k][1])
            job.mode = mode
            job.lam = float(lam)
        return self._add(fill, srcs, base, name=name)

    def report(self):
        """Per job, read back after a run (this synchronises): both ranks and both thresholds per source (as floats and as keys;
        `threshold_hi` is None where k_hi = 0, its key is 0x80000000), how many entries each source kept and lost as outliers,
        the elements whose kept entries disagree in sign, the elements no source contributes to."""
        hdr, rows = self._read()
        out = []
        for (head, counts), job, state in zip(rows, self.jobs, self._state(hdr)):
            S = job.n_src
            lo, hi = [int(k) for k in state[:, 0]], [int(k) for k in state[:, 1]]
            out.append({**head, "k_hi": [int(job.k_hi[m]) for m in range(S)], "k_lo": [int(job.k_lo[m]) for m in range(S)],
                        "threshold_lo": [_key_float(k) for k in lo], "threshold_lo_bits": lo,
                        "threshold_hi": [None if job.k_hi[m] == 0 else _key_float(hi[m]) for m in range(S)],
                        "threshold_hi_bits": hi, **counts})
        return out


def band_merge(state_dict, config, central_weight=None, density=0.9, gamma=0.01, mode="linear", lam=None, device="cuda",
               plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """Model Breadcrumbs merge (Davari & Belilovsky 2023) of the modality experts' task vectors `W_m - central` (no reference
    site; the rule: include/vlm_hip.h): per tensor and expert the `gamma` share of largest-magnitude entries (the outliers) and
    everything below the band of `density` under them (the noise) are dropped; what is left is summed (mode "linear") or
    sign-elected and averaged as in TIES (mode "ties": breadcrumbs_ties).  gamma = 0 with mode "linear" is magnitude-pruned task
    arithmetic, gamma = 0 with mode "ties" is TIES.  Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors,
    ties_merge and dare_merge; `lam=None` takes config["sum_lambda"].  A layer with ONE source is not trimmed: it is the
    task-vector job with ratio 1 that sum_task_vectors issues for it.  `plan_out` receives the BandPlan FIRST whenever a layer has
    several sources, then the MergePlan of the single-source layers if there are any; `report_out` receives BandPlan.report()
    (reading it back synchronises)."""
    band_ranks(1, density, gamma)  # ValueError before any device work
    mode = _mode(BandPlan.KIND, mode)
    return _task_vector_merge(
        BandPlan, lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, density=density, gamma=gamma, lam=lam, mode=mode, name=dst),
        state_dict, config, central_weight, lam, device, plan_out, report_out)


def della_window(density, epsilon):
    """(keep_lo, keep_hi) of the DELLA rule, in python doubles: inside a row the keep probability rises linearly with the rank of
    an entry's magnitude, from density - epsilon (a draw u keeps the smallest entry iff u < keep_lo = floor((density - epsilon) *
    2**32)) to density + epsilon (keep_hi = floor((density + epsilon) * 2**32))."""
    if not (epsilon >= 0.0 and density - epsilon > 0.0 and density + epsilon <= 1.0):  # also rejects NaN
        raise ValueError("DELLA needs epsilon >= 0 and 0 < density - epsilon, density + epsilon <= 1, got density %r, epsilon %r"
                         % (density, epsilon))
    keep_lo, keep_hi = math.floor((density - epsilon) * 2 ** 32), math.floor((density + epsilon) * 2 ** 32)
    if keep_lo < 1:
        raise ValueError("DELLA density %r - epsilon %r keeps nothing of the smallest entries" % (density, epsilon))
    return keep_lo, keep_hi


def della_row_len(tensor):
    """The row of the DELLA rank: the last dimension of a matrix (or of anything with more dimensions), a vector as a whole."""
    return int(tensor.shape[-1]) if tensor.dim() >= 2 else int(tensor.numel())


class DellaPlan(_Plan):
    """The job table of csrc/della.hip; run() enqueues the counter reset and the one streaming launch of a DELLA merge without a
    host synchronisation.  The ranks are made in LDS and the mask is a function of (seed, stream, source, element, rank): neither
    is stored."""

    KIND, GPU_ONLY, JOB = "DELLA", "the DELLA kernel runs on the GPU only", L.DellaJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_della_plan_bytes", "vlm_della_plan_upload", "vlm_della_run", L.DellaHeader

    def add(self, srcs, base, density=None, epsilon=None, lam=1.0, seed=0, stream=0, mode="linear", rescale=True, row_len=None,
            window=None, name=None):
        """One output tensor.  `density` and `epsilon` give the window (della_window); `window` = an explicit (keep_lo, keep_hi)
        instead.  `row_len` defaults to della_row_len of the first source and may not exceed DELLA_MAX_ROW."""
        mode = _mode(self.KIND, mode)
        keep_lo, keep_hi = della_window(density, epsilon) if window is None else (int(window[0]), int(window[1]))
        if not 1 <= keep_lo <= keep_hi <= 2 ** 32:
            raise L.VlmError("a DELLA window needs 1 <= keep_lo <= keep_hi <= 2**32, got %r" % ((keep_lo, keep_hi),))
        seed, stream = _seed_stream(self.KIND, seed, stream)
        rl = della_row_len(srcs[0]) if row_len is None else int(row_len)
        if not 1 <= rl <= L.DELLA_MAX_ROW:
            raise L.VlmError("a DELLA row holds 1 .. %d entries, got %d" % (L.DELLA_MAX_ROW, rl))
        if srcs[0].numel() % rl:
            raise L.VlmError("DELLA row length %d does not divide the tensor's %d entries" % (rl, srcs[0].numel()))

        def fill(job):
            job.keep_lo, job.keep_hi = keep_lo, keep_hi
            job.seed = seed
            job.row_len = rl
            job.mode = mode
            job.rescale = 1 if rescale else 0
            job.lam = float(lam)
            job.stream = stream
        return self._add(fill, srcs, base, name=name)

    def report(self):
        """Per job, read back after a run (this synchronises): the window, the row length, how many entries each source kept, the
        elements whose kept entries disagree in sign, the elements nothing contributes to."""
        _, rows = self._read()
        return [{**head, "keep_lo": int(job.keep_lo), "keep_hi": int(job.keep_hi), "row_len": int(job.row_len), **counts}
                for (head, counts), job in zip(rows, self.jobs)]


def della_merge(state_dict, config, central_weight=None, density=0.2, epsilon=0.1, mode="linear", lam=None, seed=0, rescale=True,
                device="cuda", plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """DELLA merge (Deep et al. 2024) of the modality experts' task vectors `W_m - central` (no reference site; the rule:
    include/vlm_hip.h): inside every row of a tensor (a vector is one row) the entries are ranked by magnitude and dropped with a
    probability that falls linearly with the rank -- the smallest is kept with probability density - epsilon, the largest with
    density + epsilon --, the survivors are scaled by the reciprocal of their own keep probability, then summed (mode "linear") or
    sign-elected and averaged as in TIES (mode "ties").  epsilon = 0 is DARE with drop = 1 - density.  The draws are DARE's: the
    stream of a tensor is dare_stream(dst).  Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors, ties_merge
    and dare_merge; `lam=None` takes config["sum_lambda"].  A layer with ONE source is not dropped: it is the task-vector job with
    ratio 1 that sum_task_vectors issues for it.  `plan_out` receives the DellaPlan FIRST whenever a layer has several sources,
    then the MergePlan of the single-source layers if there are any; `report_out` receives DellaPlan.report() (reading it back
    synchronises)."""
    della_window(density, epsilon)  # ValueError before any device work
    mode = _mode(DellaPlan.KIND, mode)
    return _task_vector_merge(
        DellaPlan,
        lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, density, epsilon, lam, seed, dare_stream(dst), mode, rescale=rescale, name=dst),
        state_dict, config, central_weight, lam, device, plan_out, report_out)


class StockPlan(_Plan):
    """The job table of csrc/stock.hip; run() enqueues the three launches of a Model Stock merge (the reducer of the task
    vectors' squared norms and dot products, the fold that ends in the ratio of step 3, the apply pass that reads it) without a
    host synchronisation.  Step 3 runs on the device, in correctly rounded f64; there are no counters."""

    KIND, GPU_ONLY, JOB = "Model Stock", "the Model Stock kernels run on the GPU only", L.StockJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_stock_plan_bytes", "vlm_stock_plan_upload", "vlm_stock_run", L.StockHeader
    PASSES = 2  # the reducer and the apply pass: each streams every source and the central tensor once

    def add(self, srcs, base, name=None):
        """One output tensor; the method has no parameter."""
        return self._add(lambda job: None, srcs, base, name=name)

    def results(self):
        """The raw vlm_stock_result_t of every job as the device left it (this synchronises)."""
        return self._structs(L.StockResult, self._header().results_off, len(self.jobs))

    def report(self):
        """Per job, read back after a run (this synchronises): `sq` per source; per pair (a, b), a < b, in the order of their
        slots, `dot` and `cosine`; the mean cosine `cos` (unclamped), the ratio `t`, and `scale` = float32(t / S) as a float and
        as its bits -- all as the device made them."""
        rows = []
        for name, job, r in zip(self.names, self.jobs, self.results()):
            S = job.n_src
            pairs = [{"a": a, "b": b, "dot": r.dot[L.pair_slot(a, b)], "cosine": r.cos_pair[L.pair_slot(a, b)]}
                     for b in range(1, S) for a in range(b)]
            rows.append({"dst": name, "n": int(job.n_elem), "sq": [r.sq[m] for m in range(S)], "pairs": pairs, "cos": r.cos,
                         "t": r.t, "scale": float(r.scale), "scale_bits": float32_bits(r.scale)})
        return rows


def stock_merge(state_dict, config, central_weight=None, device="cuda", plan_out: Optional[list] = None,
                report_out: Optional[list] = None):
    """Model Stock merge (Jang, Yun & Han 2024) of the modality experts (no reference site; the rule: include/vlm_hip.h): per
    tensor, dst = t * mean(W_m) + (1 - t) * central with t = S cos / (1 + (S - 1) cos), cos the mean pairwise cosine between the
    task vectors `W_m - central`, clamped to [0, 1] -- experts that agree keep their average, experts that point apart get the
    central tensor back.  The method has no hyper-parameter: config["sum_lambda"] is NOT read.  Same inputs, keys, pass-through
    and KeyError behaviour as sum_task_vectors and ties_merge.  A layer with ONE source is the task-vector job with ratio 1 that
    sum_task_vectors issues for it (t = 1).  `plan_out` receives the StockPlan FIRST whenever a layer has several sources, then
    the MergePlan of the single-source layers if there are any; `report_out` receives StockPlan.report() (reading it back
    synchronises)."""
    return _task_vector_merge(StockPlan, lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, name=dst),
                              state_dict, config, central_weight, 1.0, device, plan_out, report_out)


class ScePlan(_Plan):
    """The job table of csrc/sce.hip; run() enqueues the nine launches of an SCE merge (three histogram passes of the radix select
    over the variance of every element's task vectors, a bin pick after each, the reducer of the selected entries' squared norms,
    the fold that ends in the weights of step 5, the apply pass that reads them) without a host synchronisation."""

    KIND, GPU_ONLY, JOB = "SCE", "the SCE kernels run on the GPU only", L.SceJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_sce_plan_bytes", "vlm_sce_plan_upload", "vlm_sce_run", L.SceHeader
    PASSES = 5  # three selection passes, the reducer and the apply pass: each streams every source and the central tensor once

    def add(self, srcs, base, density=None, lam=1.0, keep=None, name=None):
        """One output tensor.  `density` gives K (ties_keep_count over all n elements); `keep` = an explicit K instead."""
        def fill(job):
            job.k = ties_keep_count(density, int(job.n_elem)) if keep is None else int(keep)
            job.lam = float(lam)
        return self._add(fill, srcs, base, name=name)

    def results(self):
        """(the raw vlm_sce_result_t, the three counters) of every job as the device left them (this synchronises)."""
        hdr, n = self._header(), len(self.jobs)
        counters = self.ws[hdr.counters_off: hdr.counters_off + 8 * L.SCE_COUNTERS * n].cpu().numpy().view("<u8").reshape(n, L.SCE_COUNTERS)
        return [(r, [int(v) for v in counters[i]]) for i, r in enumerate(self._structs(L.SceResult, hdr.state_off, n))]

    def report(self):
        """Per job, read back after a run (this synchronises): K, the variance threshold as a float and as its key, how many
        elements were selected (`kept`: one count, not one per source), per source `sq` (the energy of its selected entries) and
        `weight` (as a float and as its bits), their total `tot`, the elements whose selected entries disagree in sign and the
        elements where no entry agrees -- all as the device made them."""
        rows = []
        for name, job, (r, (kept, conflict, empty)) in zip(self.names, self.jobs, self.results()):
            S = job.n_src
            rows.append({"dst": name, "n": int(job.n_elem), "K": int(job.k), "threshold": _key_float(r.key), "threshold_bits": int(r.key),
                         "kept": kept, "sq": [r.sq[m] for m in range(S)], "tot": r.tot, "weight": [float(r.w[m]) for m in range(S)],
                         "weight_bits": [float32_bits(r.w[m]) for m in range(S)], "conflict": conflict, "empty": empty})
        return rows


def sce_merge(state_dict, config, central_weight=None, density=0.1, lam=None, device="cuda", plan_out: Optional[list] = None,
              report_out: Optional[list] = None):
    """SCE merge (select, calculate, erase; Wan et al. 2024, mergekit's `sce`) of the modality experts' task vectors `W_m - central`
    (no reference site; the rule: include/vlm_hip.h): per tensor, the `density` share of elements whose task vectors vary most
    across the experts is selected, every expert is weighted by the energy of its selected entries, the entries whose sign loses
    the TIES election are erased and the weighted mean of the rest is added to the central tensor.  Unlike mergekit's form, K counts
    over all n elements (ties_keep_count) and a zero sum elects nothing.  Same inputs, keys, pass-through and KeyError behaviour as
    sum_task_vectors and ties_merge; `lam=None` takes config["sum_lambda"].  A layer with ONE source is the task-vector job with
    ratio 1 that sum_task_vectors issues for it.  `plan_out` receives the ScePlan FIRST whenever a layer has several sources, then
    the MergePlan of the single-source layers if there are any; `report_out` receives ScePlan.report() (reading it back
    synchronises)."""
    ties_keep_count(density, 1)  # ValueError before any device work
    return _task_vector_merge(ScePlan, lambda plan, dst, srcs, c, lam, mods: plan.add(srcs, c, density=density, lam=lam, name=dst),
                              state_dict, config, central_weight, lam, device, plan_out, report_out)


def tall_threshold(tall_lambda):
    """tall_lambda of the consensus rule as a python float: a number >= 0 (an expert's entry is relevant to it iff its magnitude is
    at least tall_lambda times the magnitude of the other experts' sum there)."""
    if isinstance(tall_lambda, bool) or not isinstance(tall_lambda, (int, float)) or not (tall_lambda >= 0.0):  # also rejects NaN
        raise ValueError("tall_lambda must be a number >= 0, got %r" % (tall_lambda,))
    return float(tall_lambda)


def consensus_k(k, S=None):
    """k of the consensus rule for S sources: an integer in [0, S] (an element is kept iff at least k experts find it relevant).
    S = None: any integer >= 0, for a caller that clamps k per layer (consensus_merge)."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 0 or (S is not None and k > S):
        raise ValueError("consensus k must be an integer in [0, %s], got %r" % ("S" if S is None else S, k))
    return k


def tall_mask_words(n):
    """32-bit words of a packed mask of n elements."""
    return (int(n) + 31) // 32


def _packed_mask(mask, n, device):
    """`mask` as a restore job reads it: an int32 tensor of ceil(n / 32) words, flat, contiguous and 16-byte aligned on `device` (a
    CPU tensor is copied there); VlmError if it is not a mask of n elements."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.numel() != tall_mask_words(n):
        raise L.VlmError("a mask for %d elements is an int32 tensor of %d words, got %s" % (
            n, tall_mask_words(n), "%s x %d" % (mask.dtype, mask.numel()) if isinstance(mask, torch.Tensor) else type(mask).__name__))
    mask = mask.detach().reshape(-1)
    if mask.device != device or not mask.is_contiguous() or (mask.data_ptr() & 15):
        mask = mask.to(device, copy=True).contiguous()
    return mask


class _MaskedPlan(_Plan):
    """A plan whose jobs have packed masks (csrc/mask_chunk.h): a merge job writes none or one per source, a restore job reads
    one.  self.masks[job] holds a merge job's mask tensors (int32, ceil(n / 32) words per source; None without masks) or the one
    mask a restore job reads.  A subclass's add() and add_restore() validate their own arguments and hand the two helpers a
    `fill(job)` for the fields of their own."""

    def __init__(self, device):
        super().__init__(device)
        self.masks: List[Optional[List[torch.Tensor]]] = []

    def _add_masked(self, fill, srcs, base, masks, out, name):
        """A merge job: _add, and with `masks` one int32 tensor of ceil(n / 32) words per source, allocated here, in job.mask."""
        n = srcs[0].numel()
        made = [torch.empty(tall_mask_words(n), dtype=torch.int32, device=self.device) for _ in srcs] if masks else None

        def fill_masks(job):
            fill(job)
            for m in range(job.n_src if made else 0):
                job.mask[m] = made[m].data_ptr()
        out = self._add(fill_masks, srcs, base, out, name)
        self.masks.append(made)
        self.bytes_written += 4 * tall_mask_words(n) * len(srcs) if made else 0
        return out

    def _add_restore(self, fill, unified, base, mask, out, name):
        """A restore job: _add with the one source `unified`, and `mask` (_packed_mask) in job.mask[0]."""
        n = unified.numel()
        mask = _packed_mask(mask, n, self.device)

        def fill_mask(job):
            fill(job)
            job.mask[0] = mask.data_ptr()
        out = self._add(fill_mask, [unified], base, out, name)
        self.masks.append([mask])
        self.bytes_read += 4 * tall_mask_words(n)
        return out


TALL_OPS = {L.TALL_CONSENSUS: "consensus", L.TALL_RESTORE: "restore"}


class TallPlan(_MaskedPlan):
    """The job table of csrc/tall.hip; run() enqueues the counter reset and the one streaming launch that serves both ops -- the
    consensus merge (add) and the restore of one expert from the unified tensor, the central tensor and a packed mask
    (add_restore) -- without a host synchronisation.  self.masks: _MaskedPlan's."""

    KIND, GPU_ONLY, JOB = "consensus", "the consensus kernel runs on the GPU only", L.TallJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_tall_plan_bytes", "vlm_tall_plan_upload", "vlm_tall_run", L.TallHeader

    def add(self, srcs, base, tall_lambda, k, lam=1.0, masks=False, out=None, name=None):
        """One output tensor.  `out` may be `base` or one of `srcs` (the pass is elementwise) or any tensor that meets none of them.
        `masks=True` allocates one int32 tensor of ceil(n / 32) words per source, kept in self.masks[job]; every run writes every
        word of them."""
        tall_lambda = tall_threshold(tall_lambda)
        k = consensus_k(k, len(srcs))

        def fill(job):
            job.op = L.TALL_CONSENSUS
            job.k = k
            job.tall_lambda = tall_lambda
            job.lam = float(lam)
        return self._add_masked(fill, srcs, base, masks, out, name)

    def add_restore(self, unified, base, mask, out=None, name=None):
        """One expert's tensor: out[i] = bit i of `mask` ? unified[i] : base[i].  `mask`: an int32 tensor of ceil(n / 32) words (a CPU
        tensor is copied to the device)."""
        def fill(job):
            job.op = L.TALL_RESTORE
            job.k, job.tall_lambda, job.lam = 0, 0.0, 1.0
        return self._add_restore(fill, unified, base, mask, out, name)

    def report(self):
        """Per job, read back after a run (this synchronises): `op` ("consensus" | "restore"), `k`, `tall_lambda`, `kept` per source
        (the bits set in its mask; restore: the elements taken from the unified tensor), `selected` (the elements at least k
        experts find relevant) and `empty` (the elements none does)."""
        _, rows = self._read()
        out = []
        for (head, counts), job in zip(rows, self.jobs):
            out.append({**head, "op": TALL_OPS[int(job.op)], "k": int(job.k), "tall_lambda": float(job.tall_lambda),
                        "kept": counts["kept"], "selected": counts["conflict"], "empty": counts["empty"]})
        return out


# dst -> source template of every merged tensor name
_SRC_OF = {dst: src for i in range(NUM_MERGE_LAYERS) for src, dst in _tensor_names(i)}


def _restore(plan_type, add, unified_state_dict, masks, config, central_weight, device, plan_out):
    """The walk tall_restore and emr_restore share, ufo + masks -> all_moe: for every source key in `masks`,
    `add(plan, unified tensor, central tensor, key)` of the destination key's tensors; a layer with ONE source hands the unified
    tensor through under the source key; KeyError for a key of `masks` that names no source of a multi-source layer."""
    out = _passthrough(unified_state_dict)
    central = _central(central_weight, config)
    plan = plan_type(device)
    seen = set()
    for i in range(NUM_MERGE_LAYERS):
        mods = modalities_for_layer(config, i)
        for src, dst in _tensor_names(i):
            if len(mods) == 1:
                out[src(mods[0])] = unified_state_dict[dst]
                continue
            for m in mods:
                key = src(m)
                if key in masks:
                    out[key] = add(plan, unified_state_dict[dst], central[dst], key)
                    seen.add(key)
    missing = [key for key in masks if key not in seen]
    if missing:
        raise KeyError("masks name no source of a multi-source layer: %s" % ", ".join(sorted(missing)[:4]))
    _finish(plan, plan_out)
    return out


def consensus_merge(state_dict, config, central_weight=None, tall_lambda=0.4, k=2, lam=None, masks_out: Optional[dict] = None,
                    device="cuda", plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """Consensus merge (Wang et al. 2024) of the modality experts' task vectors `W_m - central` (no reference site; the rule:
    include/vlm_hip.h): an entry of the summed task vector is added to the central tensor only where at least `k` experts find it
    relevant to themselves -- expert m does where |x_m| >= tall_lambda * |sum of the other experts' entries|.  k = 0 is plain task
    arithmetic; k = 2 removes what one expert alone cares about and what none does.  `k` is an integer >= 0 and is NOT checked
    against a layer's source count: a layer with S sources runs with min(k, S), the one explicit rule by which k is clamped (so
    k = 3 asks for all three experts where there are three and for both where there are two).
    Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors, ties_merge and dare_merge; `lam=None` takes
    config["sum_lambda"].  A layer with ONE source is the task-vector job with ratio 1 that sum_task_vectors issues for it.
    `masks_out`, if a dict, receives {source key (e.g. transformer.blocks.3.attn.v.qkv.weight): int32 device tensor of
    ceil(n / 32) words} for every tensor with several sources: the TALL masks, with which tall_restore rebuilds an approximation
    of every expert from the k = 0 merge.  `plan_out` receives the TallPlan FIRST whenever a layer has several sources, then the
    MergePlan of the single-source layers if there are any; `report_out` receives TallPlan.report() (reading it back
    synchronises)."""
    tall_lambda = tall_threshold(tall_lambda)  # ValueError before any device work
    consensus_k(k)

    def add(plan, dst, srcs, c, lam, mods):
        out = plan.add(srcs, c, tall_lambda, min(k, len(srcs)), lam=lam, masks=masks_out is not None, name=dst)
        if masks_out is not None:
            for m, t in zip(mods, plan.masks[-1]):
                masks_out[_SRC_OF[dst](m)] = t
        return out
    return _task_vector_merge(TallPlan, add, state_dict, config, central_weight, lam, device, plan_out, report_out)


def tall_restore(unified_state_dict, masks, config, central_weight=None, device="cuda", plan_out: Optional[list] = None):
    """ufo + TALL masks -> all_moe: rebuilds an approximation of every modality expert from the unified checkpoint (the k = 0,
    lam = 1 output of consensus_merge: central + the summed task vector), the central checkpoint and the packed masks that
    consensus_merge(masks_out=...) left (no reference site; the restore rule: include/vlm_hip.h).  Returns an all_moe-keyed
    state_dict: for every source key in `masks`, the select `bit ? unified : central` of the destination key's tensors (exactly
    float32(central + mask * task-vector sum), the paper's reconstruction); for a layer with ONE source, the unified tensor itself
    under the source key; non-block keys pass through by identity.  The unified block keys themselves are not returned.  A key of
    `masks` that names no source of a multi-source layer under `config` is a KeyError; a mask whose word count does not fit its
    tensor is a VlmError.  One job per expert and tensor: each re-reads the unified and the central tensor.  `plan_out` receives
    the TallPlan if it has jobs."""
    return _restore(TallPlan, lambda plan, uni, c, key: plan.add_restore(uni, c, masks[key], name=key),
                    unified_state_dict, masks, config, central_weight, device, plan_out)


EMR_OPS = {L.EMR_MERGE: "emr", L.EMR_RESTORE: "restore"}


def emr_rescale(rescale):
    """The rescaler of an EMR restore job as a python float: a finite number >= 0."""
    if isinstance(rescale, bool) or not isinstance(rescale, (int, float)) or not (0.0 <= rescale < float("inf")):  # also rejects NaN
        raise ValueError("an EMR rescaler must be a finite number >= 0, got %r" % (rescale,))
    return float(rescale)


class EmrPlan(_MaskedPlan):
    """The job table of csrc/emr.hip; run() enqueues the one streaming launch that serves both ops -- the EMR merge (add) and the
    restore of one expert from the unified tensor, the central tensor, a packed mask and a rescaler (add_restore) -- and the fold
    that ends in the rescalers, without a host synchronisation.  self.masks: _MaskedPlan's."""

    KIND, GPU_ONLY, JOB = "EMR", "the EMR kernels run on the GPU only", L.EmrJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_emr_plan_bytes", "vlm_emr_plan_upload", "vlm_emr_run", L.EmrHeader

    def add(self, srcs, base, lam=1.0, masks=False, out=None, name=None):
        """One output tensor.  `out` may be `base` or one of `srcs` (the pass is elementwise) or any tensor that meets none of them.
        `masks=True` allocates one int32 tensor of ceil(n / 32) words per source, kept in self.masks[job]; every run writes every
        word of them."""
        def fill(job):
            job.op = L.EMR_MERGE
            job.lam, job.rescale = float(lam), 0.0
        return self._add_masked(fill, srcs, base, masks, out, name)

    def add_restore(self, unified, base, mask, rescale, out=None, name=None):
        """One expert's tensor: out[i] = base[i] + rescale * (bit i of `mask` ? unified[i] - base[i] : 0).  `mask`: an int32 tensor
        of ceil(n / 32) words (a CPU tensor is copied to the device); `rescale`: a finite number >= 0."""
        rescale = emr_rescale(rescale)

        def fill(job):
            job.op = L.EMR_RESTORE
            job.lam, job.rescale = 1.0, rescale
        return self._add_restore(fill, unified, base, mask, out, name)

    def results(self):
        """The raw vlm_emr_result_t of every job as the device left it (this synchronises)."""
        return self._structs(L.EmrResult, self._header().results_off, len(self.jobs))

    def report(self):
        """Per job, read back after a run (this synchronises): `op` ("emr" | "restore"), `kept` per source (the bits set in its
        mask; restore: the elements taken from the unified tensor), `zero` (the elements whose task vectors sum to zero: nothing is
        elected there), `conflict` (the elements whose task vectors disagree in sign), per source `abs_sum` (the L1 mass of its
        task vector) and `uni_sum` (that of the masked unified task vector), and `rescale` = float32(abs_sum / uni_sum) as python
        floats that print the fp32 values exactly -- all as the device made them.  A restore job has one `kept` and empty lists."""
        rows = []
        for name, job, r in zip(self.names, self.jobs, self.results()):
            S = job.n_src if job.op == L.EMR_MERGE else 0
            rows.append({"dst": name, "n": int(job.n_elem), "op": EMR_OPS[int(job.op)], "kept": [int(r.kept[m]) for m in range(job.n_src)],
                         "zero": int(r.zero), "conflict": int(r.conflict), "abs_sum": [r.abs_sum[m] for m in range(S)],
                         "uni_sum": [r.uni_sum[m] for m in range(S)], "rescale": [float(r.rescale[m]) for m in range(S)]})
        return rows


def emr_merge(state_dict, config, central_weight=None, lam=None, masks_out: Optional[dict] = None, rescalers_out: Optional[dict] = None,
              device="cuda", plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """EMR-Merging (Huang et al. 2024: elect, mask, rescale) of the modality experts' task vectors `W_m - central` (no reference
    site; the rule: include/vlm_hip.h): per element the sign of the summed task vectors is elected, the unified task vector takes
    the largest magnitude among the experts that agree with it, and central + lam * that is the merged tensor.  Per expert the
    method also leaves an agreement mask (one bit per element) and one scalar per tensor, the rescaler, which gives the masked
    unified task vector the L1 mass of the expert's own: with them emr_restore rebuilds an approximation of every expert from the
    lam = 1 merge.  Tuning-free: there is no parameter beside lam.  Two departures from the paper's code: rescalers are per tensor,
    not per model (layers have different expert sets), and an element whose task vectors sum to zero contributes nothing.
    Same inputs, keys, pass-through and KeyError behaviour as sum_task_vectors, ties_merge and consensus_merge; `lam=None` takes
    config["sum_lambda"].  A layer with ONE source is the task-vector job with ratio 1 that sum_task_vectors issues for it.
    `masks_out`, if a dict, receives {source key (e.g. transformer.blocks.3.attn.v.qkv.weight): int32 device tensor of
    ceil(n / 32) words} for every tensor with several sources; `rescalers_out`, if a dict, {source key: python float, the fp32
    rescaler exactly} (reading it back synchronises).  `plan_out` receives the EmrPlan FIRST whenever a layer has several sources,
    then the MergePlan of the single-source layers if there are any; `report_out` receives EmrPlan.report() (reading it back
    synchronises)."""
    keys = []

    def add(plan, dst, srcs, c, lam, mods):
        out = plan.add(srcs, c, lam=lam, masks=masks_out is not None, name=dst)
        keys.append([_SRC_OF[dst](m) for m in mods])
        if masks_out is not None:
            masks_out.update(zip(keys[-1], plan.masks[-1]))
        return out
    plans = []
    out = _task_vector_merge(EmrPlan, add, state_dict, config, central_weight, lam, device, plans, report_out)
    if plan_out is not None:
        plan_out.extend(plans)
    if rescalers_out is not None and keys:
        for ks, r in zip(keys, plans[0].results()):
            rescalers_out.update((key, float(r.rescale[m])) for m, key in enumerate(ks))
    return out


def emr_restore(unified_state_dict, masks, rescalers, config, central_weight=None, device="cuda", plan_out: Optional[list] = None):
    """ufo + EMR masks and rescalers -> all_moe: rebuilds an approximation of every modality expert from the unified checkpoint
    (the lam = 1 output of emr_merge), the central checkpoint and what emr_merge(masks_out=..., rescalers_out=...) left (no
    reference site; the restore rule: include/vlm_hip.h).  Returns an all_moe-keyed state_dict: for every source key in `masks`,
    central + rescaler * (bit ? unified - central : 0) of the destination key's tensors; for a layer with ONE source, the unified
    tensor itself under the source key; non-block keys pass through by identity.  The unified block keys themselves are not
    returned.  A key of `masks` that names no source of a multi-source layer under `config` is a KeyError, and so is a key that has
    a mask but no rescaler; a mask whose word count does not fit its tensor is a VlmError.  One job per expert and tensor: each
    re-reads the unified and the central tensor.  `plan_out` receives the EmrPlan if it has jobs."""
    return _restore(EmrPlan, lambda plan, uni, c, key: plan.add_restore(uni, c, masks[key], rescalers[key], name=key),
                    unified_state_dict, masks, config, central_weight, device, plan_out)


SPHERE_STATUS ={L.SPHERE_OK: "ok", L.SPHERE_LINEAR: "linear", L.SPHERE_ZERO: "zero"}


class SpherePlan(_Plan):
    """The job table of csrc/sphere.hip; run() enqueues the four launches of a spherical merge without a host synchronisation:
    for the tensor jobs Model Stock's three (the reducer of the Gram sums, the fold that ends in step 3, the apply pass that reads
    its S coefficients), for the row jobs one launch over tiles of whole rows.  One plan may mix both kinds.  Step 3 -- the
    weighted Karcher mean of the directions, 24 iterations in f64 -- runs on the device."""

    KIND, GPU_ONLY, JOB = "spherical", "the spherical merge kernels run on the GPU only", L.SphereJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_sphere_plan_bytes", "vlm_sphere_plan_upload", "vlm_sphere_run", L.SphereHeader
    PASSES = 2  # a tensor job: the reducer and the apply pass; add() takes one of them back for a row job

    def __init__(self, device):
        super().__init__(device)
        self.coefs: List[Optional[torch.Tensor]] = []  # per job: the coef_out tensor, float32 [groups, MERGE_MAX_SRC], or None

    def add(self, srcs, base, weights, lam=1.0, rows=False, row_len=None, coef_out=False, name=None):
        """One output tensor.  `base`: the central tensor (the sources' task vectors are merged and lam scales the result) or None
        (the sources themselves; lam must be 1).  `weights`: one non-negative number per source, not all zero.  `rows` (or a
        `row_len`): one mean per row -- `row_len` defaults to della_row_len of the first source, may not exceed DELLA_MAX_ROW and
        must divide the tensor.  `coef_out`: keep the float32 coefficients of every group in self.coefs[job]."""
        ws = [float(w) for w in weights]
        if len(ws) != len(srcs) or not all(math.isfinite(w) and w >= 0.0 for w in ws) or not sum(ws) > 0.0:
            raise L.VlmError("a spherical job takes one finite weight >= 0 per source, not all zero; got %r for %d sources" % (weights, len(srcs)))
        if base is None and float(lam) != 1.0:
            raise L.VlmError("a spherical job without a base has no lam (got %r)" % (lam,))
        rl = 0
        if rows or row_len is not None:
            rl = della_row_len(srcs[0]) if row_len is None else int(row_len)
            if not 1 <= rl <= L.DELLA_MAX_ROW:
                raise L.VlmError("a row of the spherical merge holds 1 .. %d entries, got %d" % (L.DELLA_MAX_ROW, rl))
            if srcs[0].numel() % rl:
                raise L.VlmError("row length %d does not divide the tensor's %d entries" % (rl, srcs[0].numel()))
        groups = srcs[0].numel() // rl if rl else 1
        coef = torch.zeros((groups, L.MERGE_MAX_SRC), dtype=torch.float32, device=self.device) if coef_out else None

        def fill(job):
            for k, w in enumerate(ws):
                job.w[k] = w
            job.lam = float(lam)
            job.row_len = rl
            job.coef_out = 0 if coef is None else coef.data_ptr()
        out = self._add(fill, srcs, base, name=name)
        self.coefs.append(coef)
        if rl:  # a row job reads its inputs once
            self.bytes_read -= 4 * srcs[0].numel() * (len(srcs) + (0 if base is None else 1))
        return out

    def results(self):
        """The raw vlm_sphere_result_t of every job as the device left it (this synchronises)."""
        return self._structs(L.SphereResult, self._header().results_off, len(self.jobs))

    def report(self):
        """Per job, read back after a run (this synchronises): `n`, `row_len` (0: one group, the tensor), `weights`, `lam`; a
        tensor job: `sq` per source, `dot` per pair in slot order, `coef64`, `coef32` (as floats and as their bits), `rho`,
        `resid`, `status` ("ok" | "linear" | "zero"); a row job: `rows`, `rows_linear`, `rows_zero`, `resid_max` -- all as the
        device made them."""
        out = []
        for name, job, r in zip(self.names, self.jobs, self.results()):
            S = job.n_src
            row = {"dst": name, "n": int(job.n_elem), "row_len": int(job.row_len), "weights": [job.w[m] for m in range(S)],
                   "lam": float(job.lam)}
            if job.row_len:
                row.update(rows=int(job.n_elem) // int(job.row_len), rows_linear=int(r.rows_linear), rows_zero=int(r.rows_zero),
                           resid_max=r.resid_max)
            else:
                row.update(sq=[r.sq[m] for m in range(S)],
                           pairs=[{"a": a, "b": b, "dot": r.dot[L.pair_slot(a, b)]} for b in range(1, S) for a in range(b)],
                           coef64=[r.coef64[m] for m in range(S)], coef32=[float(r.coef32[m]) for m in range(S)],
                           coef32_bits=[float32_bits(r.coef32[m]) for m in range(S)], rho=r.rho, resid=r.resid,
                           status=SPHERE_STATUS[int(r.status)])
            out.append(row)
        return out


def sphere_merge(state_dict, config, central_weight=None, on="weights", rows=False, lam=None, device="cuda",
                 plan_out: Optional[list] = None, report_out: Optional[list] = None):
    """Spherical merge of the modality experts (no reference site; the rule: include/vlm_hip.h): SLERP for two experts, the
    weighted Karcher mean of the directions for three, scaled by the weighted mean of the norms -- the counterpart of merge_weights
    that keeps the norm where the experts point apart.  The weights are merge_weights': interpolation_ratios(modalities,
    config["merge_ratio"]).  `rows`: one mean per row of a tensor (a vector is one row) instead of one per tensor.
    `on="weights"` merges the experts' weights themselves: merge_weights' inputs, keys, pass-through and KeyError behaviour; no
    central checkpoint is needed and none is read; `lam` must be None.  `on="delta"` merges their task vectors `W_m - central` and
    adds lam times the mean to the central tensor: sum_task_vectors' contract, `lam=None` takes config["sum_lambda"].
    A layer with ONE source is the job merge_weights or sum_task_vectors issues for it (ratio 1).  `plan_out` receives the
    SpherePlan FIRST whenever a layer has several sources, then the MergePlan of the single-source layers if there are any;
    `report_out` receives SpherePlan.report() (reading it back synchronises)."""
    if on not in ("weights", "delta"):
        raise ValueError("sphere_merge merges on 'weights' or on 'delta', got %r" % (on,))
    delta = on == "delta"
    if not delta and lam is not None:
        raise ValueError("sphere_merge on the weights has no lambda (got %r)" % (lam,))

    def add(plan, dst, srcs, c, lam, mods):
        ratios = interpolation_ratios(mods, config["merge_ratio"])
        return plan.add(srcs, c, [ratios[m] for m in mods], lam=lam, rows=rows, name=dst)
    return _task_vector_merge(SpherePlan, add, state_dict, config, central_weight, lam if delta else 1.0, device, plan_out,
                              report_out, delta=delta)


# ------------------------------------------------------------------------------------------------- expert-pair statistics
_PAIR_SUMS =("dot", "dist2", "ssd_sum", "tssd_sum")          # doubles
_PAIR_COUNTS = ("live", "conflict", "tlive", "tconflict")     # integers


def pair_derived(p):
    """The measures derived from a pair's raw sums, in python doubles; None where the denominator is zero."""
    norm = math.sqrt(p["sq_a"] * p["sq_b"])
    return {"l2": math.sqrt(p["dist2"]),
            "cosine": p["dot"] / norm if norm != 0 else None,
            "ssd": 1.0 - p["ssd_sum"] / p["live"] if p["live"] else None,
            "tssd": 1.0 - p["tssd_sum"] / p["tlive"] if p["tlive"] else None,
            "conflict_rate": p["conflict"] / p["live"] if p["live"] else None}


def float32_bits(x):
    """bits(float32(x)) for a python double x."""
    return struct.unpack("<I", struct.pack("<f", x))[0]


class PairStatsPlan(_Plan):
    """The job table of csrc/pairstats.hip; run() enqueues the streaming launch and the fold without a host synchronisation.
    A job reads its sources (and its base) and writes no tensor: add() allocates nothing."""

    KIND, GPU_ONLY, JOB = "pair-statistics", "the pair-statistics kernels run on the GPU only", L.PairStatsJob
    BYTES, UPLOAD, RUN, HEADER = "vlm_pairstats_plan_bytes", "vlm_pairstats_plan_upload", "vlm_pairstats_run", L.PairStatsHeader
    HAS_DST = False

    @staticmethod
    def _keys(tkeys, n_src):
        ks = [0] * n_src if tkeys is None else [int(k) for k in tkeys]
        if len(ks) != n_src or not all(0 <= k < 2 ** 32 for k in ks):
            raise L.VlmError("a pair-statistics job takes one 32-bit threshold key per source, got %r for %d sources" % (tkeys, n_src))
        return ks

    def add(self, srcs, base=None, tkeys=None, name=None):
        """One tensor.  `base`: the central tensor the sources are taken relative to (None: the sources as they are);
        `tkeys`: the threshold key (bits of a non-negative float32) per source for the truncated statistics, default 0."""
        def fill(job):
            for k, key in enumerate(self._keys(tkeys, job.n_src)):
                job.tkey[k] = key
        self._add(fill, srcs, base, name=name)

    def set_tkeys(self, i, tkeys):
        """Other threshold keys for job i: the next run() uploads the plan again (a host synchronisation)."""
        job = self.jobs[i]
        for k, key in enumerate(self._keys(tkeys, job.n_src)):
            job.tkey[k] = key
        self.ws = None

    def report(self):
        """Per job, read back after a run (this synchronises): the raw sums as the device left them -- `sq`, `nnz` per source;
        per pair (a, b), a < b, in the order of their slots, the sums of the rule (include/vlm_hip.h) with both sides' `sq` --
        and the derived measures (pair_derived)."""
        rows = []
        for i, (job, r) in enumerate(zip(self.jobs, self._structs(L.PairStatsResult, self._header().results_off, len(self.jobs)))):
            S = job.n_src
            pairs = []
            for b in range(1, S):
                for a in range(b):
                    k = L.pair_slot(a, b)
                    p = {"a": a, "b": b, "sq_a": r.sq[a], "sq_b": r.sq[b], "dot": r.dot[k], "dist2": r.dist2[k], "ssd_sum": r.ssd[k],
                         "tssd_sum": r.tssd[k], "live": int(r.live[k]), "conflict": int(r.conflict[k]), "tlive": int(r.tlive[k]),
                         "tconflict": int(r.tconflict[k])}
                    p.update(pair_derived(p))
                    pairs.append(p)
            rows.append({"dst": self.names[i], "n": int(job.n_elem), "tkey": [int(job.tkey[m]) for m in range(S)],
                         "sq": [r.sq[m] for m in range(S)], "nnz": [int(r.nnz[m]) for m in range(S)], "pairs": pairs})
        return rows


def rms_tkeys(row, trunc_rms):
    """The threshold keys of a report row for `trunc_rms` = r: bits(float32(r * sqrt(sq_m / n))), in python doubles."""
    return [float32_bits(trunc_rms * math.sqrt(sq / row["n"])) for sq in row["sq"]]


def expert_stats(state_dict, config, central_weight=None, raw=False, trunc_rms=None, device="cuda",
                 plan_out: Optional[list] = None):
    """How far apart the modality experts are, per tensor and over the checkpoint: squared norms, dot products, L2 distance,
    cosine similarity, soft sign dissimilarity (1 - mean |x_a + x_b| / (|x_a| + |x_b|) over the elements where either is
    non-zero), its truncated form and sign-conflict counts between every pair of experts (no reference site; the rule:
    include/vlm_hip.h).  Nothing is merged and no tensor is written.

    The statistics are those of the task vectors `W_m - central`: the walk is sum_task_vectors' (same keys, same pass-through rule,
    same KeyError behaviour; `central_weight` defaults to torch.load(config["central_weight"])).  `raw=True` takes the experts'
    weights as they are, needs no central checkpoint and walks as merge_weights does.  One job per tensor whose sources are all
    present; a layer with ONE source has `sq` and `nnz` only.

    `trunc_rms=r` (r > 0): the truncated statistics count an element only if one of the two entries has a magnitude of at least
    r times its own tensor's root mean square.  The thresholds come from the sums of a first run, so this costs a SECOND pass
    over the checkpoint and a host synchronisation between the two.  With None every threshold is zero: `tssd_sum == ssd_sum`
    and `tlive == live`.

    Returns {"raw", "trunc_rms", "tensors": [row per tensor, in the walk's order], "summary": {pair name: sums and measures}}.
    A row names its sources ("v", "l", "vl"), keys `sq`, `nnz`, `tkey` by them and its pairs by "v-l", "v-vl", "l-vl".  The
    summary adds a pair's raw sums over all tensors (math.fsum for the doubles) and derives the same measures from them.
    Reading the results back synchronises.  `plan_out` receives the PairStatsPlan if it has jobs."""
    if trunc_rms is not None and not (trunc_rms > 0.0 and math.isfinite(trunc_rms)):  # also rejects NaN
        raise ValueError("trunc_rms must be a positive finite number, got %r" % (trunc_rms,))
    plan = PairStatsPlan(device)
    central = None if raw else _central(central_weight, config)
    mods_of = []
    for dst, mods, srcs, through in _walk(state_dict, config, central):
        if srcs is not None:
            plan.add(_tensors(srcs), None if raw else central[dst], name=dst)
            mods_of.append([m for m, _ in srcs])
    rows = []
    if plan.jobs:
        plan.run()
        rows = plan.report()
        if trunc_rms is not None:
            for i, row in enumerate(rows):
                plan.set_tkeys(i, rms_tkeys(row, trunc_rms))
            plan.run()
            rows = plan.report()
        if plan_out is not None:
            plan_out.append(plan)
    tensors = []
    for row, mods in zip(rows, mods_of):
        tensors.append({"dst": row["dst"], "n": row["n"], "sources": mods,
                        **{k: dict(zip(mods, row[k])) for k in ("sq", "nnz", "tkey")},
                        "pairs": {"%s-%s" % (mods[p["a"]], mods[p["b"]]): {k: v for k, v in p.items() if k not in ("a", "b")}
                                  for p in row["pairs"]}})
    summary = {}
    for name in sorted({k for t in tensors for k in t["pairs"]}, key=["v-l", "v-vl", "l-vl"].index):
        ps = [t["pairs"][name] for t in tensors if name in t["pairs"]]
        total = {"tensors": len(ps), "n": sum(t["n"] for t in tensors if name in t["pairs"])}
        total.update({k: math.fsum(p[k] for p in ps) for k in ("sq_a", "sq_b") + _PAIR_SUMS})
        total.update({k: sum(p[k] for p in ps) for k in _PAIR_COUNTS})
        total.update(pair_derived(total))
        summary[name] = total
    return {"raw": bool(raw), "trunc_rms": trunc_rms, "tensors": tensors, "summary": summary}
