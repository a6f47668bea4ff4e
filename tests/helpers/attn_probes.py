"""Attention probes: inputs in which single (query, key) pairs show, a float64 reference, bounds from a rounding count, mutations.

Plain torch on whatever device it is given; nothing of the package is imported.  tests/test_attention_probes_cpu.py proves on
the CPU that the bounds below can see the errors listed under MUTATIONS; tests/test_attention_probes_gpu.py holds the kernels to
the same bounds.

PROBES.  code(p)[c] = 1 if c == p % 64 else 0 (p: the position in index coordinates -- text token t is t, image token i is
pos1 + i), the same for every head, exact in bf16.  One operand is the code, so an output entry is shared by at most ceil(NP / 64)
pairs.  `ints` are dense nonzero integers of [-3, 3] (exact in bf16).
  F   Q = 0, K random, V = code(k), dO = ints.    O[q, c] = sum_{k = c mod 64} P[q, k];  lse[q] = log2 sum_k 2^bias2[q, k]
  BV  Q = 0, dO = code(q), K and V = ints.        dV[k, c] = sum_{q = c mod 64} P[q, k]
  BQ  Q = 0, K = code(k), V and dO = ints.        dQ[q, c] = scale sum_{k = c mod 64} dS[q, k]
  BK  K = 0, Q = code(q), V and dO = ints.        dK[k, c] = scale sum_{q = c mod 64} dS[q, k]
  T   BQ with sparse V and dO, for the table bins only (below).
In all of them Q K^T = 0: the scores are the bias alone, so P depends on the geometry, the mode and the masks only.  With dense
integers every dS[q, k] = P (dP - delta) is nonzero (the CPU test asserts that no query row of BQ / BK has dS identically 0), so
every pair reaches dQ, dK and its table bin.
A table bin, however, sums B NP^2 / R pairs whose gradients are of one size with dense operands, and ONE pair among them cannot
exceed the bin's rounding error at any table scale (all pairs of a bin share the bias value).  Mutation (f) is therefore stated
on probe T alone: V = +-3 code(k) on the comb rows of Case.v_rows (the keys the mutations sit on and a fill), the same in every
sample, and dO = (+-3 on comb rows, +-1 elsewhere) code(q + sample number), so that few pairs per bin carry a gradient.  T shows
that the bins' bound can see a lost pair where the pair carries the bin; it says nothing about most pairs (most dS rows of T are
0), which is what the dense probes are for.
The index and the table are those of build_case in tests/test_attention_gpu.py: a random index in [0, R) per pair, the constant
text -> image (R - 2) and image -> text (R - 1) blocks, a two-layer N(0, 1) table of which layer 1 is used (times 3 for the
dense probes: Case), ragged text masks.

REFERENCE.  float64 restatement of vision_transformer.py:346-358 in the segment-major layout (`reference`, gradients by torch
autograd), with the mask and SEPARATE rules of reference() in tests/test_attention_gpu.py.  The bias is the DOCUMENTED fp16 table
of vlm_attn_desc_t.bias_dense, fp16(fp32(table) * fp32(log2 e)) (attention_fwd.hip:292, checked by test_bias_dense_tables), so
the fp16 rounding of the bias is part of the reference and not of the bound; the table's gradient passes straight through it.
`evaluate` is the same computation written out (P, dP, delta, dS as tensors): it yields the bounds' absolute-value contractions
and takes the mutations; the CPU test holds it to the autograd reference at 1e-12.
A kept-row call (q_keep) and a dead (sample, segment) (row_live) have the reference dO zero on the rows that do not count; only
kept rows of out / lse are compared, and the dQ rows outside the prefixes / the dqkv rows of a dead sample must be exactly 0.
Not covered: a fully masked text segment in SEPARATE mode (the reference yields NaN, the kernel 0); the masks here keep >= 1 key.

BOUNDS.  Each compared entry y = sum_i t_i gets tau = k u A: u = 2^-9 is the unit the counts are stated in, A the reference's
contraction of the absolute values, k the roundings on the path.  ONE round-to-nearest to bf16 costs RB = 2 units: bf16 keeps 8
significant bits, so its relative error is bounded by 2^-8 = 2 u (docs/experiments.md has the measured ratios).
The roundings, read off the kernels (csrc/):
  SLACK = 1/8 (in units of u) stands for every fp32 effect of a path together: an fp32 accumulation of n <= 1 100 terms
      (n 2^-24 <= u / 30), v_exp_f32 (attention_common.h:15, 1 ulp), the fp32 score / exponent arithmetic (2^-22 |lse| ln 2 <= u / 700).
  O:   P -> bf16 before P.V (attention_fwd.hip:204; the hand-placed stream: the v_cvt_pk_bf16_f32 of attention_fwd2_body.inc),
       the row sum is the sum of the SAME rounded weights (attention_fwd.hip:205), so O is a convex combination whose weights
       carry the rounding twice (numerator and sum): 2 RB u P|V|; the store (attention_fwd.hip:233, attention_fwd2.hip:236):
       RB u |O| <= RB u P|V|.  K_O = 3 RB + SLACK, A = P |V|.
  lse: m + log2f(lt) (attention_fwd.hip:236), lt the sum of the bf16-rounded weights: relative error (RB + SLACK) u of lt, i.e.
       log2(e) (RB + SLACK) u absolute, plus the fp32 store 2^-23 |lse|.  (The bound is nearly reached: the constant text -> image
       block gives a text query about n1 keys of ONE weight, which all round the same way.)
  P of the backward = exp2(bias2 - lse) with the FORWARD's lse: relative error ln 2 * (the lse bound above), plus the split of
       -lse into two bf16 terms on the matrix pipe (attention_bwd_dkvb.h:276-277: 2^-16 |lse|; attention_bwd_dq2.h:36-40 keeps
       three terms; the generic kernels take fp32 C operands, attention_bwd.hip:427):  K_P(q) = RB + SLACK + ln 2 |lse| (2^-7 + 2^-14).
  dV:  P (K_P) -> bf16 (attention_bwd_dkvb.h:321, attention_bwd.hip:484): + RB; the store (attention_bwd_dkvb.h:349,
       attention_bwd.hip:519): + RB.  K = K_P + 2 RB + SLACK, A = P^T |dO|.
  delta = rowsum(dO o O) is formed from the bf16-ROUNDED O (attention_bwd.hip:117-119, attention_bwd_dq2.h:183): its error
       K_O u sum_c |dO| (P|V|), plus 2^-16 |delta| for its split into two bf16 terms (attention_bwd_dkvb.h:276-277), together
       u E_delta(q), enters dS as P E_delta -- not proportional to |dS|.
  dS = P (dP - delta): K_P |dS| + P E_delta;  dS -> bf16 before dS.K / dS^T.Q (attention_bwd.hip:253 and :485,
       attention_bwd_dkvb.h:321, attention_dq2_body.inc v_cvt_pk_bf16_f32): + RB; the store (attention_bwd.hip:279,
       attention_bwd_dq2.h:280, attention_bwd_dkvb.h:348, attention_bwd.hip:518): + RB.
       a = P ((K_P + 2 RB + SLACK) |dP - delta| + E_delta);  A_dQ = scale a |K|,  A_dK = scale a^T |Q|.
  column sums: the kernels sum the fp32 values they round for the store (attention_bwd.hip:306, attention_bwd_dkvb.h:350-365):
       tau = the sum of the entries' tau over the segment's rows; the store term the sum does not pay (RB u |y| per entry)
       covers the fp32 fold and its float atomics (<= 2^-24 x 2^15 addends = u |y| at most).
  table gradient: dS is NOT rounded to bf16 on this path (fp32 panel attention_bwd_dkvb.h:309-315; fp32 fma
       attention_bwd.hip:729): a_t = P ((K_P + SLACK) |dP - delta| + E_delta) summed over the bin; the fixed-point step, 2^-46
       (attention_bwd_dkvb.h:392; 2^-48 in attention_bwd.hip:757) of the item's largest value per addend: 2^-45 n_bin max|dS|;
       the float atomics of the items' sums (attention_bwd_dkvb.h:423, attention_bwd.hip:789), <= 128 per bin: 2^-17 sum |dS|.
  The bias itself costs nothing: the reference reads the fp16 table the kernels read (REFERENCE above).

MUTATIONS (applied to `evaluate`, never to a kernel): see `mutations`.  Each must move some compared entry beyond 4 tau.
"""
import math

import torch

U = 2.0 ** -9
LOG2E = 1.4426950408889634
SCALE = 0.125
RB = 2.0             # one round-to-nearest to bf16, in units of U: 8 significant bits, relative error <= 2^-8 = 2 U
SLACK = 0.125
K_O = 3.0 * RB + SLACK
POWER = 4.0          # a mutation must exceed POWER * tau (tests/test_attention_probes_cpu.py)
LAYER = 1
PROBES = ("F", "BV", "BQ", "BK", "T")
TABLE_SHARP = 3.0
F64, BF16 = torch.float64, torch.bfloat16

# id: (B, n0, n1, H, R)
GEOMS = {
    "G1": (9, 40, 145, 2, 300), "G2": (3, 64, 64, 1, 300), "G3": (3, 57, 71, 1, 300), "G4": (3, 72, 65, 2, 300),
    "G5": (2, 0, 130, 1, 300), "G6": (3, 40, 0, 1, 300), "G7": (2, 40, 728, 1, 300), "G8": (2, 40, 729, 1, 300),
    "G9": (2, 40, 984, 1, 300), "G10": (2, 40, 985, 1, 300), "G11": (2, 40, 696, 1, 8191), "G12": (2, 40, 728, 1, 8191),
}


def roundup(x, m):
    return (x + m - 1) // m * m


class Case:
    """One geometry's bias index, table and masks (the same on every device: drawn on the CPU from `seed`)."""

    def __init__(self, gid, device="cpu", with_bias=True, image_mask=False, seed=None, sharp=True):
        self.gid, self.device, self.with_bias, self.sharp = gid, torch.device(device), with_bias, sharp
        B, n0, n1, H, R = GEOMS[gid]
        self.B, self.n0, self.n1, self.H, self.R, self.D = B, n0, n1, H, R, 64 * H
        self.pos1 = roundup(n0, 8)
        self.NP = self.pos1 + n1
        self.N = n0 + n1
        self.rows = B * self.N
        g = torch.Generator(); g.manual_seed(1000 + sorted(GEOMS).index(gid) if seed is None else seed)
        ld = roundup(self.NP, 4)
        idx = torch.randint(0, R, (self.NP, ld), generator=g)
        if n0 and n1:
            idx[:n0, self.pos1:] = R - 2
            idx[self.pos1:, :n0] = R - 1
        self.idx = idx.to(torch.int16).to(self.device)                              # [NP, ld], index (not x 4)
        # fp32, two layers; N(0, 1) as in build_case, times TABLE_SHARP for the dense probes (the issue's remedy for a geometry
        # that misses the power check: with N(0, 1) a neighbouring bias entry or a lost query block moved a 1 024-position
        # entry by 1 .. 3.9 tau only)
        self.table = (torch.randn(R, 2 * H, generator=g) * (TABLE_SHARP if sharp else 1.0)).to(self.device)
        self.pos = torch.cat([torch.arange(n0), self.pos1 + torch.arange(n1)]).to(self.device)   # sequence slot -> position
        self.keep0 = self.keep1 = self.lens = None
        if n0:  # ragged: sample 0 keeps every token, sample 1 the fewest, the others a random number in between
            lens = torch.randint(max(1, n0 // 4), n0, (B,), generator=g)
            lens[0] = n0
            self.lens = lens
            self.keep0 = (torch.arange(n0)[None] < lens[:, None]).to(torch.uint8).contiguous().to(self.device)
        if image_mask:  # as test_attention_with_an_image_keep_mask: the last 37 and three middle image tokens dropped
            keep1 = torch.ones(B, n1, dtype=torch.uint8)
            keep1[:, -37:] = 0
            keep1[0, 50:53] = 0
            self.keep1 = keep1.to(self.device)

    # --- layout -------------------------------------------------------------------------------------------------------------
    def keep(self):
        k = torch.ones(self.B, self.N, dtype=torch.bool, device=self.device)
        if self.keep0 is not None:
            k[:, :self.n0] = self.keep0.bool()
        if self.keep1 is not None:
            k[:, self.n0:] = self.keep1.bool()
        return k

    def to_seq(self, x):
        """segment-major [rows, F] -> [B, N, F]"""
        B, n0, n1 = self.B, self.n0, self.n1
        F = x.shape[-1]
        return torch.cat([x[:B * n0].view(B, n0, F), x[B * n0:].view(B, n1, F)], 1)

    def from_seq(self, y):
        B, n0 = self.B, self.n0
        F = y.shape[-1]
        return torch.cat([y[:, :n0].reshape(B * n0, F), y[:, n0:].reshape(-1, F)], 0)

    def heads(self, x):
        """segment-major [rows, H*64] -> [B, H, N, 64]"""
        return self.to_seq(x).view(self.B, self.N, self.H, 64).permute(0, 2, 1, 3)

    def unheads(self, y):
        return self.from_seq(y.permute(0, 2, 1, 3).reshape(self.B, self.N, self.D))

    def row_mask(self, per_sample):
        """bool [B, N] -> bool [rows]"""
        return self.from_seq(per_sample[..., None])[:, 0]

    def kept_rows(self, q_keep):
        m = torch.zeros(self.B, self.N, dtype=torch.bool, device=self.device)
        m[:, :min(q_keep[0], self.n0)] = True
        m[:, self.n0:self.n0 + min(q_keep[1], self.n1)] = True
        return self.row_mask(m)

    def sample_rows(self, b, segments=(0, 1)):
        m = torch.zeros(self.B, self.N, dtype=torch.bool, device=self.device)
        if 0 in segments:
            m[b, :self.n0] = True
        if 1 in segments:
            m[b, self.n0:] = True
        return self.row_mask(m)

    # --- the bias ---------------------------------------------------------------------------------------------------------------
    def table2(self):
        """[R, H] float64: the documented fp16 value of layer LAYER's table in exponent units (bias * log2 e)."""
        t = self.table[:, LAYER * self.H:(LAYER + 1) * self.H]
        return (t * torch.tensor(LOG2E, dtype=torch.float32)).to(torch.float16).to(F64)

    def bias2(self, t2, dq=0, dk=0):
        """[H, N, N] exponent-unit bias of the pair (q + dq, k + dk) in POSITION coordinates (the neighbouring pair a wrong
        fetch would take, gap positions included; a neighbour past the end of the index is the one on the other side)."""
        if not self.with_bias:
            return torch.zeros(self.H, self.N, self.N, dtype=F64, device=self.device)
        pq = torch.where(self.pos + dq < self.NP, self.pos + dq, self.pos - dq)
        pk = torch.where(self.pos + dk < self.NP, self.pos + dk, self.pos - dk)
        ii = self.idx.long()[pq][:, pk]
        return t2[ii].permute(2, 0, 1)

    def mode_mask(self, sep):
        blk = torch.ones(self.N, self.N, dtype=torch.bool, device=self.device)
        if sep:
            blk[:self.n0, self.n0:] = False
            blk[self.n0:, :self.n0] = False
        return blk

    def v_rows(self, sep):
        """bool [N], the comb: the rows that are nonzero in the sparse operands (V of the backward probes, dO of probe F) and
        carry the large dO values elsewhere -- the keys the mutations sit on (edge_keys: the first and last position of a 32-, a
        64- and a 128-position tile, every sample's last kept text key, the first image key, the last key), the first three rows
        of either segment (where the kept prefixes end), filled up with random rows to 160 R / (B N).  A comb row holds ONE
        integer in one channel; the pairs (q, k) whose dO channel meets a comb key's V channel carry the gradient, and only a few
        of them fall into one table bin (B N^2 / R pairs): few enough for one pair to stand out of its bin's bound."""
        m = torch.zeros(self.N, dtype=torch.bool)
        for kk in edge_keys(self, sep).values():
            m[kk.cpu() if torch.is_tensor(kk) else kk] = True
        m[:min(3, self.n0)] = True
        m[self.n0:self.n0 + min(3, self.n1)] = True
        budget = int(160 * self.R / (self.B * self.N))
        if budget > int(m.sum()):
            g = torch.Generator(); g.manual_seed(5)
            extra = torch.randperm(self.N, generator=g)
            extra = extra[~m[extra]]
            m[extra[: budget - int(m.sum())]] = True
        return m


def case_for(gid, probe, **kw):
    """The case of a probe: the sharp table for the dense probes, the N(0, 1) one for T (its pairs of a bin should be of one size)."""
    return Case(gid, sharp=probe != "T", **kw)


def code(pos):
    return (pos[:, None] % 64 == torch.arange(64, device=pos.device)[None]).to(torch.float32)


def ints(shape, g):
    """integers of [-3, 3] without 0"""
    return torch.randint(1, 4, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def coded_ints(c, g, shift, sep):
    """[B, H, N, 64]: one nonzero integer per row, in channel (position + shift * sample) % 64 -- the pairs (q, k) with
    q + shift * b = k (mod 64) are the ones in which such a dO row meets such a V row"""
    B, H, N = c.B, c.H, c.N
    ch = (c.pos.cpu()[None, :] + shift * torch.arange(B)[:, None]) % 64
    if shift:  # dO: +-3 on the comb rows (the tile edges stand out), +-1 on the others
        val = (torch.randint(0, 2, (B, H, N), generator=g).float() * 2 - 1) * torch.where(c.v_rows(sep), 3.0, 1.0)
    else:  # V: +-3, the same for every sample (the table gradient sums the samples: opposite signs would cancel in a bin)
        val = (3.0 * (torch.randint(0, 2, (1, H, N), generator=g).float() * 2 - 1)).expand(B, H, N)
    return torch.nn.functional.one_hot(ch, 64).float()[:, None] * val[..., None]


def probe_inputs(c, probe, sep):
    """(qkv bf16 [rows, 3 D], dO bf16 [rows, D]) of probe `probe`, segment-major; the same values on every device."""
    g = torch.Generator(); g.manual_seed(77 + 13 * PROBES.index(probe) + sorted(GEOMS).index(c.gid))
    B, N, H = c.B, c.N, c.H
    cd = code(c.pos.cpu())[None, None].expand(B, H, N, 64)
    zero = torch.zeros(B, H, N, 64)
    dense = lambda: ints((B, H, N, 64), g)
    if probe == "F":   # (dO is free here: one channel per row, every row, so that dV[k, c] sums the queries = c mod 64 only)
        q, k, v, do = zero, torch.randn(B, H, N, 64, generator=g) * 1.5, cd, cd * ints((B, H, N, 1), g)
    elif probe == "BV":
        q, k, v, do = zero, dense(), dense(), cd
    elif probe == "BQ":
        q, k, v, do = zero, cd, dense(), dense()
    elif probe == "BK":
        q, k, v, do = cd, zero, dense(), dense()
    elif probe == "T":   # the table bins: BQ with V on the comb and one dO channel per row (Case.v_rows)
        q, k, v, do = zero, cd, coded_ints(c, g, 0, sep) * c.v_rows(sep)[None, None, :, None], coded_ints(c, g, 1, sep)
    else:
        raise ValueError(probe)
    qkv = torch.cat([c.unheads(t.contiguous()) for t in (q, k, v)], 1).to(BF16)   # (the layout helpers take any device)
    return qkv.to(c.device), c.unheads(do.contiguous()).to(BF16).to(c.device)


# ---- the float64 reference (autograd) ------------------------------------------------------------------------------------------
def reference(c, qkv, dout, sep):
    """out [rows, D], lse [H, rows] (log2 domain), dqkv [rows, 3 D], dtable [H, R] (layer LAYER's columns), all float64.
    `dout` is the gradient that COUNTS (zero where a kept-row or dead-sample call says so)."""
    x = qkv.to(F64).requires_grad_(True)
    tab = c.table.to(F64).requires_grad_(True)
    q, k, v = (c.heads(x[:, i * c.D:(i + 1) * c.D]) for i in range(3))
    s = SCALE * (q @ k.transpose(-1, -2))
    if c.with_bias:
        t = tab[:, LAYER * c.H:(LAYER + 1) * c.H]
        t = t + (c.table2() / LOG2E - t).detach()     # the fp16 table the kernels read; gradient straight through
        s = s + c.bias2(t)[None]
    s = s.masked_fill(~c.keep()[:, None, None, :], float("-inf"))
    s = s.masked_fill(~c.mode_mask(sep)[None, None], float("-inf"))
    out = c.unheads(s.softmax(-1) @ v)
    lse = c.unheads(torch.logsumexp(s, -1, keepdim=True).expand(-1, -1, -1, 64))[:, ::64].t() * LOG2E
    (out * dout.to(F64)).sum().backward()
    dtab = tab.grad[:, LAYER * c.H:(LAYER + 1) * c.H].t().contiguous() if c.with_bias else None
    return dict(out=out.detach(), lse=lse.detach().contiguous(), dqkv=x.grad, dbias=dtab)


# ---- the same computation written out: outputs, bounds, mutations ----------------------------------------------------------------
def evaluate(c, qkv, dout, sep, *, mut=None, bounds=True):
    """dict of outputs (out, lse, dq, dk, dv [rows, D]; csq, csv [2, D] per-segment column sums; dbias [H, R]) and, with
    `bounds`, a dict `tau` of the same keys.  `mut`: a mutation of `mutations` (None: the clean computation)."""
    mut = mut or {}
    x = qkv.to(F64)
    q, k, v = (c.heads(x[:, i * c.D:(i + 1) * c.D]) for i in range(3))
    do = c.heads(dout.to(F64))
    t2 = c.table2() if c.with_bias else None
    b2 = c.bias2(t2)
    if "bias_from" in mut:           # (c): the bias of the pairs (., k) taken from the neighbouring pair
        dq_, dk_, cols = mut["bias_from"]
        b2 = b2.clone()
        b2[:, :, cols] = c.bias2(t2, dq_, dk_)[:, :, cols]
    s2 = (SCALE * LOG2E) * (q @ k.transpose(-1, -2)) + b2[None]
    keep = c.keep()
    if "unmask" in mut:              # (d): keep0 longer by one
        keep = keep | mut["unmask"]
    s2 = s2.masked_fill(~keep[:, None, None, :], float("-inf")).masked_fill(~c.mode_mask(sep)[None, None], float("-inf"))
    if "logw" in mut:                # (a) / (b): a key dropped (weight 0) or counted twice (weight 2)
        s2 = s2 + mut["logw"][:, None, None, :]
    lse2 = torch.logsumexp(s2 * math.log(2.0), -1, keepdim=True) * LOG2E
    P = torch.exp2(s2 - lse2)
    O = P @ v
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    G = dP - delta
    dS = P * G
    res_zero_rows = int(((dS.abs().amax(-1) == 0) & keep.any(-1)[:, None, None]).sum())
    Pk, dSk = P, dS
    if "qskip" in mut:               # (e): one 32-query block left out of dK / dV / the table gradient
        live = (~mut["qskip"]).to(F64)[None, None, :, None]
        Pk, dSk = P * live, dS * live
    res = dict(out=c.unheads(O), lse=c.unheads(lse2.expand(-1, -1, -1, 64))[:, ::64].t().contiguous(),
               dq=c.unheads(SCALE * (dS @ k)), dk=c.unheads(SCALE * (dSk.transpose(-1, -2) @ q)),
               dv=c.unheads(Pk.transpose(-1, -2) @ do))
    res["zero_dS_rows"] = res_zero_rows       # (sample, head, query) rows whose dS is identically 0
    nt = c.B * c.n0
    seg_sum = lambda y: torch.stack([y[:nt].sum(0), y[nt:].sum(0)])
    res["csq"], res["csv"] = seg_sum(res["dq"]), seg_sum(res["dv"])
    ii = c.idx.long()[c.pos][:, c.pos].reshape(-1) if c.with_bias else None

    def bins(y):  # [B, H, N, N] -> [H, R]
        return torch.zeros(c.H, c.R, dtype=F64, device=c.device).index_add_(1, ii, y.sum(0).reshape(c.H, -1))

    if c.with_bias:
        res["dbias"] = bins(dSk)
        if "pair" in mut:            # (f): one pair (q, k) left out of its bin -- the q whose dP - delta is largest at key k ...
            kk = mut["pair"]
            # ... among the queries of the key's own segment: the text <-> image pairs share ONE table row by construction
            # (vilt_module.py:180-181), and one pair of that row's B n0 n1 is beyond any bound made of roundings
            own = (torch.arange(c.N, device=c.device) < c.n0) == (kk < c.n0)
            if c.n0 and c.n1:        # (the random index of an own-segment pair can name one of the two shared rows as well)
                own = own & (c.idx.long()[c.pos, c.pos[kk]] < c.R - 2)
            qq = ((G * (P > 0))[:, :, :, kk].abs().sum(0) * own).argmax(1)      # [H]
            for h in range(c.H):
                res["dbias"][h, c.idx[c.pos[qq[h]], c.pos[kk]].long()] -= dSk[:, h, qq[h], kk].sum()
    if not bounds:
        return res
    kP = RB + SLACK + math.log(2.0) * lse2.abs() * (2.0 ** -7 + 2.0 ** -14)          # [B, H, N, 1]
    AO = P @ v.abs()
    Ed = K_O * (do.abs() * AO).sum(-1, keepdim=True) + 2.0 ** -7 * delta.abs()
    a = P * ((kP + 2.0 * RB + SLACK) * G.abs() + Ed)
    tau = dict(out=U * K_O * c.unheads(AO),
               lse=c.unheads((LOG2E * U * (RB + SLACK) + 2.0 ** -23 * lse2.abs()).expand(-1, -1, -1, 64))[:, ::64].t().contiguous(),
               dq=U * SCALE * c.unheads(a @ k.abs()), dk=U * SCALE * c.unheads(a.transpose(-1, -2) @ q.abs()),
               dv=U * c.unheads(((kP + 2.0 * RB + SLACK) * P).transpose(-1, -2) @ do.abs()))
    tau["csq"], tau["csv"] = seg_sum(tau["dq"]), seg_sum(tau["dv"])
    if c.with_bias:
        at = P * ((kP + SLACK) * G.abs() + Ed)
        n_bin = torch.zeros(c.R, dtype=F64, device=c.device).index_add_(0, ii, torch.ones_like(ii, dtype=F64))
        tau["dbias"] = U * bins(at) + 2.0 ** -17 * bins(dS.abs()) + 2.0 ** -45 * n_bin[None] * dS.sum(0).abs().amax((1, 2))[:, None]
    res["tau"] = tau
    return res


OUTPUTS = ("out", "lse", "dq", "dk", "dv", "csq", "csv", "dbias")


def reference_with_bounds(c, qkv, dout, sep):
    """The autograd reference's values with the written-out evaluation's bounds (what the GPU tests compare against)."""
    ev, ref = evaluate(c, qkv, dout, sep), reference(c, qkv, dout, sep)
    D, nt = c.D, c.B * c.n0
    new = dict(out=ref["out"], lse=ref["lse"], dq=ref["dqkv"][:, :D], dk=ref["dqkv"][:, D:2 * D], dv=ref["dqkv"][:, 2 * D:])
    if c.with_bias:
        new["dbias"] = ref["dbias"]
    for name, y in new.items():  # the two must agree far below any bound (the CPU test holds them to 1e-12)
        d = float((y - ev[name]).abs().max())
        assert d <= 1e-11 * max(1.0, float(y.abs().max())), "%s: autograd and written-out evaluation differ by %.3g" % (name, d)
    new["csq"] = torch.stack([new["dq"][:nt].sum(0), new["dq"][nt:].sum(0)])
    new["csv"] = torch.stack([new["dv"][:nt].sum(0), new["dv"][nt:].sum(0)])
    ev.update(new)
    return ev


def worst_ratio(got, ref, rows=None):
    """{output: max |got - ref| / tau}; entries whose tau is 0 must be equal (ratio 0 or inf).  `rows`: bool [rows], the rows of
    out / lse that are compared (kept-row calls)."""
    r = {}
    for name in OUTPUTS:
        if name not in ref or ref[name] is None or name not in got:
            continue
        e, t = (got[name].to(F64) - ref[name]).abs(), ref["tau"][name]
        if rows is not None and name == "out":
            e, t = e[rows], t[rows]
        if rows is not None and name == "lse":
            e, t = e[:, rows], t[:, rows]
        ratio = torch.where(e == 0, torch.zeros_like(e), e / t)
        r[name] = float(ratio.max()) if ratio.numel() else 0.0
    return r


# ---- mutations -------------------------------------------------------------------------------------------------------------------
def edge_keys(c, sep):
    """{label: sequence slots [B] or int} of the keys the mutations sit on: the first and last position of a 32-, 64- and
    128-position tile (the tile that holds the middle of the largest part; tiles start at the part's origin), the last kept text
    key of every sample, the first image key, the last key of the ragged tail."""
    n0, n1, pos1 = c.n0, c.n1, c.pos1
    slot_of = {int(p): i for i, p in enumerate(c.pos.tolist())}
    if sep or not n0:
        org, end = (pos1, c.NP) if n1 >= n0 else (0, n0)
    else:
        org, end = 0, c.NP
    keys = {}
    for w in (32, 64, 128):
        t = (end - org) // 2 // w
        for lab, p in (("first", org + t * w), ("last", min(org + t * w + w, end) - 1)):
            while p not in slot_of:      # a gap position: the next member
                p += 1
            if slot_of[p] not in keys.values():
                keys["%s of %d-tile" % (lab, w)] = slot_of[p]
    if n0:
        keys["last kept text key"] = (c.lens - 1).to(c.device)
    if n1:
        keys["first image key"] = n0
    keys["last key"] = c.N - 1
    return keys


def mutations(c, sep):
    """[(name, mut)] for `evaluate`: (a) .. (f) of the issue at every key of edge_keys (those the case can state)."""
    dev, out = c.device, []
    ar = torch.arange(c.B, device=dev)
    keepm = c.keep()
    for lab, kk in edge_keys(c, sep).items():
        per_sample = torch.is_tensor(kk)
        kcol = kk if per_sample else torch.full((c.B,), kk, device=dev)
        if not bool(keepm[ar, kcol].any()):
            continue                     # a key no sample keeps (image keep mask): nothing to lose
        for nm, w in (("a dropped", float("-inf")), ("b twice", 1.0)):
            lw = torch.zeros(c.B, c.N, dtype=F64, device=dev)
            lw[ar, kcol] = w
            out.append(("%s: %s" % (nm, lab), dict(logw=lw)))
        k0 = int(kcol[0])
        if c.with_bias:
            out.append(("c bias of (q, k+1): %s" % lab, dict(bias_from=(0, 1, k0))))
            out.append(("c bias of (q+1, k): %s" % lab, dict(bias_from=(1, 0, k0))))
            out.append(("f pair left out: %s" % lab, dict(pair=k0)))
        p = int(c.pos[k0])
        org = (c.pos1 if p >= c.pos1 else 0) if sep else 0
        blk = (c.pos - org) // 32 == (p - org) // 32
        if sep:
            blk = blk & ((c.pos >= c.pos1) == (p >= c.pos1))
        out.append(("e query block left out: %s" % lab, dict(qskip=blk)))
    if c.keep0 is not None and bool((c.lens < c.n0).any()):
        um = torch.zeros(c.B, c.N, dtype=torch.bool, device=dev)
        short = (c.lens < c.n0).to(dev)
        um[ar[short], c.lens.to(dev)[short]] = True
        out.append(("d keep0 longer by one", dict(unmask=um)))
    return out


def prefix_longer(c, q_keep):
    """(g): the rows a prefix longer by one adds (the text prefix where it can grow, else the image prefix)."""
    longer = (q_keep[0] + 1, q_keep[1]) if q_keep[0] < c.n0 else (q_keep[0], q_keep[1] + 1)
    return c.kept_rows(longer)


def exceeds(mutated, ref):
    """Does the mutated evaluation leave the clean one's bounds by more than POWER tau somewhere?  (largest ratio, output)"""
    best = (0.0, None)
    for name in OUTPUTS:
        if name in ref and name in mutated and ref[name] is not None:
            e, t = (mutated[name] - ref[name]).abs(), ref["tau"][name]
            r = torch.where(e == 0, torch.zeros_like(e), e / t)
            if r.numel() and float(r.max()) > best[0]:
                best = (float(r.max()), name)
    return best
