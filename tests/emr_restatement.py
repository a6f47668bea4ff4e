"""EMR-Merging (Huang et al., NeurIPS 2024: elect, mask, rescale) restated in numpy: the literal transcription of the rule in
include/vlm_hip.h, steps 1-7 and the restore rule, INCLUDING the order of every floating-point sum.  The reference has no such
merge, so this restatement -- not the reference -- is what the HIP kernels are held to, bit for bit: outputs, mask words with their
padding bits, sums, counts and rescalers.  numpy float32 / float64 array operations round once per operation.

The ordered sums are pairstats_restatement's tree with ONE difference, the ragged tail: here the n & 3 tail elements belong to the
one thread that stands at the partial float4 n4 = n >> 2 -- thread n4 & 255 of the job's last chunk -- and enter that thread's sums
after its float4s, in element order (the pair statistics hand tail element t to thread t)."""
import numpy as np

from pairstats_restatement import CHUNK, n_chunks
from tall_restatement import pack, unpack

F, D = np.float32, np.float64
MAX_SRC = 4


def chunk_records(term):
    """term: float64 [K, n], one addend per sum and element.  Returns the chunk records, float64 [K, chunks], by the pinned tree
    with this rule's tail."""
    K, n = term.shape
    n4, nc = n // 4, n_chunks(n)
    body = np.zeros((K, nc * CHUNK), D)
    body[:, :4 * n4] = term[:, :4 * n4]
    v = body.reshape(K, nc, 4, 256, 4)
    acc = np.zeros((K, nc, 256), D)
    for u in range(4):                                   # thread: its float4s in order, in each the components in order
        for c in range(4):
            acc = acc + v[:, :, u, :, c]
    t = n4 & 255                                         # then the tail, all of it in the thread that stands at float4 n4
    for i in range(4 * n4, n):
        acc[:, nc - 1, t] = acc[:, nc - 1, t] + term[:, i]
    w = acc.reshape(K, nc, 4, 64)
    for half in (32, 16, 8, 4, 2, 1):                    # wave: folded by halves
        w = w[..., :half] + w[..., half:2 * half]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]  # workgroup: ((w0 + w1) + w2) + w3


def ordered_sums(term_list):
    """The job's sums (a list of float64 [n] addends): the chunk records added one after the other, from +0.0."""
    rec = chunk_records(np.stack([np.ascontiguousarray(t, dtype=D) for t in term_list]))
    total = np.zeros(rec.shape[0], D)
    for k in range(rec.shape[1]):
        total = total + rec[:, k]
    return [float(t) for t in total]


def emr(c, srcs, lam):
    """c: fp32 central tensor; srcs: fp32 sources in order.  Returns (out, info): info has the S boolean masks `agree`, their packed
    `words`, the unified task vector `u`, the sums `abs_sum` and `uni_sum` (python floats), `rescale` (numpy float32 scalars) and
    the counts `kept` (per source), `zero`, `conflict`, and `votes` (how many sources agree, per element)."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n, S = c.size, len(srcs)
    assert 1 <= S <= MAX_SRC
    xs = [np.ascontiguousarray(w, dtype=F).reshape(-1) - c for w in srcs]          # 1
    s = np.zeros(n, F)
    for x in xs:                                                                    # 2
        s = s + x
    sp, sn = s > 0, s < 0
    agree = [(sp & (x > 0)) | (sn & (x < 0)) for x in xs]                           # 3
    e = np.zeros(n, F)
    for x, ag in zip(xs, agree):
        e = np.where(ag, np.maximum(e, np.abs(x)), e).astype(F)
    u = np.where(sp, e, np.where(sn, -e, F(0.0))).astype(F)
    out = (c + F(lam) * u).astype(F)                                                # 4
    ed = e.astype(D)
    sums = ordered_sums([np.abs(x).astype(D) for x in xs] + [np.where(ag, ed, D(0.0)) for ag in agree])   # 6
    a, b = sums[:S], sums[S:]
    with np.errstate(divide="ignore", invalid="ignore"):
        rescale = [F(D(a[m]) / D(b[m])) if b[m] > 0 else F(0.0) for m in range(S)]  # 7
    has_pos, has_neg = np.zeros(n, bool), np.zeros(n, bool)
    votes = np.zeros(n, np.int32)
    for x, ag in zip(xs, agree):
        has_pos |= x > 0
        has_neg |= x < 0
        votes = votes + ag
    info = {"agree": agree, "words": [pack(ag) for ag in agree], "u": u, "s": s, "abs_sum": a, "uni_sum": b, "rescale": rescale,   # 5
            "kept": [int(ag.sum()) for ag in agree], "zero": int((~(sp | sn)).sum()), "conflict": int((has_pos & has_neg).sum()),
            "votes": votes}
    return out, info


def restore(uni, c, words, rescale):
    """t = uni - c;  y = bit ? t : +0.0;  dst = c + rescale * y.  Returns (out, info) with the one count of a restore job."""
    uni = np.ascontiguousarray(uni, dtype=F).reshape(-1)
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    bits = unpack(words, uni.size)
    t = uni - c
    y = np.where(bits, t, F(0.0)).astype(F)
    return (c + F(rescale) * y).astype(F), {"kept": [int(bits.sum())]}
