"""Consensus merging with TALL masks (Wang et al., ICML 2024) restated in numpy: the literal transcription of the rule in
include/vlm_hip.h, steps 1-6 and the restore rule.  The reference has no such merge, so this restatement -- not the reference -- is
what the HIP kernel is held to, bit for bit, mask words and padding bits included.  numpy float32 array operations round once per
operation."""
import numpy as np

F = np.float32
CONSENSUS, RESTORE = 0, 1


def pack(keep):
    """A boolean mask of n elements as ceil(n / 32) little-endian 32-bit words: element i is bit i & 31 of word i >> 5, the bits at
    positions >= n are zero."""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    words = (keep.size + 31) // 32
    bits = np.zeros(32 * words, np.uint8)
    bits[:keep.size] = keep
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def unpack(words, n):
    """The host's reading of a packed mask (include/vlm_hip.h, step 6)."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def consensus(c, srcs, tall_lambda, k, lam):
    """c: fp32 central tensor; srcs: fp32 sources in order.  Returns (out, info): info has the S boolean masks `keep`, their packed
    `words`, the multi-task vector `d`, and the counters `kept` (per source), `selected` and `empty`."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n, S = c.size, len(srcs)
    assert 0 <= k <= S and tall_lambda >= 0
    xs = [np.ascontiguousarray(w, dtype=F).reshape(-1) - c for w in srcs]          # 1
    d = np.zeros(n, F)
    for x in xs:                                                                    # 2
        d = d + x
    with np.errstate(invalid="ignore"):
        keep = [np.abs(x) >= F(tall_lambda) * np.abs(d - x) for x in xs]            # 3
    votes = np.zeros(n, np.int32)
    for km in keep:                                                                 # 4
        votes = votes + km
    sel = votes >= k
    out = c + F(lam) * np.where(sel, d, F(0.0)).astype(F)                           # 5
    info = {"keep": keep, "words": [pack(km) for km in keep], "d": d, "kept": [int(km.sum()) for km in keep],   # 6
            "selected": int(sel.sum()), "empty": int((votes == 0).sum()), "votes": votes}
    return out.astype(F), info


def restore(u, c, words):
    """dst[i] = bit_i ? u[i] : c[i].  Returns (out, info) with the counters of a restore job: kept[0] = the elements taken from u."""
    u = np.ascontiguousarray(u, dtype=F).reshape(-1)
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    bits = unpack(words, u.size)
    return np.where(bits, u, c).astype(F), {"kept": [int(bits.sum())], "selected": 0, "empty": 0}
