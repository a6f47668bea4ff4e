"""DELLA (magnitude-ranked drop and rescale) restated in numpy: the literal transcription of the rule in include/vlm_hip.h.  The
reference has no DELLA, so this restatement -- not the reference -- is what the HIP kernel is held to, bit for bit.  numpy float32
array operations round once per operation; the draws are dare_restatement's; the ranks come from a stable argsort of the keys of
each row, and the keep thresholds are made in uint64."""
import math

import numpy as np

from dare_restatement import draws

F = np.float32
U32 = np.uint32
U64 = np.uint64
LINEAR, TIES = 0, 1
MAX_ROW = 4096


def window(density, epsilon):
    """(keep_lo, keep_hi) in python doubles."""
    return math.floor((density - epsilon) * 2 ** 32), math.floor((density + epsilon) * 2 ** 32)


def keys(t):
    return np.ascontiguousarray(t, dtype=F).view(U32) & U32(0x7FFFFFFF)


def ranks(t, row_len):
    """r[i] = how many j of i's row have key(t[j]) < key(t[i]), or the same key and j < i (step 2): a stable argsort per row."""
    k = keys(t).reshape(-1, row_len)
    order = np.argsort(k, axis=1, kind="stable")
    r = np.empty_like(order)
    np.put_along_axis(r, order, np.broadcast_to(np.arange(row_len), k.shape), axis=1)
    return r.reshape(-1).astype(U64)


def keep_thresholds(r, row_len, keep_lo, keep_hi):
    """kb[i] of step 3, uint64."""
    lo, span = U64(keep_lo), U64(keep_hi - keep_lo)
    if row_len == 1:
        return np.full(r.shape, lo + (span >> U64(1)), U64)
    return lo + span * r // U64(row_len - 1)  # < 2^44: no wrap


def della(c, srcs, row_len, keep_lo, keep_hi, lam, seed, stream, mode, rescale=True):
    """c: fp32 central tensor; srcs: fp32 sources in order.  Returns (out, info) with info = kept per source, conflict and empty
    counts, the masks, the ranks and the thresholds (for tests that compare patterns)."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n = c.size
    assert 1 <= row_len <= MAX_ROW and n % row_len == 0 and 1 <= keep_lo <= keep_hi <= 2 ** 32
    tts, masks, rks, kbs = [], [], [], []
    for m, w in enumerate(srcs):
        t = np.ascontiguousarray(w, dtype=F).reshape(-1) - c                      # 1
        r = ranks(t, row_len)                                                     # 2
        kb = keep_thresholds(r, row_len, keep_lo, keep_hi)                        # 3
        k = draws(n, m, stream, seed).astype(U64) < kb                            # 4, 5
        scale = F(4294967296.0) / kb.astype(F) if rescale else np.ones(n, F)
        tts.append(np.where(k, t * scale, F(0.0)).astype(F))
        masks.append(k)
        rks.append(r)
        kbs.append(kb)
    pos = np.any([tt > 0 for tt in tts], axis=0)
    neg = np.any([tt < 0 for tt in tts], axis=0)
    if mode == LINEAR:                                                            # 6
        d = np.zeros(n, F)
        for tt in tts:
            d = d + tt
        empty = ~np.any(masks, axis=0)
    else:
        s = np.zeros(n, F)
        for tt in tts:
            s = s + tt
        num, cnt = np.zeros(n, F), np.zeros(n, np.int32)
        for tt in tts:
            agree = ((s > 0) & (tt > 0)) | ((s < 0) & (tt < 0))
            num = np.where(agree, num + tt, num)
            cnt = cnt + agree
        d = np.where(cnt > 0, num / np.maximum(cnt, 1).astype(F), F(0.0)).astype(F)
        empty = cnt == 0
    out = c + F(lam) * d                                                          # 7
    info = {"keep_lo": keep_lo, "keep_hi": keep_hi, "row_len": row_len, "kept": [int(k.sum()) for k in masks],
            "conflict": int((pos & neg).sum()), "empty": int(empty.sum()), "masks": masks, "ranks": rks, "kb": kbs}
    return out.astype(F), info
