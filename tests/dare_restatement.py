"""DARE (drop and rescale) restated in numpy: the literal transcription of the rule in include/vlm_hip.h.  The reference has no
DARE, so this restatement -- not the reference -- is what the HIP kernel is held to, bit for bit.  numpy float32 array operations
round once per operation; Philox4x32-10 is written with uint64 products, whose halves are the two words a round needs."""
import math

import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = U64(0xFFFFFFFF)
LINEAR, TIES = 0, 1


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape; key: two python ints.  Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=U64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c[0]  # < 2^64: no wrap
        p1 = M1 * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF  # bumped after each round
        k1 = (k1 + W1) & 0xFFFFFFFF
    return [x.astype(U32) for x in c]


def draws(n, m, stream, seed):
    """u_m[0 .. n): word (i & 3) of the block with counter (i >> 2, 0, m, stream) and key (seed & 0xffffffff, seed >> 32)."""
    n4 = (n + 3) // 4
    w = philox4x32_10([np.arange(n4, dtype=U64), 0, m, stream], (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def keep_below(drop):
    return math.floor((1.0 - drop) * 2 ** 32)


def rescale_of(drop, rescale=True):
    return F(1.0 / (1.0 - drop)) if rescale else F(1.0)


def dare(c, srcs, drop, lam, seed, stream, mode, rescale=True):
    """c: fp32 central tensor; srcs: fp32 sources in order.  Returns (out, info) with info = keep_below, kept per source, conflict
    and empty counts, and the masks themselves (for tests that compare patterns)."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n = c.size
    kb = keep_below(drop)
    assert 1 <= kb <= 2 ** 32
    r = rescale_of(drop, rescale)
    tts, masks = [], []
    for m, w in enumerate(srcs):
        t = np.ascontiguousarray(w, dtype=F).reshape(-1) - c                      # 1
        k = draws(n, m, stream, seed).astype(U64) < U64(kb)                       # 2, 3
        tts.append(np.where(k, t * r, F(0.0)).astype(F))
        masks.append(k)
    pos = np.any([tt > 0 for tt in tts], axis=0)
    neg = np.any([tt < 0 for tt in tts], axis=0)
    if mode == LINEAR:                                                            # 4
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
    out = c + F(lam) * d                                                          # 5
    info = {"keep_below": kb, "kept": [int(k.sum()) for k in masks], "conflict": int((pos & neg).sum()),
            "empty": int(empty.sum()), "masks": masks}
    return out.astype(F), info
