"""TIES-merging (trim, elect sign, disjoint mean) restated in numpy: the literal transcription of the rule in
include/vlm_hip.h.  The reference has no TIES, so this restatement -- not the reference -- is what the HIP kernels are held to,
bit for bit.  numpy float32 array operations round once per operation; np.partition on the uint32 keys gives the threshold."""
import math

import numpy as np

F = np.float32


def keep_count(density, n):
    return max(1, min(n, math.ceil(density * n)))


def ties(c, srcs, density, lam, keep=None):
    """c: fp32 central tensor; srcs: fp32 sources in order.  Returns (out, info) with info = thresholds (uint32 keys), kept per
    source, conflict and empty counts."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n = c.size
    tts, thr, kept = [], [], []
    for m, w in enumerate(srcs):
        t = np.ascontiguousarray(w, dtype=F).reshape(-1) - c                      # 1
        key = t.view(np.uint32) & np.uint32(0x7FFFFFFF)                           # 2
        K = keep_count(density, n) if keep is None else keep[m]
        th = np.partition(key, n - K)[n - K]                                      # the K-th largest key
        k = key >= th
        tts.append(np.where(k, t, F(0.0)))
        thr.append(int(th))
        kept.append(int(k.sum()))
    s = np.zeros(n, F)
    for tt in tts:                                                                # 3
        s = s + tt
    num, cnt = np.zeros(n, F), np.zeros(n, np.int32)
    for tt in tts:                                                                # 4
        agree = ((s > 0) & (tt > 0)) | ((s < 0) & (tt < 0))
        num = np.where(agree, num + tt, num)
        cnt = cnt + agree
    d = np.where(cnt > 0, num / np.maximum(cnt, 1).astype(F), F(0.0)).astype(F)
    out = c + F(lam) * d                                                          # 5
    pos = np.any([tt > 0 for tt in tts], axis=0)
    neg = np.any([tt < 0 for tt in tts], axis=0)
    info = {"threshold_bits": thr, "threshold": [float(np.uint32(x).view(F)) for x in thr], "kept": kept,
            "conflict": int((pos & neg).sum()), "empty": int((cnt == 0).sum())}
    return out.astype(F), info
