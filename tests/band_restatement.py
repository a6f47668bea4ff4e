"""Model Breadcrumbs (magnitude band trim; Davari & Belilovsky 2023) restated in numpy: the literal transcription of the rule in
include/vlm_hip.h.  The reference has no such merge, so this restatement -- not the reference -- is what the HIP kernels are held
to, bit for bit.  numpy float32 array operations round once per operation; np.partition on the uint32 keys gives both thresholds."""
import math

import numpy as np

F = np.float32
LINEAR, TIES = 0, 1
NO_OUTLIER = 0x80000000  # thr_hi of k_hi = 0: above every key


def ranks(n, density, gamma):
    """(k_hi, k_lo) in python doubles, as merge.band_ranks states them."""
    k_hi = min(n - 1, math.floor(gamma * n))
    return k_hi, min(n, k_hi + max(1, math.ceil(density * n)))


def kth_largest(key, k):
    n = key.size
    return int(np.partition(key, n - k)[n - k])


def thresholds(key, k_hi, k_lo):
    """(thr_lo, thr_hi) as integers: step 2."""
    return kth_largest(key, k_lo), (kth_largest(key, k_hi) if k_hi >= 1 else NO_OUTLIER)


def band(c, srcs, ranks_per_source, lam, mode=LINEAR):
    """c: fp32 central tensor; srcs: fp32 sources in order; ranks_per_source: (k_hi, k_lo) per source.  Returns (out, info) with
    info = both thresholds (uint32 keys), kept and outlier per source, conflict and empty counts."""
    c = np.ascontiguousarray(c, dtype=F).reshape(-1)
    n = c.size
    tts, masks, lo, hi, kept, outlier = [], [], [], [], [], []
    for w, (k_hi, k_lo) in zip(srcs, ranks_per_source):
        assert 0 <= k_hi < k_lo <= n
        t = np.ascontiguousarray(w, dtype=F).reshape(-1) - c                      # 1
        key = t.view(np.uint32) & np.uint32(0x7FFFFFFF)                           # 2
        thr_lo, thr_hi = thresholds(key, k_hi, k_lo)
        out_m = key.astype(np.uint64) >= thr_hi
        kept_m = (key >= thr_lo) & ~out_m
        tts.append(np.where(kept_m, t, F(0.0)))
        masks.append(kept_m)
        lo.append(thr_lo)
        hi.append(thr_hi)
        kept.append(int(kept_m.sum()))
        outlier.append(int(out_m.sum()))
    if mode == LINEAR:                                                            # 3
        d = np.zeros(n, F)
        for tt in tts:
            d = d + tt
        empty = ~np.any(masks, axis=0)
    else:
        s = np.zeros(n, F)
        for tt in tts:                                                            # TIES 3
            s = s + tt
        num, cnt = np.zeros(n, F), np.zeros(n, np.int32)
        for tt in tts:                                                            # TIES 4
            agree = ((s > 0) & (tt > 0)) | ((s < 0) & (tt < 0))
            num = np.where(agree, num + tt, num)
            cnt = cnt + agree
        d = np.where(cnt > 0, num / np.maximum(cnt, 1).astype(F), F(0.0)).astype(F)
        empty = cnt == 0
    out = c + F(lam) * d                                                          # 4
    pos = np.any([tt > 0 for tt in tts], axis=0)
    neg = np.any([tt < 0 for tt in tts], axis=0)
    info = {"threshold_lo_bits": lo, "threshold_hi_bits": hi,
            "threshold_lo": [float(np.uint32(x).view(F)) for x in lo],
            "threshold_hi": [None if x == NO_OUTLIER else float(np.uint32(x).view(F)) for x in hi],
            "kept": kept, "outlier": outlier, "kept_mask": masks,
            "conflict": int((pos & neg).sum()), "empty": int(empty.sum())}
    return out.astype(F), info
