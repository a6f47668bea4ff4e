"""SCE (select, calculate, erase) restated in numpy and python doubles: the literal transcription of the rule in include/vlm_hip.h.
The reference has no such merge, so this restatement -- not the reference -- is what the HIP kernels are held to, bit for bit.
Steps 1-3 and 6-7 are numpy float32 array operations, which round once per operation (numpy's float32 division is correctly
rounded); np.partition on the uint32 keys gives the threshold; step 4 is the pair statistics' ordered sums
(pairstats_restatement.ordered_sums); step 5 is python float arithmetic (IEEE double, one rounding per operation), rounded once to
float32."""
import struct

import numpy as np

from pairstats_restatement import keys, ordered_sums, task_vectors
from ties_restatement import keep_count

F, D = np.float32, np.float64
MAX_SRC = 4


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def variance(xs):
    """Step 2: the population variance of the S task-vector entries of every element, in fp32, source order."""
    S = len(xs)
    total = np.zeros(xs[0].size, F)
    for x in xs:
        total = total + x
    mean = total / F(S)
    q = np.zeros(xs[0].size, F)
    for x in xs:
        e = x - mean
        q = q + e * e
    return (q / F(S)).astype(F)


def weights(sq):
    """Step 5.  sq: S doubles.  Returns (tot, [w_m as python floats that hold the float32])."""
    S = len(sq)
    tot = 0.0
    for v in sq:
        tot = tot + v
    if tot > 0:
        return tot, [float(F(v / tot)) for v in sq]  # float64 -> float32: one rounding, to nearest even
    return tot, [float(F(1.0 / S))] * S


def erase(xs, sel, w):
    """Step 6 for task vectors xs, the selection and the weights: (d, the tt_m, how many entries agree per element)."""
    n = xs[0].size
    tts = [np.where(sel, x, F(0.0)).astype(F) for x in xs]
    s = np.zeros(n, F)
    for tt in tts:
        s = s + tt
    num, den, cnt = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int32)
    for tt, wm in zip(tts, w):
        agree = ((s > 0) & (tt > 0)) | ((s < 0) & (tt < 0))
        num = np.where(agree, num + F(wm) * tt, num).astype(F)
        den = np.where(agree, den + F(wm), den).astype(F)
        cnt = cnt + agree
    some = den > 0
    d = np.where(some, num / np.where(some, den, F(1.0)), F(0.0)).astype(F)
    return d, tts, cnt


def sce(c, srcs, density, lam, keep=None, name=None):
    """One job: (the output, float32 [n]; the row ScePlan.report() gives).  `keep` = an explicit K instead of the density's."""
    xs = task_vectors(srcs, c)                                                       # step 1
    S, n = len(xs), xs[0].size
    assert 1 <= S <= MAX_SRC
    key = keys(variance(xs))                                                         # step 2
    K = keep_count(density, n) if keep is None else keep
    thr = np.partition(key, n - K)[n - K]                                            # step 3: the K-th largest key
    sel = key >= thr
    sq = ordered_sums([np.where(sel, x.astype(D) * x.astype(D), D(0.0)) for x in xs])  # step 4
    tot, w = weights(sq)                                                             # step 5
    d, tts, cnt = erase(xs, sel, w)                                                  # step 6
    out = np.ascontiguousarray(c, dtype=F).reshape(-1) + F(lam) * d                  # step 7
    pos = np.any([tt > 0 for tt in tts], axis=0)
    neg = np.any([tt < 0 for tt in tts], axis=0)
    row = {"dst": name, "n": int(n), "K": int(K), "threshold": float(np.uint32(thr).view(F)), "threshold_bits": int(thr),
           "kept": int(sel.sum()), "sq": sq, "tot": tot, "weight": w, "weight_bits": [f32_bits(v) for v in w],
           "conflict": int((pos & neg).sum()), "empty": int((cnt == 0).sum())}
    return out.astype(F), row
