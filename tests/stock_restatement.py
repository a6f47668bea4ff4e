"""Model Stock restated in numpy and python doubles: the literal transcription of the rule in include/vlm_hip.h.  The reference has
no such merge, so this restatement -- not the reference -- is what the HIP kernels are held to, bit for bit.  Step 2 is the pair
statistics' ordered sums (pairstats_restatement.ordered_sums); step 3 is python float arithmetic (IEEE double, one rounding per
operation) with math.sqrt; steps 1 and 4 are numpy float32 array operations, which round once per operation."""
import math
import struct

import numpy as np

from pairstats_restatement import ordered_sums, pair_slot, task_vectors

F, D = np.float32, np.float64
MAX_SRC = 4


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def ratio(sq, dot):
    """Step 3.  sq: S doubles; dot: S (S - 1) / 2 doubles in slot order.  Returns (cos_pair, cos, t, scale) with scale a python
    float that holds the float32."""
    S = len(sq)
    cos_pair = []
    for b in range(1, S):
        for a in range(b):
            den = math.sqrt(sq[a] * sq[b])
            cos_pair.append(dot[pair_slot(a, b)] / den if den > 0 else 0.0)
    if S == 1:
        cos, t = 0.0, 1.0
    else:
        total = 0.0
        for cp in cos_pair:
            total = total + cp
        cos = total / len(cos_pair)
        cc = (cos if cos < 1 else 1.0) if cos > 0 else 0.0
        t = (S * cc) / (1 + (S - 1) * cc)
    return cos_pair, cos, t, float(F(t / S))  # float64 -> float32: one rounding, to nearest even


def stock(c, srcs, name=None):
    """One job: (the output, float32 [n]; the row StockPlan.report() gives)."""
    xs = task_vectors(srcs, c)                                                       # step 1
    S = len(xs)
    assert 1 <= S <= MAX_SRC
    xd = [x.astype(D) for x in xs]
    order = [(a, b) for b in range(1, S) for a in range(b)]
    assert [pair_slot(a, b) for a, b in order] == list(range(len(order)))
    flat = ordered_sums([d * d for d in xd] + [xd[a] * xd[b] for a, b in order])     # step 2
    sq, dot = flat[:S], flat[S:]
    cos_pair, cos, t, scale = ratio(sq, dot)                                         # step 3
    d = np.zeros(xs[0].size, F)
    for x in xs:                                                                     # step 4
        d = d + x
    out = np.ascontiguousarray(c, dtype=F).reshape(-1) + F(scale) * d
    row = {"dst": name, "n": int(xs[0].size), "sq": sq,
           "pairs": [{"a": a, "b": b, "dot": dot[i], "cosine": cos_pair[i]} for i, (a, b) in enumerate(order)],
           "cos": cos, "t": t, "scale": scale, "scale_bits": f32_bits(scale)}
    return out.astype(F), row
