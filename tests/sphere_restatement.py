"""The spherical merge (SLERP / weighted Karcher mean) restated in numpy and python doubles: the literal transcription of the rule in
include/vlm_hip.h.  The reference has no such merge, so this restatement -- not the reference -- is what the HIP kernels are held
to.  Step 2 of a tensor group is Model Stock's (pairstats_restatement.ordered_sums); step 2 of a row group is the pinned lane order
written out below; step 3 is python float arithmetic (IEEE double, one rounding per operation) with math.sqrt, math.acos, math.sin
and math.cos; steps 1 and 4 are numpy float32 array operations, which round once per operation.  Everything but acos / sin / cos is
bit-exact against the device; those three are the host libm's here and the device library's there."""
import math
import struct

import numpy as np

from pairstats_restatement import ordered_sums, pair_slot, task_vectors

F, D = np.float32, np.float64
MAX_SRC = 4
ITERS = 24
EDGE = 2.0 ** -20
QMIN = 2.0 ** -40
OK, LINEAR, ZERO = "ok", "linear", "zero"


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32(x):
    """float32(x) of a python double, as a python double: one rounding, to nearest even."""
    return float(F(x))


def pair_order(S):
    order = [(a, b) for b in range(1, S) for a in range(b)]
    assert [pair_slot(a, b) for a, b in order] == list(range(len(order)))
    return order


def row_sums(terms, L):
    """Step 2 of row groups.  terms: float64 [K, rows * L] addends.  Returns float64 [K, rows]: lane l of 64 adds the addends of
    elements l, l + 64, ... of the row in rising order, from +0.0 (a lane without elements stays +0.0; padding with +0.0 changes no
    sum, since a sum that starts at +0.0 is never -0.0), then the fold by halves."""
    K, n = terms.shape
    rows = n // L
    steps = -(-L // 64)
    body = np.zeros((K, rows, steps * 64), D)
    body[:, :, :L] = terms.reshape(K, rows, L)
    v = body.reshape(K, rows, steps, 64)
    acc = np.zeros((K, rows, 64), D)
    for k in range(steps):
        acc = acc + v[:, :, k, :]
    for half in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :half] + acc[..., half:2 * half]
    return acc[..., 0]


def solve(sq, dot, w):
    """Step 3.  sq: S doubles; dot: S (S - 1) / 2 doubles in slot order; w: S doubles.  Returns a dict with status, coef64, coef32
    (python floats that hold the float32), rho, resid."""
    S = len(sq)
    ws = 0.0
    for m in range(S):
        if sq[m] > 0:
            ws = ws + w[m]
    if not ws > 0:
        return {"status": ZERO, "coef64": [0.0] * S, "coef32": [0.0] * S, "rho": 0.0, "resid": 0.0}
    ww = [w[m] / ws if sq[m] > 0 else 0.0 for m in range(S)]
    n = [math.sqrt(sq[m]) for m in range(S)]
    C = [[1.0 if i == j else (dot[pair_slot(min(i, j), max(i, j))] / (n[i] * n[j]) if ww[i] > 0 and ww[j] > 0 else 0.0)
          for j in range(S)] for i in range(S)]

    def nrm2(v):
        t = 0.0
        for i in range(S):
            for j in range(S):
                t = t + (v[i] * v[j]) * C[i][j]
        return t

    rho = 0.0
    for m in range(S):
        rho = rho + ww[m] * n[m]
    a = list(ww)
    q = nrm2(a)
    if not q > QMIN:
        return {"status": LINEAR, "coef64": list(ww), "coef32": [f32(x) for x in ww], "rho": rho, "resid": 0.0}
    r = math.sqrt(q)
    a = [x / r for x in a]
    vn = 0.0
    for _ in range(ITERS):
        v = [0.0] * S
        for i in range(S):
            if not ww[i] > 0:
                continue
            ci = 0.0
            for j in range(S):
                ci = ci + a[j] * C[j][i]
            if ci >= 1 - EDGE:
                k = 1.0
            elif ci <= -1 + EDGE:
                k = 0.0
            else:
                th = math.acos(ci)
                k = th / math.sin(th)
            wk = ww[i] * k
            for j in range(S):
                v[j] = v[j] + wk * ((1.0 if j == i else 0.0) - ci * a[j])
        q = nrm2(v)
        if not q > 0:
            vn = 0.0
            break
        vn = math.sqrt(q)
        cv, sv = math.cos(vn), math.sin(vn) / vn
        b = [cv * a[j] + sv * v[j] for j in range(S)]
        q2 = nrm2(b)
        if not q2 > QMIN:
            break
        r = math.sqrt(q2)
        a = [x / r for x in b]
    coef = [(rho * a[m]) / n[m] if ww[m] > 0 else 0.0 for m in range(S)]
    return {"status": OK, "coef64": coef, "coef32": [f32(x) for x in coef], "rho": rho, "resid": vn}


def gram_terms(xs):
    xd = [x.astype(D) for x in xs]
    return [d * d for d in xd] + [xd[a] * xd[b] for a, b in pair_order(len(xs))]


def apply(c, xs, coef32, lam=1.0, row_len=0):
    """Step 4.  coef32: [S] floats for a tensor group, or an array [rows, >= S] for row groups.  Returns float32 [n]."""
    n = xs[0].size
    d = np.zeros(n, F)
    for m, x in enumerate(xs):
        cm = F(coef32[m]) if not row_len else np.repeat(np.asarray(coef32, dtype=F)[:, m], row_len)
        d = d + cm * x
    if c is None:
        return d.astype(F)
    return (np.ascontiguousarray(c, dtype=F).reshape(-1) + F(lam) * d).astype(F)


def sphere(c, srcs, w, lam=1.0, row_len=0, coef32=None):
    """One job: (the output float32 [n]; for a tensor job the solve's dict with sq and dot added, for a row job the list of the
    rows' dicts).  `coef32`: take these coefficients in step 4 (the device's own bits) in place of the restatement's."""
    xs = task_vectors(srcs, c)                                                       # step 1
    S = len(xs)
    assert 1 <= S <= MAX_SRC and len(w) == S
    if c is None:
        assert lam == 1.0
    w = [float(x) for x in w]
    if not row_len:
        flat = ordered_sums(gram_terms(xs))                                          # step 2
        res = solve(flat[:S], flat[S:], w)                                           # step 3
        res.update(sq=flat[:S], dot=flat[S:])
        out = apply(c, xs, res["coef32"] if coef32 is None else coef32, lam)         # step 4
        return out, res
    assert xs[0].size % row_len == 0
    sums = row_sums(np.stack(gram_terms(xs)), row_len)
    rows = [solve([float(v) for v in sums[:S, r]], [float(v) for v in sums[S:, r]], w) for r in range(sums.shape[1])]
    mine = np.array([r["coef32"] for r in rows], dtype=F).reshape(len(rows), S)
    return apply(c, xs, mine if coef32 is None else coef32, lam, row_len), rows


def counters(rows):
    """What a row job's result counts: (rows_linear, rows_zero, resid_max)."""
    return (sum(r["status"] == LINEAR for r in rows), sum(r["status"] == ZERO for r in rows), max([0.0] + [r["resid"] for r in rows]))


def slerp(x0, x1, t):
    """Closed-form SLERP(t) of the directions of x0 and x1 (float64 arrays) with the norm interpolated linearly."""
    n0, n1 = math.sqrt(float(x0 @ x0)), math.sqrt(float(x1 @ x1))
    u0, u1 = x0 / n0, x1 / n1
    om = math.acos(max(-1.0, min(1.0, float(u0 @ u1))))
    if om < 1e-9:
        d = (1 - t) * u0 + t * u1
    else:
        d = (math.sin((1 - t) * om) * u0 + math.sin(t * om) * u1) / math.sin(om)
    return ((1 - t) * n0 + t * n1) * d
