"""Expert-pair statistics restated in numpy: the literal transcription of the rule in include/vlm_hip.h, INCLUDING the order of
every floating-point sum (thread, wave, workgroup, job).  The reference has no such measure, so this restatement -- not the
reference -- is what the HIP kernels are held to, bit for bit.  numpy float32 / float64 array operations round once per operation.

The per-thread sums are vectorised per chunk as [chunks, 4, 256, 4] (chunk, float4 u of the thread, thread t, component c): the
float4 at index 1024 chunk + 256 u + t belongs to thread t.  Places past the end hold +0.0: every sum starts at +0.0 and so is
never -0.0, hence adding +0.0 for a place the kernel skips gives the bytes the kernel has."""
import math
import struct

import numpy as np

F, D = np.float32, np.float64
MAX_SRC = 4
CHUNK = 4096      # floats per chunk: 256 threads x 4 float4
SUMS = ("dot", "dist2", "ssd_sum", "tssd_sum")
COUNTS = ("live", "conflict", "tlive", "tconflict")


def pair_slot(a, b):
    """Where the pair (a, b), a < b, lives in a result: independent of the source count."""
    assert 0 <= a < b < MAX_SRC
    return b * (b - 1) // 2 + a


def n_chunks(n):
    return max(1, -(-(n // 4) // (CHUNK // 4)))


def chunk_records(term):
    """term: float64 [K, n], one addend per statistic and element.  Returns the chunk records, float64 [K, chunks], by the pinned
    tree."""
    K, n = term.shape
    n4, nc = n // 4, n_chunks(n)
    body = np.zeros((K, nc * CHUNK), D)
    body[:, :4 * n4] = term[:, :4 * n4]
    v = body.reshape(K, nc, 4, 256, 4)
    acc = np.zeros((K, nc, 256), D)
    for u in range(4):                                   # thread: its float4s in order, in each the components in order
        for c in range(4):
            acc = acc + v[:, :, u, :, c]
    tail = n & 3
    if tail:                                             # then the ragged-tail element 4 n4 + t, in the chunk of the last float4
        acc[:, nc - 1, :tail] = acc[:, nc - 1, :tail] + term[:, 4 * n4:]
    w = acc.reshape(K, nc, 4, 64)
    for half in (32, 16, 8, 4, 2, 1):                    # wave: folded by halves
        w = w[..., :half] + w[..., half:2 * half]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]  # workgroup: ((w0 + w1) + w2) + w3


def ordered_sums(term_list):
    """The job's sums of K statistics (a list of float64 [n] addends): the chunk records added one after the other, from +0.0."""
    rec = chunk_records(np.stack([np.ascontiguousarray(t, dtype=D) for t in term_list]))
    total = np.zeros(rec.shape[0], D)
    for k in range(rec.shape[1]):
        total = total + rec[:, k]
    return [float(t) for t in total]


def ordered_sum(term):
    return ordered_sums([term])[0]


def task_vectors(srcs, c=None):
    """Step 1: x_m = W_m - c in fp32, or W_m itself without a central tensor."""
    xs = [np.ascontiguousarray(w, dtype=F).reshape(-1) for w in srcs]
    if c is not None:
        c = np.ascontiguousarray(c, dtype=F).reshape(-1)
        xs = [x - c for x in xs]
    return xs


def keys(x):
    return x.view(np.uint32) & np.uint32(0x7FFFFFFF)


def terms(srcs, c=None, tkeys=None):
    """The addends of every statistic, per element: ({"sq": [S arrays], "nnz": [...]}, {(a, b): {name: array}}).  Doubles are
    float64 arrays, counts boolean arrays."""
    xs = task_vectors(srcs, c)
    S = len(xs)
    assert 1 <= S <= MAX_SRC
    tkeys = [0] * S if tkeys is None else list(tkeys)
    xd = [x.astype(D) for x in xs]
    inside = [keys(x) >= np.uint32(k) for x, k in zip(xs, tkeys)]
    per_src = {"sq": [d * d for d in xd], "nnz": [x != 0 for x in xs]}               # step 2
    per_pair = {}
    for b in range(1, S):                                                            # step 3
        for a in range(b):
            xa, xb = xs[a], xs[b]
            den = np.abs(xa) + np.abs(xb)
            live = den > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(live, np.abs(xa + xb) / den, F(0.0)).astype(F)
            conf = ((xa > 0) & (xb < 0)) | ((xa < 0) & (xb > 0))
            t = live & (inside[a] | inside[b])
            d = xd[a] - xd[b]
            rd = r.astype(D)
            per_pair[(a, b)] = {"dot": xd[a] * xd[b], "dist2": d * d, "ssd_sum": rd, "tssd_sum": np.where(t, rd, D(0.0)),
                                "live": live, "conflict": conf, "tlive": t, "tconflict": t & conf}
    return per_src, per_pair


def derived(p):
    """The measures derived from a pair's raw sums, in python doubles; None where the denominator is zero."""
    norm = math.sqrt(p["sq_a"] * p["sq_b"])
    return {"l2": math.sqrt(p["dist2"]),
            "cosine": p["dot"] / norm if norm != 0 else None,
            "ssd": 1.0 - p["ssd_sum"] / p["live"] if p["live"] else None,
            "tssd": 1.0 - p["tssd_sum"] / p["tlive"] if p["tlive"] else None,
            "conflict_rate": p["conflict"] / p["live"] if p["live"] else None}


def pair_stats(srcs, c=None, tkeys=None, name=None):
    """One job, as PairStatsPlan.report() gives its row."""
    per_src, per_pair = terms(srcs, c, tkeys)
    S = len(srcs)
    order = sorted(per_pair, key=lambda ab: pair_slot(*ab))
    flat = ordered_sums(per_src["sq"] + [per_pair[ab][k] for ab in order for k in SUMS])
    sq, rest = flat[:S], flat[S:]
    pairs = []
    for i, (a, b) in enumerate(order):
        tm = per_pair[(a, b)]
        p = {"a": a, "b": b, "sq_a": sq[a], "sq_b": sq[b]}
        p.update(zip(SUMS, rest[len(SUMS) * i: len(SUMS) * (i + 1)]))
        p.update({k: int(tm[k].sum()) for k in COUNTS})
        p.update(derived(p))
        pairs.append(p)
    return {"dst": name, "n": int(per_src["sq"][0].size), "tkey": [int(k) for k in (tkeys or [0] * S)], "sq": sq,
            "nnz": [int(t.sum()) for t in per_src["nnz"]], "pairs": pairs}


def density_keys(srcs, c, density):
    """Threshold keys as TIES takes them: per source the K-th largest key, K = max(1, min(n, ceil(density n)))."""
    out = []
    for x in task_vectors(srcs, c):
        n = x.size
        K = max(1, min(n, math.ceil(density * n)))
        out.append(int(np.partition(keys(x), n - K)[n - K]))
    return out


def rms_keys(row, r):
    """tkey[m] = bits(float32(r * sqrt(sq_m / n))), computed in python doubles."""
    return [struct.unpack("<I", struct.pack("<f", r * math.sqrt(sq / row["n"])))[0] for sq in row["sq"]]


def bits(v):
    """A value as what is compared: a double by its bytes, anything else as it is; containers element by element."""
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, dict):
        return {k: bits(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [bits(x) for x in v]
    return v


def summary(rows_by_pair):
    """rows_by_pair: pair name -> [(n, pair dict)] over the tensors that have the pair.  The checkpoint's totals: math.fsum for
    the doubles, integer sums for the counts, the same derived measures."""
    out = {}
    for name, items in rows_by_pair.items():
        ps = [p for _, p in items]
        total = {"tensors": len(ps), "n": sum(n for n, _ in items)}
        total.update({k: math.fsum(p[k] for p in ps) for k in ("sq_a", "sq_b") + SUMS})
        total.update({k: sum(p[k] for p in ps) for k in COUNTS})
        total.update(derived(total))
        out[name] = total
    return out
