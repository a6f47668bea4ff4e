"""Numpy restatement of the Iso-C rule (include/vlm_hip.h), float64: the definition through an SVD, the QDWH iteration the device
runs, step for step, and the two elementwise ends of the device's pipeline in its order of operations."""
import numpy as np

F = np.float32
D64 = np.float64


def schedule(l0=1e-6, steps=8):
    """The formulas of the iteration's coefficients, in numpy doubles."""
    out, l = [], D64(l0)
    for _ in range(steps):
        if l >= 1.0:
            a, b, c = D64(3), D64(1), D64(3)
        else:
            d = np.cbrt(4 * (1 - l ** 2) / l ** 4)
            a = np.sqrt(1 + d) + 0.5 * np.sqrt(8 - 4 * d + 8 * (2 - l ** 2) / (l ** 2 * np.sqrt(1 + d)))
            b = (a - 1) ** 2 / 4
            c = a + b - 1
        out.append((float(a), float(b), float(c)))
        l = min(D64(1), l * (a + b * l ** 2) / (1 + c * l ** 2))
    return out


def delta(c, srcs):
    """D = ((0 + (W_0 - c)) + (W_1 - c)) + ... in float64, in the tensor's own orientation."""
    d = np.zeros(c.shape, D64)
    for w in srcs:
        d = d + (w.astype(D64) - c.astype(D64))
    return d


def working(d):
    """The orientation the device works in: [rows >= cols]."""
    return np.ascontiguousarray(d.T) if d.shape[0] < d.shape[1] else d


def polar_svd(d):
    """(U V^T over the singular values above 1e-13 sigma_max, sum sigma) of a matrix, through the SVD."""
    u, s, vt = np.linalg.svd(d, full_matrices=False)
    if s.size == 0 or s[0] == 0:
        return np.zeros_like(d), 0.0
    k = int((s > 1e-13 * s[0]).sum())
    return u[:, :k] @ vt[:k], float(s.sum())


def finish(c, X, nuclear, lam, r):
    """dst = fl32(c + ((lam * nuclear) / r) * X): X in the tensor's own orientation, product and sum separate, one rounding."""
    s = (D64(lam) * D64(nuclear)) / D64(r)
    return (c.astype(D64) + s * X).astype(F)


def iso_svd(c, srcs, lam):
    """The rule by its definition.  Returns (dst, Q, nuclear); dst = c where D = 0."""
    d = delta(c, srcs)
    if not np.any(d):
        return c.copy(), np.zeros_like(d), 0.0
    q, nuc = polar_svd(d)
    return finish(c, q, nuc, lam, min(d.shape)), q, nuc


def qdwh(d, l0=1e-6, steps=8, extra=0):
    """The iteration on a matrix [rows >= cols]: (X, the Frobenius norms of the steps).  `extra` further (3, 1, 3) steps."""
    alpha = np.sqrt((d * d).sum())
    X = d / alpha
    eye = np.eye(d.shape[1])
    norms = []
    for a, b, c in schedule(l0, steps) + [(3.0, 1.0, 3.0)] * extra:
        Z = eye + c * (X.T @ X)
        Lc = np.linalg.cholesky(Z)
        Y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, X.T)).T   # X (L L^T)^-1
        Xn = (b / c) * X + (a - b / c) * Y
        norms.append(float(np.sqrt(((Xn - X) ** 2).sum())))
        X = Xn
    return X, norms


def iso_qdwh(c, srcs, lam, l0=1e-6, steps=8, extra=0):
    """The rule through the iteration.  Returns (dst, X in the tensor's orientation, nuclear, step norms)."""
    d = delta(c, srcs)
    if not np.any(d):
        return c.copy(), np.zeros_like(d), 0.0, []
    w = working(d)
    X, norms = qdwh(w, l0, steps, extra)
    nuc = float((X * w).sum())
    Xo = X.T if d.shape[0] < d.shape[1] else X
    return finish(c, Xo, nuc, lam, min(d.shape)), Xo, nuc, norms


def ulp_diff(a, b):
    """Per element, how many float32 values lie between a and b (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 31)) - i, i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------------------------- inputs
SHAPES = [(16, 16, 2), (48, 16, 3), (16, 32, 2), (40, 24, 4), (130, 70, 2), (200, 72, 3), (257, 129, 2)]
# Past the limits of csrc/isoc.hip, kept apart from SHAPES so that no other parametrised test grows: 363 x 362 gives 65 partials
# (the one-wave fold's second trip), 727 x 723 = 525 621 elements, odd and above 256 workgroups x 2048 (the stride loops' second
# trip); each tall and wide, because the device works on the transpose when m < n.
BOUNDARY_SHAPES = [(363, 362, 3), (362, 363, 2), (727, 723, 2), (723, 727, 2)]


def planted_delta(m, n, sig, rng):
    """A float64 [m, n] matrix with the singular values sig."""
    u, _ = np.linalg.qr(rng.standard_normal((m, len(sig))))
    v, _ = np.linalg.qr(rng.standard_normal((n, len(sig))))
    return (u * sig) @ v.T


def inputs(m, n, S, seed=0, spectrum=None, zero_cols=None):
    """c Gaussian fp32, sources c + 0.02 * Gaussian; `spectrum`: the first source carries a planted task vector with these
    singular values instead and the others equal c (their task vectors are exact zeros, so D is the planted matrix as fp32
    arithmetic leaves it); `zero_cols`: those columns of every source equal c's."""
    rng = np.random.default_rng(1000 * m + n + seed)
    c = rng.standard_normal((m, n)).astype(F)
    if spectrum is None:
        srcs = [(c + F(0.02) * rng.standard_normal((m, n)).astype(F)).astype(F) for _ in range(S)]
    else:
        srcs = [(c + planted_delta(m, n, np.asarray(spectrum, D64), rng).astype(F)).astype(F)] + [c.copy() for _ in range(S - 1)]
    if zero_cols is not None:
        for s in srcs:
            s[:, zero_cols] = c[:, zero_cols]
    return c, srcs


def case(m, n, S):
    """The inputs of a row of SHAPES."""
    if (m, n) == (130, 70):
        return inputs(m, n, S, zero_cols=slice(5, 9))
    if (m, n) == (200, 72):
        return inputs(m, n, S, spectrum=np.geomspace(1.0, 1e-3, 72))
    return inputs(m, n, S)
