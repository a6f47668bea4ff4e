"""Numpy restatement of the WUDI rule (include/vlm_hip.h), float64: the setup (n_i, G, B, K, X_0), the Adam steps in the operation
order of torch.optim.Adam, the output.  `permute=True` forms G and X G with the reduction index permuted: the same rule with the
matrix products summed in another order -- the difference between the two modes is the restatement's own noise floor."""
import numpy as np

F = np.float32
D64 = np.float64
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def taus(c, srcs):
    return [w.astype(D64) - c.astype(D64) for w in srcs]


def setup(c, srcs, permute=False):
    """(tau list, n list, G, B, K, X_0) of the rule's steps 1 - 3."""
    ts = taus(c, srcs)
    m, n = c.shape
    rows = np.random.default_rng(7).permutation(m) if permute else np.arange(m)
    ns = [D64((t * t).sum()) for t in ts]
    G, B, K = np.zeros((n, n), D64), np.zeros((m, n), D64), D64(0)
    X0 = np.zeros((m, n), D64)
    for t, sq in zip(ts, ns):
        w = D64(1) / sq if sq > 0 else D64(0)
        Gi = w * (t[rows].T @ t[rows])
        G = G + Gi
        B = B + t @ Gi
        K = K + sq * D64((Gi * Gi).sum())
        X0 = X0 + t
    return ts, ns, G, B, K, X0


def wudi(c, srcs, lam, iters, lr=1e-5, permute=False):
    """The rule.  Returns a dict: out (fp32), X (X_T), X0, losses (loss_0 .. loss_{T-1}), loss_first, loss_last, sq."""
    ts, ns, G, B, K, X = setup(c, srcs, permute)
    n = c.shape[1]
    cols = np.random.default_rng(11).permutation(n) if permute else np.arange(n)
    X0 = X.copy()
    M, V = np.zeros_like(X), np.zeros_like(X)
    losses = []
    for t in range(1, iters + 1):
        XG = X[:, cols] @ G[cols, :]
        losses.append(float((X * (XG - 2.0 * B)).sum() + K))
        g = 2.0 * (XG - B)
        M = BETA1 * M + (1.0 - BETA1) * g
        V = BETA2 * V + ((1.0 - BETA2) * g) * g
        step = lr / (1.0 - BETA1 ** t)
        bc2s = np.sqrt(D64(1.0 - BETA2 ** t))
        X = X - step * (M / (np.sqrt(V) / bc2s + EPS))
    return dict(out=finish(c, X, lam), X=X, X0=X0, losses=losses, loss_first=losses[0], loss_last=losses[-1], sq=[float(v) for v in ns])


def finish(c, X, lam):
    """dst = fl32(c + lam * X): product and sum in float64, one rounding."""
    return (c.astype(D64) + D64(lam) * X).astype(F)


def loss_by_definition(c, srcs, X):
    """L(X) = sum_i (1 / ||tau_i||_F^2) ||(X - tau_i) tau_i^T||_F^2."""
    total = 0.0
    for t in taus(c, srcs):
        sq = (t * t).sum()
        if sq > 0:
            r = (X - t) @ t.T
            total += float((r * r).sum() / sq)
    return total


def ulp_diff(a, b):
    """Per element, how many float32 values lie between a and b (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 31)) - i, i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------------------------- inputs
# (m, n, S): ragged tiles; a wide matrix whose reduction 80 is no multiple of 16; 3 x 2 tiles with a ragged reduction; exactly one
# tile; one row; one column
SHAPES = [(80, 48, 2), (48, 80, 3), (130, 70, 2), (64, 64, 2), (1, 130, 2), (67, 1, 3)]
STEPS = [1, 7, 40]
LONG = ((80, 48, 2), 300)   # one run at the default step count
# Past the limits of csrc/wudi.hip, kept apart from SHAPES so that no other parametrised test grows, ((m, n, S), steps): 727 x 723 is
# odd, above 256 workgroups x 2048 elements (the stride loops' second trip) and 12 x 12 = 144 tiles (the loss fold's third trip),
# tall and wide because the sum grid takes the larger of [m][n] and [n][n]; 363 x 362 gives 65 partials (the fold's second trip)
BOUNDARY_CASES = [((727, 723, 2), 7), ((723, 727, 3), 7), ((363, 362, 2), 40)]


def inputs(m, n, S, s=1e-3, seed=0):
    """c = 0.02 N(0, 1) and W_i = c + s N(0, 1), float32."""
    rng = np.random.default_rng(1000 * m + n + seed)
    c = (F(0.02) * rng.standard_normal((m, n)).astype(F)).astype(F)
    return c, [(c + F(s) * rng.standard_normal((m, n)).astype(F)).astype(F) for _ in range(S)]


def case(m, n, S):
    """The inputs of a row of SHAPES: task vectors of size 1e-3, for (130, 70) of size 2e-2."""
    return inputs(m, n, S, s=2e-2 if (m, n) == (130, 70) else 1e-3)


def grid_inputs(m, n, S, seed=0):
    """c and every W_i integer multiples of 2^-10 with |value| < 4: c + sum_i (W_i - c) is exact in float32."""
    rng = np.random.default_rng(77 + 1000 * m + n + seed)
    def draw():
        return (rng.integers(-4095, 4096, size=(m, n)) / 1024.0).astype(F)
    return draw(), [draw() for _ in range(S)]
