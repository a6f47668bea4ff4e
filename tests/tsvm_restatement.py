"""Numpy restatement of the TSV-M rule (include/vlm_hip.h), float64, through np.linalg.svd -- and of the one-sided Jacobi sweep the
device runs (csrc/jacobi.hip), pair formulas and tournament included, for choosing sweep counts without a GPU.

`flip=True` takes the first SVDs on tau^T instead of tau: the same rule through another LAPACK path.  The difference between the two
results is the restatement's own noise (`spread`)."""
import numpy as np

F = np.float32
D64 = np.float64
POLAR_FLOOR = 2.0 ** -40


def taus(c, srcs):
    return [w.astype(D64) - c.astype(D64) for w in srcs]


def polar(B):
    """(sum over sigma_j > 2^-40 sigma_max of p_j q_j^T, the number of directions dropped) of B = P diag(sigma) Q^T."""
    P, sig, Qt = np.linalg.svd(B, full_matrices=False)
    if sig.size == 0 or not sig[0] > 0:
        return np.zeros_like(B), int(sig.size)
    keep = sig > POLAR_FLOOR * sig[0]
    return P[:, keep] @ Qt[keep], int((~keep).sum())


def truncation(tau, k, flip=False):
    """(U_k [m, k], s [r], V_k [n, k]) of the thin SVD of tau, singular values descending; columns of zero triplets are zero."""
    if flip:
        v, s, ut = np.linalg.svd(tau.T, full_matrices=False)
        u, vt = ut.T, v.T
    else:
        u, s, vt = np.linalg.svd(tau, full_matrices=False)
    live = (s[:k] > 0).astype(D64)
    return u[:, :k] * live, s, vt[:k].T * live


def tsvm(c, srcs, lam, flip=False):
    """The rule for one matrix with S >= 2 sources.  Returns a dict: out (fp32), T (the merged task vector, float64), k, scat,
    s (per source, all of them), dropped (U, V)."""
    m, n = c.shape
    S = len(srcs)
    k = min(m, n) // S
    ts = taus(c, srcs)
    if k == 0:
        T = np.zeros((m, n), D64)
        return dict(out=c.copy(), T=T, k=0, scat=np.zeros(0, D64), s=[np.linalg.svd(t, compute_uv=False) for t in ts], dropped=(0, 0))
    parts = [truncation(t, k, flip) for t in ts]
    Ucat = np.concatenate([p[0] for p in parts], axis=1)
    Vcat = np.concatenate([p[2] for p in parts], axis=1)
    scat = np.concatenate([p[1][:k] for p in parts])
    Uo, du = polar(Ucat)
    Vo, dv = polar(Vcat)
    T = (Uo * scat) @ Vo.T
    return dict(out=finish(c, T, lam), T=T, k=k, scat=scat, s=[p[1] for p in parts], dropped=(du, dv))


def finish(c, T, lam):
    """dst = fl32(c + lam * T): product and sum in float64, one rounding."""
    return (c.astype(D64) + D64(lam) * T).astype(F)


def rank_k(tau, k):
    u, s, vt = np.linalg.svd(tau, full_matrices=False)
    return (u[:, :k] * s[:k]) @ vt[:k]


def ulp_diff(a, b):
    """Per element, how many float32 values lie between a and b (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-(2 ** 31)) - i, i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------------- the device's sweep
def steps(p):
    return 0 if p < 2 else (p if p & 1 else p - 1)


def pairs(p, step):
    """The (i, j) of a tournament step (csrc/jacobi_schedule.h): two int arrays of floor(p / 2) entries, i < j."""
    n = p + (p & 1)
    ring = n - 1
    k = np.arange(p >> 1) + (p & 1)
    a = np.where(k == 0, n - 1, (step + k) % ring)
    b = np.where(k == 0, step, (step + ring - k) % ring)
    return np.minimum(a, b), np.maximum(a, b)


def sweep(A, R):
    """One sweep of the one-sided Jacobi iteration on the rows of A [p, q] (R takes the same rotations), in place.  Returns
    (rotations, the largest |gamma| / sqrt(alpha beta))."""
    p, q = A.shape
    thr = np.sqrt(D64(q)) * 2.0 ** -53
    rot, off = 0, 0.0
    for t in range(steps(p)):
        i, j = pairs(p, t)
        ai, aj = A[i], A[j]
        alpha, beta, gamma = (ai * ai).sum(1), (aj * aj).sum(1), (ai * aj).sum(1)
        ab = np.sqrt(alpha * beta)
        go = np.abs(gamma) > thr * ab
        with np.errstate(divide="ignore", invalid="ignore"):
            off = max(off, float(np.where(ab > 0, np.abs(gamma) / ab, 0.0).max(initial=0.0)))
            zeta = (beta - alpha) / (2.0 * gamma)
            tt = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
        tt = np.where(go, tt, 0.0)
        cs = 1.0 / np.sqrt(1.0 + tt * tt)
        sn = cs * tt
        A[i], A[j] = cs[:, None] * ai - sn[:, None] * aj, sn[:, None] * ai + cs[:, None] * aj
        ri, rj = R[i], R[j]
        R[i], R[j] = cs[:, None] * ri - sn[:, None] * rj, sn[:, None] * ri + cs[:, None] * rj
        rot += int(go.sum())
    return rot, off


def jacobi(A0, cap=30):
    """Sweeps until one rotates nothing.  Returns (A = diag(s) V^T, R = U^T, the rotations of every sweep)."""
    A = np.array(A0, D64)
    R = np.eye(A.shape[0])
    counts = []
    while len(counts) < cap and A.shape[0] > 1:
        counts.append(sweep(A, R)[0])
        if counts[-1] == 0:
            break
    return A, R, counts


# ---------------------------------------------------------------------------------------------------------------- inputs
# working shapes (p, q) of the primitive; the merge takes each tall and wide
SHAPES = [(1, 1), (2, 3), (5, 7), (8, 8), (33, 70), (64, 192), (96, 288)]


# the merge: every working shape tall and wide, S = 2 and 3 (lam = 0.75 and 1 share an input)
MERGE_CASES = sorted({(m, n, S) for (p, q) in SHAPES for (m, n) in ((p, q), (q, p)) for S in (2, 3)})


# Past the limits of csrc/jacobi.hip and csrc/tsvm.hip, kept apart from SHAPES and MERGE_CASES so that no other parametrised test
# grows: the step kernel is instantiated for PER = 1, 2, 4, 8, 12, 16, 32 doubles per lane and row and dispatched by ceil(q / 256).
PAIR_Q = [300, 768, 1100, 3072, 3073, 8192]             # one q per instantiation above PER = 1: 2, 4, 8, 12, 16, 32
# skinny: the first and the last q of every instantiation from 4 up, each run as given and tall
BOUNDARY_SKINNY = [(2, 513), (3, 1024), (2, 1025), (3, 2048), (2, 2049), (3, 3072), (2, 3073), (3, 4096), (2, 4097), (3, 8192), (4, 768)]
# p > 256: the second register slot of a row of R and the second trip of the rank loop; p p > 1024 x 256: the reset grid's cap
BOUNDARY_TALL = [(257, 300), (513, 520)]
# m n > 256 x 1024 (the delta grid's cap); the second has kS = 513 = p, ragged by one against the 16-row stage of the apply
BOUNDARY_MERGE = [(513, 520, 2), (520, 513, 3)]


def pair_columns(q):
    """The first and the last element of every 256-wide register slot a row of q doubles fills, with 0 and q - 1."""
    cols = {0, q - 1}
    for u in range((q + 255) // 256):
        cols |= {u * 256, min(u * 256 + 255, q - 1)}
    return sorted(cols)


def duplicate_pairs(q):
    """(A [2 L, q], C, v): rows 2a and 2a + 1 both hold the single entry v[a] = (-1)^a 2^-(a % 20) at column C[a] = pair_columns(q)[a].
    Distinct pairs have disjoint supports (gamma = 0: no rotation); a duplicate pair has alpha = beta = gamma: zeta = 0, t = 1,
    c = s, and its one rotation leaves row 2a exactly zero and row 2a + 1 = (c v + c v) e_C[a]."""
    C = pair_columns(q)
    v = np.array([(-1.0) ** a * 2.0 ** -(a % 20) for a in range(len(C))])
    A = np.zeros((2 * len(C), q))
    for a, col in enumerate(C):
        A[2 * a, col] = A[2 * a + 1, col] = v[a]
    return A, C, v


def check_duplicate_pairs(C, v, s, Vt, Rm, rotations):
    """What a Jacobi SVD of duplicate_pairs(q) gives, with no tolerance beyond the rounding of c = 1 / sqrt(2) itself: s [2 L] the
    row norms, Vt [2 L, q] the unit rows (zero rows where s = 0), Rm [2 L, 2 L] the accumulated rotations, rotations per sweep."""
    L = len(C)
    assert list(rotations) == [L, 0]                                       # every duplicate pair once; the second sweep rotates nothing
    assert int((s == 0.0).sum()) == L and not s[0::2].any()                # one exact zero per pair: a slot never loaded or stored breaks it
    want = np.sqrt(2.0) * np.abs(v)
    assert (np.abs(s[1::2] - want) <= 2 * np.spacing(want)).all()
    hot = np.zeros_like(Vt)
    hot[2 * np.arange(L) + 1, C] = np.sign(v)                              # (c v + c v) / |c v + c v|: exactly +-1 at the planted column
    assert np.array_equal(Vt, hot)
    c = 1.0 / np.sqrt(2.0)
    a = 2 * np.arange(L)
    blocks = np.stack([Rm[a, a], -Rm[a, a + 1], Rm[a + 1, a], Rm[a + 1, a + 1]])   # (c, -s; s, c) with s = c
    assert (np.abs(blocks - c) <= np.spacing(c)).all()
    rest = Rm.copy()
    for d in ((0, 0), (0, 1), (1, 0), (1, 1)):
        rest[a + d[0], a + d[1]] = 0.0
    assert not rest.any()


def gaussian(p, q, seed=0):
    return np.random.default_rng(5000 * p + q + seed).standard_normal((p, q))


def planted(m, n, S, seed=0, scale=0.02):
    """c Gaussian fp32 and S sources whose task vectors have a PLANTED GAP at the cut k = min(m, n) // S: seeded orthogonal factors,
    the top k singular values geometric from 1 to 0.5, the rest geometric from 0.05 down to 0.005 (times `scale`).  The sources are
    fp32, so the task vectors are the planted matrices as fp32 arithmetic leaves them."""
    rng = np.random.default_rng(7000 * m + 10 * n + S + seed)
    r = min(m, n)
    k = r // S
    c = rng.standard_normal((m, n)).astype(F)
    srcs = []
    for _ in range(S):
        sig = np.concatenate([np.geomspace(1.0, 0.5, k) if k else np.zeros(0), np.geomspace(0.05, 0.005, r - k) if r > k else np.zeros(0)])
        u, _ = np.linalg.qr(rng.standard_normal((m, r)))
        v, _ = np.linalg.qr(rng.standard_normal((n, r)))
        srcs.append((c + (scale * (u * sig) @ v.T).astype(F)).astype(F))
    return c, srcs


def exact_case(m, n, S, lam_pow=0, with_central=False, seed=0):
    """Task vectors that are signed permutations times diagonals of DISTINCT powers of two with disjoint row and column supports
    across the experts: expert i owns rows and columns [i w, (i + 1) w), w = min(m, n) // S, one entry per owned row.  c is zero,
    so every W_i is its task vector.  Returns (c, srcs, the closed-form merged task vector for k = w)."""
    rng = np.random.default_rng(31 * m + n + S + seed)
    w = min(m, n) // S
    c = np.zeros((m, n), F)
    srcs, total = [], np.zeros((m, n), D64)
    for i in range(S):
        t = np.zeros((m, n), F)
        if not (with_central and i == S - 1):
            cols, exps = rng.permutation(w), rng.permutation(w)
            for a in range(w):
                t[i * w + a, i * w + cols[a]] = F((-1.0) ** int(rng.integers(2)) * 2.0 ** -int(exps[a]))
        srcs.append(t)
        total += t
    return c, srcs, total
