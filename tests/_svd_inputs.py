"""Inputs of test_gpu_svd.py and a numpy replay of the route decisions svd.hip::gesdd_tall takes on them.

gesdd_tall chooses by data.  With G = A^T A, R1 = chol(G), Q = A R1^-1, G2 = Q^T Q, R = chol(G2) R1 (or R1):
  a  Gram route          fp64, 32 < n <= 256, cond(A)^2 <= 1e3 (the sweeps' norm monitor) and max |U^T U - I| <= 1e-13
  e  Jacobi on A         chol(G) fails, or max / min |diag R1| >= 1e7 (fp64) / 1e3 (fp32)
  c  one pass            max |G2 - I| <= 1e-13 / 5e-6: the second factorization is skipped
  f  undo                chol(G2) fails
  b  Cholesky-QR twice   otherwise
  d  V recovered         (beside b or c) diagonal ratio < 1e3 and ||R||_F ||R^-1||_F < 1e3 / 30
`replay` evaluates these quantities in the precision of the call and returns the routes together with the smallest factor by which a
quantity that decided them cleared its threshold; test_svd_inputs.py holds every ROUTE_CASES entry to its route with a factor >= 10, so
that a different summation order on the device cannot move a GPU case to another route."""
import numpy as np

LIM = {
    "f64": dict(ratio=1e7, one_pass=1e-13, rinv=1e3, eps=np.finfo(np.float64).eps),
    "f32": dict(ratio=1e3, one_pass=5e-6, rinv=30.0, eps=float(np.finfo(np.float32).eps)),
}
NPDT = {"f64": np.float64, "f32": np.float32}


def _orth(rng, m, n):
    return np.linalg.qr(rng.standard_normal((m, n)))[0]


def with_spectrum(m, n, s, seed, rotate=True):
    """U diag(s) V^T with Haar-like U (m x n) and V (n x n); rotate=False keeps V = I, so that column j has norm s[j] (a graded matrix)"""
    rng = np.random.default_rng(seed)
    U = _orth(rng, m, n)
    return (U * s) @ _orth(rng, n, n).T if rotate else U * s


def kahan(n, theta, perturb=0.0):
    """the Kahan matrix as rlhip_gen_kahan builds it (upper triangular, rows scaled by sin^i)"""
    sn, cs = np.sin(theta), np.cos(theta)
    K = np.triu(-cs * np.ones((n, n)), 1) + np.eye(n)
    K = (sn ** np.arange(n))[:, None] * K
    return K + np.diag(perturb * np.finfo(np.float64).eps * (n - np.arange(n)))


def rank_deficient(m, n, r, seed):
    """exact rank r (in exact arithmetic): the product of an m x r and an r x n factor with small integer entries, so that the product is exact
    in both precisions and its rank is r whatever the rounding"""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, (m, r)).astype(np.float64) @ rng.integers(-4, 5, (r, n)).astype(np.float64)


def _chol_upper(G):
    try:
        R = np.linalg.cholesky(G).T
    except np.linalg.LinAlgError:
        return None
    return R if np.all(np.isfinite(R)) else None


def replay(A, prec, gram=True):
    """-> (routes, margin, numbers): routes a subset string of 'abcdef' as svd.hip would take them on A in precision `prec` (gram: the
    gesdd_gram option), margin the smallest threshold / value (or value / threshold) factor among the decisions taken"""
    lim, dt = LIM[prec], NPDT[prec]
    A = np.asarray(A).astype(dt)
    m, n = A.shape
    num = {}
    margins = []

    def below(name, v, thr):            # v <= thr decided the route
        num[name] = float(v)
        margins.append(thr / max(float(v), 1e-300))

    def above(name, v, thr):
        num[name] = float(v)
        margins.append(float(v) / thr)

    if gram and prec == "f64" and 32 < n <= 256:
        s = np.linalg.svd(A, compute_uv=False)
        cond2 = (s[0] / s[-1]) ** 2 if s[-1] > 0 else np.inf
        lam, V = np.linalg.eigh(A.T @ A)
        with np.errstate(all="ignore"):
            W = V / np.sqrt(np.abs(lam))
            defect = np.abs(W.T @ (A.T @ A) @ W - np.eye(n)).max() if np.all(lam > 0) else np.inf
        if cond2 <= 1e3 and defect <= 1e-13:
            below("cond2", cond2, 1e3)
            below("gram_defect", defect, 1e-13)
            return "a", min(margins), num
        num["cond2"], num["gram_defect"] = float(cond2), float(defect)
        margins.append(max(cond2 / 1e3, defect / 1e-13))
    G = A.T @ A
    R1 = _chol_upper(G)
    if R1 is None:
        num["chol1"] = 0.0
        return "e", min(margins + [np.inf]), num
    dg = np.abs(np.diag(R1)).astype(np.float64)
    ratio = dg.max() / dg.min()
    if ratio >= lim["ratio"]:
        above("ratio", ratio, lim["ratio"])
        return "e", min(margins), num
    below("ratio", ratio, lim["ratio"])
    Q = np.linalg.solve(R1.T, A.T).T.astype(dt)
    G2 = Q.T @ Q
    dev = np.abs(np.triu(G2 - np.eye(n, dtype=dt))).max()
    one_pass = dev <= lim["one_pass"]
    if one_pass:
        below("dev", dev, lim["one_pass"])
        R, routes = R1, "c"
    else:
        above("dev", dev, lim["one_pass"])
        R2 = _chol_upper(G2)
        lmin = np.linalg.eigvalsh(G2.astype(np.float64)).min()
        num["lmin_G2"] = float(lmin)
        noise = n * lim["eps"] * np.abs(G2).max()
        if R2 is None:
            margins.append(-lmin / noise if lmin < 0 else 0.0)      # f only counts when G2 is indefinite beyond rounding
            return "f", min(margins), num
        margins.append(lmin / noise)
        R, routes = (R2 @ R1).astype(dt), "b"
    nrni = np.linalg.norm(R.astype(np.float64)) * np.linalg.norm(np.linalg.inv(R.astype(np.float64)))
    num["nrni"] = float(nrni)
    if ratio < 1e3 and nrni < lim["rinv"]:
        margins.append(min(1e3 / ratio, lim["rinv"] / nrni))
        routes += "d"
    else:
        margins.append(max(ratio / 1e3, nrni / lim["rinv"]))
    return routes, min(margins), num


def _dup(m, n, seed, zero=False):
    """well-conditioned columns, the last one an exact copy of column 1 (or exactly zero).  The copied pair is scaled by 2^-5 (exact), so
    that even a factorization that squeezes a pivot of sqrt(eps) out of the copy leaves a diagonal ratio 32 times past that"""
    A = with_spectrum(m, n, np.linspace(2.0, 1.0, n), seed)
    A = np.round(A * 2.0 ** 12) / 2.0 ** 12            # (few bits: the fp32 input equals the fp64 one)
    if zero:
        A[:, n - 1] = 0.0
    else:
        A[:, 1] *= 2.0 ** -5
        A[:, n - 1] = A[:, 1]
    return A


# name -> (builder, precisions, gram option, expected routes).  Not reachable with a factor 10 on every decision, and therefore absent:
#   b + d   d needs ||R|| ||R^-1|| <= 100 / 3, i.e. cond <= 100 / n <= 3 and cond ~ 1; b needs max |Q^T Q - I| ~ eps cond^2 >= 1e-12 / 5e-5,
#           i.e. cond >= 100 / 30: in fp64 the two meet in one point where rounding decides, in fp32 they exclude each other;
#   c (fp32, n > 2) without d needs n >= 300 columns whose Gram matrix is the identity to 5e-7, below fp32 summation noise at that size;
#   f       the second factorization fails only when eps cond^2 ~ 1, where the first one already fails or shows a diagonal ratio past
#           its limit; Kahan matrices (n = 40 .. 90, theta = 1.0 .. 1.2) reach it in fp32 with an indefiniteness of 1e-8, at rounding level.
ROUTE_CASES = {
    "gram_wellcond": (lambda: with_spectrum(2000, 64, np.linspace(2.0, 1.0, 64), 1), ("f64",), True, "a"),
    "onepass_recover": (lambda: with_spectrum(2000, 64, np.linspace(2.0, 1.0, 64), 1), ("f64",), False, "cd"),
    "onepass_recover_n2": (lambda: with_spectrum(64, 2, np.array([1.0, 1.0]), 2), ("f64", "f32"), False, "cd"),
    "onepass_small": (lambda: with_spectrum(300, 24, np.linspace(1.5, 1.0, 24), 3), ("f64",), False, "cd"),
    "twopass_cond1e5": (lambda: with_spectrum(3000, 128, np.logspace(0, -5, 128), 4), ("f64",), False, "b"),
    "twopass_cond3e3": (lambda: with_spectrum(1000, 48, np.logspace(0, -3.5, 48), 5), ("f64",), True, "b"),
    "twopass_cond160_f32": (lambda: with_spectrum(1000, 48, np.logspace(0, -2.2, 48), 6), ("f32",), False, "b"),
    "graded_ratio": (lambda: with_spectrum(1500, 64, np.logspace(0, -9, 64), 7, rotate=False), ("f64",), True, "e"),
    "graded_ratio_f32": (lambda: with_spectrum(1500, 64, np.logspace(0, -5, 64), 7, rotate=False), ("f32",), False, "e"),
    "duplicate_column": (lambda: _dup(800, 40, 8), ("f64", "f32"), True, "e"),
    "zero_column": (lambda: _dup(800, 40, 9, zero=True), ("f64", "f32"), True, "e"),
}
