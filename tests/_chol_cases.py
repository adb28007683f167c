"""Cases of test_gpu_chol.py, their input builders, the bounds and a plain-Python replay of the route that chol.hip takes
(rlhip::potrf_upper, potrf_small_kernel, chol_rowsolve_kernel).  tests/test_chol_cases.py checks the tables, the conditions and a plain
NumPy Cholesky in the working precision against every limit the device is held to.

Routes.  n <= PS_MAXN = 448: potrf_small_kernel alone ("small"), 32-wide panels (jb32, rest32); the trailing update of a panel runs on
16 x 16 MFMA tiles over ceil(rest32 / 16) * 16 columns, the padding columns zeroed in LDS.  Larger n ("two-level"): 256-wide steps
(j0, jb, rest) of {potrf_small_kernel on the diagonal block, chol_rowsolve_kernel on the block row, the K = 256 GEMM on the trailing
matrix}; a block row exists only right of a full block, so chol_rowsolve_kernel always runs with jb = 256.  There are no counters: route(n)
exists so that the table below can state which edge a size hits (test_chol_cases.py holds the table to it).

Family E (exact; one definition for both precisions).  A = U^T U with U upper triangular and integer: the diagonal from {1, 2, 4}, at most
three entries from {-2, -1, 1, 2} per column above it, at random rows.  |a_ij| <= 16 + 3 * 4 = 28 (Cauchy-Schwarz on two columns), so A
is exact in fp32, and every Schur complement is (U[k:, k:])^T U[k:, k:], a matrix of the same kind.  The device takes r = sqrt(d) for
d in {1, 4, 16} exactly (Newton on the hardware seed, then one Heron step), y = 1 / sqrt(d) exactly or one bit below (2^-k (1 - 2^-53)).
  fp32: (float)y is the power of two, (float)((double)a y) is the integer it should be, chol_rowsolve_kernel divides by the exact r, every
        sum is of integers far below 2^24: the factor is U bit for bit, on every route.
  fp64: the last bit of y may stay, amplified by the conditioning of U: max |R - U| <= tol_E,
            tol_E = sqrt(2) kappa_2(A) eps ||U||_2,    eps = gamma_(n+3) || |U|^T |U| ||_F / ||A||_2,    u = 2^-53,
        Higham, Accuracy and Stability, Theorem 10.8 with the backward error of Theorem 10.3 (n + 3: two roundings of a y against one
        division).  Evaluated in float64 from the singular values of U (||A||_2 = s_max^2, kappa_2(A) = (s_max / s_min)^2: A = U^T U
        exactly).  An indexing, tile or padding error moves an integer a_kj by at least 1 and so some u_kj by at least 1 / 4.
Conditions of the table, for every listed n (checked on the CPU): kappa_2(A) eps <= 1 / 2, tol_E <= 2^-6, max |A| < 2^24.  A size that
misses one is thinned (E_LEVEL: two entries of +-1 per column, then one, then none); the conditions stay.

Family R (rounding).  G = X^T X / (2 n), X Gaussian (2 n + 3) x n, rounded to the precision under test; the rounded matrix is A.
Entrywise on the upper triangle, in float64 with the device's R:
            |A - R^T R| <= gamma_(n+3) |R|^T |R|,    u from UNIT_ROUNDOFF,
for any summation order (the LDS MFMA tiles, the fp32 GEMM of the two-level update, the register panel); doubled for fp64 data, whose
float64 evaluation of the residual obeys the same bound (as test_gpu_lu.py and test_gpu_tri.py do).  There is no other factor.

Family F (failure; exact integers).  A family E matrix with the pivot at k = position - 1 spoiled:
  neg   A[k, k] -= u_kk^2 + 1: in exact arithmetic the k-th updated pivot is -1, and tol_E << 1 keeps it negative in fp64;
  nan   A[k, k] = NaN (the diagonal only: where an off-diagonal NaN surfaces depends on the route);
  zero  row and column k of A zero: column k of U above the diagonal is then exactly zero and so is the pivot.
The return value is the position.  Rows 0 .. k - 1 of the factor are final through the last column of the failing pivot's 32-panel
(checked_columns) and equal U there (column k zero for 'zero'): bitwise in fp32, within tol_E in fp64.  The pivot entry holds its updated
value.  What lies right of and below the failing pivot's block is unspecified, as with dpotrf."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

from _tri_cases import NPDT, OFF, POISON, PRECS, UINT, UNIT_ROUNDOFF, poison_lower  # noqa: F401  (one set of conventions)

PS_MAXN, BS, NB = 448, 256, 32              # chol.hip: constexpr int PS_MAXN, constexpr int64_t BS, constexpr int NB
PAD_A = 5                                   # lda = n + PAD_A in the poison parent

SIZES = {
    1: "smallest", 2: "smallest",
    31: "one ragged 32-panel", 32: "one full 32-panel", 33: "rest = 1: one padded tile of 15 zero columns",
    47: "rest = 15: one padded tile", 48: "rest = 16: one full tile", 49: "rest = 17: the second tile holds one column",
    64: "two full 32-panels", 65: "two 32-panels and one column",
    255: "a ragged 256 block", 256: "a full 256 block (the CholQR Gram matrices)", 257: "256 and one column, still one workgroup",
    447: "below the one-workgroup maximum", 448: "the one-workgroup maximum, the largest LDS footprint",
    449: "first two-level size: jb = 256, rest = 193",
    511: "last block of 255 columns", 512: "last block of 256 columns", 513: "last block of 1 column",
    705: "three blocks, the last ragged in both levels", 768: "three full blocks",
}
E_LEVEL = {705: 1}                          # n -> thinning level of family E where level 0 misses a condition (705: tol_E = 0.148 > 2^-6)
E_LEVELS = ((3, (-2, -1, 1, 2)), (2, (-1, 1)), (1, (-1, 1)), (0, (1,)))
KAPPA_EPS_MAX, TOL_E_MAX, A_MAX = 0.5, 2.0 ** -6, 2 ** 24

F_POSITIONS = {40: (1, 32, 33, 40), 300: (97, 256, 257, 300), 449: (449,), 705: (3, 256, 257, 512, 513, 705)}
F_KINDS = ("neg", "nan", "zero")
REPEAT = ((705, 257, "neg"), 47, 449)       # a failing two-level call, then a small and a two-level success on the same context
CHOLQRQ_M, CHOLQRQ_K, CHOLQRQ_ZERO_COLUMN = 16384, 256, 100


def _seed(name):
    return zlib.crc32(name.encode())


def _gamma(t, u):
    return t * u / (1.0 - t * u)


# ---------------------------------------------------------------------------------------------------------------------------------------
# replay of the route
# ---------------------------------------------------------------------------------------------------------------------------------------
def panels(n):
    """potrf_small_kernel on n columns: (jb32, rest32) per 32-panel"""
    return tuple((min(NB, n - j0), n - j0 - min(NB, n - j0)) for j0 in range(0, n, NB))


@dataclass(frozen=True)
class Route:
    kind: str                    # "small" | "two-level"
    blocks: tuple                # (j0, jb, rest, panels(jb)) per 256-step; one entry (0, n, 0, panels(n)) for "small"

    @property
    def steps(self):
        return tuple(b[:3] for b in self.blocks)


def route(n):
    assert n >= 1
    if n <= PS_MAXN:
        return Route("small", ((0, n, 0, panels(n)),))
    out = []
    for j0 in range(0, n, BS):
        jb = min(BS, n - j0)
        out.append((j0, jb, n - j0 - jb, panels(jb)))
    return Route("two-level", tuple(out))


def padded_columns(rest32):
    """zero columns that pad the trailing update of a 32-panel to whole 16 x 16 tiles"""
    return -rest32 % 16


def checked_columns(n, k):
    """one past the last column of the 32-panel that holds pivot k: rows above a failing pivot k are final through it"""
    j0 = 0 if n <= PS_MAXN else (k // BS) * BS
    jb = n if n <= PS_MAXN else min(BS, n - j0)
    p0 = j0 + ((k - j0) // NB) * NB
    return min(p0 + NB, j0 + jb)


# ---------------------------------------------------------------------------------------------------------------------------------------
# family E
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family_e_master(n, level):
    """-> U, n x n int8 upper triangular"""
    count, values = E_LEVELS[level]
    rng = np.random.default_rng(_seed(f"chol-E-{n}"))
    U = np.zeros((n, n), dtype=np.int8)
    d = rng.choice(np.array([1, 2, 4], dtype=np.int8), n)
    for j in range(1, n):
        if count:
            U[rng.integers(0, j, count), j] = rng.choice(np.array(values, dtype=np.int8), count)
    U[np.arange(n), np.arange(n)] = d
    return U


@dataclass(frozen=True)
class ECase:
    n: int
    U: np.ndarray                # float64, integer entries
    A: np.ndarray                # float64, = U^T U exactly, symmetric
    tol: float                   # tol_E (fp64)
    kappa_eps: float             # kappa_2(A) eps
    kappa_u: float               # kappa_2(U)


def tol_e(U):
    """-> (tol_E, kappa_2(A) eps, kappa_2(U)) in float64 (module docstring)"""
    U = np.asarray(U, dtype=np.float64)
    n = U.shape[0]
    s = np.linalg.svd(U, compute_uv=False)
    norm_u, norm_a, kappa_a = s[0], s[0] ** 2, (s[0] / s[-1]) ** 2
    eps = _gamma(n + 3, UNIT_ROUNDOFF["f64"]) * np.linalg.norm(np.abs(U).T @ np.abs(U), "fro") / norm_a
    return float(np.sqrt(2.0) * kappa_a * eps * norm_u), float(kappa_a * eps), float(s[0] / s[-1])


@functools.lru_cache(maxsize=None)
def family_e(n, level=None):
    U = _family_e_master(n, E_LEVEL.get(n, 0) if level is None else level).astype(np.float64)
    tol, ke, ku = tol_e(U)
    return ECase(n, U, U.T @ U, tol, ke, ku)


def conditions_hold(e):
    return e.kappa_eps <= KAPPA_EPS_MAX and e.tol <= TOL_E_MAX and np.abs(e.A).max() < A_MAX


def stored(A, prec):
    """the symmetric A as the device gets it: the precision under test, NaN-payload poison strictly below the diagonal"""
    return poison_lower(A, prec, False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# family R
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def family_r(n, prec):
    """-> A: G = X^T X / (2 n) rounded to the precision under test, symmetric, as float64"""
    rng = np.random.default_rng(_seed(f"chol-R-{n}"))
    X = rng.standard_normal((2 * n + 3, n))
    G = np.triu((X.T @ X) / (2.0 * n)).astype(NPDT[prec]).astype(np.float64)
    return G + np.triu(G, 1).T


def residual_ratio(A, R, prec):
    """max over the upper triangle of |A - R^T R| / bound (module docstring); an entry whose bound is zero must have a zero residual"""
    n = A.shape[0]
    R = np.triu(np.asarray(R, dtype=np.float64))
    res = np.abs(np.asarray(A, dtype=np.float64) - R.T @ R)
    bound = _gamma(n + 3, UNIT_ROUNDOFF[prec]) * (np.abs(R).T @ np.abs(R))
    if prec == "f64":
        bound *= 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, res / bound, np.where(res > 0, np.inf, 0.0))
    return float(ratio[np.triu_indices(n)].max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# family F
# ---------------------------------------------------------------------------------------------------------------------------------------
def f_ids():
    return [(n, pos, kind) for n, ps in F_POSITIONS.items() for pos in ps for kind in F_KINDS]


def family_f(n, pos, kind):
    """-> (A symmetric float64 with pivot pos - 1 spoiled, the U that rows 0 .. pos - 2 of the factor must equal, tol_E)"""
    e = family_e(n)
    k = pos - 1
    A, U = e.A.copy(), e.U.copy()
    if kind == "neg":
        A[k, k] -= U[k, k] ** 2 + 1.0
    elif kind == "nan":
        A[k, k] = np.nan
    else:
        assert kind == "zero"
        A[k, :] = 0.0
        A[:, k] = 0.0
        U[:, k] = 0.0
    return A, U, e.tol


# ---------------------------------------------------------------------------------------------------------------------------------------
# a plain Cholesky in the working precision
# ---------------------------------------------------------------------------------------------------------------------------------------
def potrf_plain(A, prec):
    """right-looking A = R^T R from the upper triangle of A, every operation in the precision under test, division and square root as NumPy
    has them -> (R upper triangular, LAPACK's info).  On a pivot that is not > 0 the rows above it are final and the pivot entry holds
    its updated value."""
    T = NPDT[prec]
    R = np.triu(np.asarray(A)).astype(T)
    n = R.shape[0]
    info = 0
    for k in range(n):
        d = R[k, k]
        if not d > 0:
            info = k + 1
            break
        r = np.sqrt(d)
        R[k, k] = r
        if k + 1 < n:
            row = R[k, k + 1:] / r
            R[k, k + 1:] = row
            R[k + 1:, k + 1:] -= np.outer(row, row)
    assert R.dtype == T
    return np.triu(R), info
