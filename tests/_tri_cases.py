"""Cases of test_gpu_tri.py, their input builders, the float64 references and a plain-Python replay of the host-side route decisions of
tri.hip (rlhip::trsm_right_upper, trsm_oop_fused, trsm_right_upper_oop, trsm_right_upper_oop_range, tf_launch and the two trmm forms).
tests/test_tri_cases.py checks the tables, the conditions and the references on the CPU.

Routes and their counters (2, 3, 4 through rlhip_path_count; 67 .. 73 through rlhip_tri_path_count; all counted on the host where the
launch is enqueued).  One letter per 256-column block makes a case's signature:

  F  fused     a run of full, well-conditioned 256-blocks in ONE trsm_fused_kernel launch: m >= TF_MIN_ROWS, n >= BW, try_blk,
               tf_offsets_fit(ldb, m); everything left of the run comes in through one GEMM and the run starts at K0blk = Jb          2 per run
               "+12": the launch took the twelve-wavefront instantiation (fp32, in place, when its rounds cost less)               69 beside 2
  K  blk       the block on trsm_blk_kernel<T, 1> (try_blk: m >= 16 and n >= 128 and nblk <= TF_MAX_BLOCKS; the block passed the guard)      67
  Q  blk, two row tiles: the same with m >= 65536, trsm_blk_kernel<T, 2>                                                               68
  S  substitution: pack_upper_rows_kernel + trsm_diag_kernel per 32-column sub-block (refused blocks, and every block without try_blk)  3 per sub-block
  out of place (rlhip_trsm_gather_*, rlhip_trsm_gather_range_*): one fused launch over all blocks when m >= TF_MIN_ROWS, n a multiple
               of BW, nblk <= TF_MAX_BLOCKS, tf_offsets_fit(ldb, m) and no block is refused                                           4
               without a pivot vector (whole solve only, tf_offsets_fit(ldsrc, m)): the identity twin, OOP = 2                   70 beside 4
               otherwise trsm_gather copies the columns and runs the in-place solver                                             71 + in place
  trmm         side Right 72, side Left 73 (copy_triu_kernel + lacpy + one GEMM)

The guard.  trsm_blk_pack_kernel refuses a 256-block when !(kappa_F^2 <= 1e6) for one of its 32 x 32 diagonal sub-blocks (unit diagonal
substituted for Diag::Unit; a ragged sub-block is padded with the identity).  guard_verdicts() evaluates that in float64 from the input.
Every listed case keeps its good sub-blocks at kappa_F^2 <= 1e5 and its bad ones at >= 1e8 (checked on the CPU): a tenfold margin on
either side of the device's limit, so the fp32 evaluation on the device cannot flip a verdict.
The 32-bit offset gate tf_offsets_fit (4 ld + m < 2^28) would need a parent above 60 GB to cross on the device; it is exercised in
the replay's CPU test only.

Family E (exact; one definition for both precisions).  U = D Uhat, D = diag(d).  Uhat: two entries from {-1, 1} per column strictly
above the 32 x 32 diagonal blocks; a diagonal block is I + N with entries of N from {-1, 0, 1} in its rows 0 .. 15 and columns 16 .. 31
only, so that N^2 = 0 and the inverse is I - N exactly.  d = 1 except in the chosen sub-block of a block marked bad, where
d = 2^-arange(32) (kappa_F^2 > 1e12); a bad block narrower than 32 columns has only its ragged sub-block of w columns, graded
d = 2^-(12 + arange(w)): the device pads it with the identity, so one column holding 2^-12 gives (31 + 2^-24) (31 + 2^24) = 5.2e8.  The solution is X = X0 / d with X0 integer, 1 <= |X0| <= 3 (no zeros: the sign of a computed zero
depends on the route), the right-hand side B = X U = X0 Uhat: small integers.  alpha is -0.5 or 2.  Every product x_i u_ij is a small
integer, the reciprocal of a diagonal entry is a power of two, and the inverse route only ever meets d = 1 (T_s and T_s (I - N) are
small integers times alpha): every route, in either precision and any summation order, returns alpha X bit for bit.
The strictly lower triangle of the stored A holds NaN-payload poison, and so does the stored diagonal of a Diag::Unit case.

Family R (rounding).  Gaussian B; U = triu(randn) / sqrt(n) + 2 I, the rows of the chosen sub-block of a bad block scaled by
logspace(0, -8, 32) (logspace(-6, -8, w) where that sub-block is a ragged one of w columns); everything rounded to the precision under test; alpha = 0.75.

The bound of family R is entrywise, on R = X U - alpha B evaluated in float64 with the device's X.  u is the unit roundoff,
gamma_t = t u / (1 - t u).
  * Substitution.  x_j = fl((alpha b_j - sum_{i<j} x_i u_ij) r_j), r_j = fl(1 / u_jj).  Higham, Accuracy and Stability, Lemma 8.4: however
    the j - 1 products and c = fl(alpha b_j) are summed (GEMM prefix, narrow GEMMs, the kernel's own loop; fused or not),
    u_jj x_j (1 + th_0) = c - sum x_i u_ij (1 + th_i) with |th| <= gamma_j, one more for the reciprocal.  c itself carries the one rounding
    of alpha b_j.  Hence |x U - alpha b|_j <= gamma_(j+1) sum_{i<=j} |x_i| |u_ij| + u |alpha b_j|, the row-wise form of Theorem 8.5; the test
    uses gamma_(n+2) for every column.
  * Explicit inverses.  T_s = fl(alpha B_s - X_<s U_<s,s) obeys the same lemma without the division:
    |T_s - (alpha B_s - X_<s U_<s,s)| <= gamma_n (|T_s| + |X_<s| |U_<s,s|) + u |alpha B_s|.  Then X_s = fl(T_s Dh_s) with the computed inverse
    Dh_s (columns by back substitution: |U_ss Dh_s - I| <= gamma_32 |U_ss| |Dh_s|, hence to first order
    |Dh_s U_ss - I| <= gamma_32 |D_s| |U_ss| |D_s| |U_ss|), so X_s U_ss - T_s = T_s (Dh_s U_ss - I) + E U_ss with |E| <= gamma_32 |T_s| |D_s|.
    With |T_s| <= (1 + gamma) (|X_s| |U_ss|) the columns of sub-block s add
        gamma_66 ((|X_s| |U_ss|) (|D_s| |U_ss| + |D_s| |U_ss| |D_s| |U_ss|))
    (66 = 2 * 32 + 2 absorbs the second-order terms), with D_s the float64 inverse of the sub-block.
  * For fp64 data the float64 evaluation of R obeys the same bound, so the bound is doubled (as test_gpu_lu.py does).
There is no other factor.

trmm inputs are small integers with alpha = -0.5: the result is exactly the float64 product (compared after adding +0.0 to both sides:
an exact zero has no defined sign)."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

NPDT = {"f64": np.float64, "f32": np.float32}
UINT = {"f64": np.uint64, "f32": np.uint32}
POISON = {"f64": 0x7FF80000DEADBEEF, "f32": 0x7FC0BEEF}
UNIT_ROUNDOFF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
PRECS = ("f64", "f32")

SB = 32
BW = 256
TF_MIN_ROWS = 16384
TF_MAX_BLOCKS = 32
KAPPA2_LIMIT = 1.0e6
KAPPA2_GOOD, KAPPA2_BAD = 1.0e5, 1.0e8
FUSED, SUBST, OOP, BLK1, BLK2, TWELVE, IDENT, GATHER, TRMM_R, TRMM_L = 2, 3, 4, 67, 68, 69, 70, 71, 72, 73
COUNTERS = (FUSED, SUBST, OOP, BLK1, BLK2, TWELVE, IDENT, GATHER, TRMM_R, TRMM_L)
NUM_CU = 256

PAD_B, PAD_A, PAD_SRC, OFF = 7, 5, 9, 3


def _cdiv(a, b):
    return -(-a // b)


def off_of(pad):
    return OFF if pad else 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# replay of the host-side decisions
# ---------------------------------------------------------------------------------------------------------------------------------------
def try_blk(m, n):
    return m >= 16 and n >= 128 and _cdiv(n, BW) <= TF_MAX_BLOCKS


def tf_offsets_fit(ld, m):
    return 4 * ld + m < 2 ** 28


def twelve_wavefronts(prec, m, num_cu=NUM_CU):
    """tf_launch: the fp32 in-place launch takes twelve wavefronts per workgroup when its rounds cost less"""
    if prec != "f32":
        return False
    ncu = num_cu if num_cu > 0 else 256

    def cost(nw):
        return _cdiv(_cdiv(m, 16 * nw), ncu) * nw

    return cost(12) < cost(8)


@dataclass
class Replay:
    rc: int
    counts: dict                 # counter -> increment (only the ones that move)
    blocks: str                  # one letter per 256-block of the in-place solve ('' when none ran)
    twelve: bool = False

    @property
    def sig(self):
        return self.blocks + ("+12" if self.twelve else "")


def _trim(counts):
    return {w: c for w, c in counts.items() if c}


def trsm_replay(prec, m, n, ldb, bad, num_cu=NUM_CU):
    """rlhip::trsm_right_upper.  bad: the guard's verdict per 256-block (guard_verdicts), read only where the device reads it."""
    counts = {w: 0 for w in COUNTERS}
    if m == 0 or n == 0:
        return Replay(0, {}, "")
    nblk = _cdiv(n, BW)
    tb = try_blk(m, n)
    badh = [bool(b) for b in bad] if tb else [True] * nblk
    assert len(badh) == nblk
    use_fused = tb and m >= TF_MIN_ROWS and n >= BW and tf_offsets_fit(ldb, m)
    have_uneg = use_fused and any(not badh[b] for b in range(n // BW))          # (a ragged last block stays on the blk path)
    blocks, twelve = "", False
    j0 = 0
    while j0 < n:
        nb, b = min(BW, n - j0), j0 // BW
        if have_uneg and not badh[b] and j0 + BW <= n:
            Je = b
            while Je < nblk and not badh[Je] and (Je + 1) * BW <= n:
                Je += 1
            counts[FUSED] += 1
            if twelve_wavefronts(prec, m, num_cu):
                counts[TWELVE] += 1
                twelve = True
            blocks += "F" * (Je - b)
            j0 = Je * BW
            continue
        if tb and not badh[b]:
            counts[BLK2 if m >= 65536 else BLK1] += 1
            blocks += "Q" if m >= 65536 else "K"
        else:
            counts[SUBST] += _cdiv(nb, SB)
            blocks += "S"
        j0 += BW
    return Replay(0, _trim(counts), blocks, twelve)


def _oop_fused_taken(m, n, ldb, bad):
    """trsm_oop_fused: the sizes it serves and the verdict of every block (n = col1)"""
    nblk = _cdiv(n, BW)
    if m < TF_MIN_ROWS or n < BW or n % BW != 0 or nblk > TF_MAX_BLOCKS or not tf_offsets_fit(ldb, m):
        return False
    return not any(bad[:nblk])


def gather_replay(prec, m, n, ldb, ldsrc, bad, has_perm, aliased=False, num_cu=NUM_CU):
    """rlhip::trsm_right_upper_oop with a valid pivot vector (or none)"""
    if m == 0 or n == 0:
        return Replay(0, {}, "")
    if aliased:
        return Replay(-14, {}, "") if has_perm else trsm_replay(prec, m, n, ldb, bad, num_cu)
    if _oop_fused_taken(m, n, ldb, bad):
        counts = {OOP: 1}
        if not has_perm and tf_offsets_fit(ldsrc, m):
            counts[IDENT] = 1
        return Replay(0, counts, "")
    r = trsm_replay(prec, m, n, ldb, bad, num_cu)
    r.counts[GATHER] = 1
    return r


def range_replay(m, nsrc, ldb, bad, col0, col1, aliased=False):
    """rlhip::trsm_right_upper_oop_range (the identity twin is never taken: may_ident = false)"""
    if col0 < 0 or col1 <= col0 or col0 % BW or col1 % BW or nsrc < col1:
        return Replay(-7, {}, "")
    if m == 0:
        return Replay(0, {}, "")
    if aliased:
        return Replay(-14, {}, "")
    if _oop_fused_taken(m, col1, ldb, bad):
        return Replay(0, {OOP: 1}, "")
    return Replay(1, {}, "")


def trmm_replay(side, m, n):
    if m == 0 or n == 0:
        return {}
    return {TRMM_R if side == "R" else TRMM_L: 1}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the guard in float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def sub_block_kappa2(U, unit=False):
    """kappa_F^2 of every 32 x 32 diagonal sub-block of the upper triangle U in float64; a ragged last one is padded with the identity, as
    the device pads it; inf where the sub-block holds a NaN or an inf"""
    n = U.shape[0]
    out = []
    for s0 in range(0, n, SB):
        w = min(SB, n - s0)
        P = np.eye(SB)
        P[:w, :w] = np.triu(np.asarray(U[s0:s0 + w, s0:s0 + w], dtype=np.float64))
        if unit:
            P[np.arange(w), np.arange(w)] = 1.0
        if not np.isfinite(P).all():
            out.append(np.inf)
            continue
        Pi = np.linalg.inv(P)
        out.append(float((P ** 2).sum() * (Pi ** 2).sum()))
    return np.array(out)


def guard_verdicts(U, unit=False):
    """per 256-block: refused when any of its sub-blocks is"""
    k2 = sub_block_kappa2(U, unit)
    return tuple(bool(np.any(~(k2[b:b + BW // SB] <= KAPPA2_LIMIT))) for b in range(0, len(k2), BW // SB))


# ---------------------------------------------------------------------------------------------------------------------------------------
# in-place trsm cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TrsmCase:
    name: str
    m: int
    n: int
    sig: str                     # the signature the case is listed under (Replay.sig at 256 compute units)
    verdicts: str = ""           # one letter per 256-block, G or B; '' = all G
    fams: tuple = ("E",)
    precs: tuple = PRECS
    unit: bool = False
    alpha_e: float = -0.5
    needs_cu: int = 0            # the route depends on the number of compute units: skipped elsewhere

    @property
    def nblk(self):
        return _cdiv(self.n, BW)

    @property
    def bad(self):
        v = self.verdicts or "G" * self.nblk
        assert len(v) == self.nblk
        return tuple(ch == "B" for ch in v)

    @property
    def fused(self):
        return "F" in self.sig


def bad_sub_block(b, width):
    """the sub-block of bad block b (width columns) that carries the grading: a full one, away from the block's edges where there is room;
    the ragged one where the block has no full sub-block"""
    full = width // SB
    return (3 + 2 * b) % full if full else 0


TRSM = [
    TrsmCase("tiny-1x1", 1, 1, "S"),
    TrsmCase("tiny-7x5", 7, 5, "S", alpha_e=2.0),
    TrsmCase("gate-m15", 15, 128, "S"),
    TrsmCase("gate-n127", 300, 127, "S", alpha_e=2.0),
    TrsmCase("ragged-sub", 257, 33, "S", fams=("E", "R")),
    TrsmCase("blk-16", 16, 128, "K"),
    TrsmCase("blk-ragged", 333, 300, "KK", fams=("E", "R"), alpha_e=2.0),
    TrsmCase("blk-wave-GG", 513, 257, "KK"),
    TrsmCase("blk-wave-GB", 513, 257, "KS", "GB"),                            # the one-column ragged block refused (graded from 2^-12)
    TrsmCase("blk-wave-BG", 513, 257, "SK", "BG", alpha_e=2.0),
    TrsmCase("blk-wave-GB-34", 513, 290, "KS", "GB", alpha_e=2.0),            # a refused ragged block with one full sub-block and a ragged one
    TrsmCase("blk-GBG", 1000, 768, "KSK", "GBG", fams=("E", "R")),
    TrsmCase("all-refused", 400, 512, "SS", "BB", alpha_e=2.0),
    TrsmCase("block-count-gate", 40, 8224, "S" * 33),
    TrsmCase("fused-smallest", 16384, 256, "F", alpha_e=2.0),
    TrsmCase("fused-ragged-rows", 16421, 512, "FF", fams=("E", "R")),
    TrsmCase("fused-GGG", 16421, 768, "FFF", "GGG", alpha_e=2.0),
    TrsmCase("fused-BGG", 16421, 768, "SFF", "BGG"),
    TrsmCase("fused-GBG", 16421, 768, "FSF", "GBG", fams=("E", "R")),
    TrsmCase("fused-GGB", 16421, 768, "FFS", "GGB", alpha_e=2.0),
    TrsmCase("fused-then-ragged", 16421, 582, "FFK"),
    TrsmCase("two-tiles", 65557, 160, "Q", fams=("E", "R"), alpha_e=2.0),     # (family R: the residual on residual_rows() only;
    TrsmCase("fused-then-two-tiles", 65557, 288, "FQ", fams=("E", "R")),      #  family E is exact on every row)
    TrsmCase("twelve-waves", 32805, 256, "F+12", precs=("f32",), needs_cu=256),
    TrsmCase("twelve-waves-full-round", 49152, 256, "F+12", precs=("f32",), alpha_e=2.0, needs_cu=256),
    TrsmCase("unit-subst", 257, 33, "S", unit=True),
    TrsmCase("unit-blk", 333, 300, "KK", unit=True, alpha_e=2.0),
    TrsmCase("unit-fused", 16421, 512, "FF", unit=True),
]
XASM_CASES = ("fused-smallest", "fused-GBG")
NAN_CASE = TrsmCase("nan", 64, 256, "S", "B", fams=("R",))
NAN_AT = (37, 45)                                                             # strictly upper, inside diagonal sub-block 1
ALPHA_R = 0.75


def trsm_case(name):
    return next(c for c in TRSM + [NAN_CASE] if c.name == name)


def trsm_ids():
    return [(c, fam, prec) for c in TRSM for fam in c.fams for prec in c.precs]


def id_of(t):
    c, fam, prec = t
    return f"{c.name}-{fam}-{prec}"


def _seed(name):
    return zlib.crc32(name.encode())


RAGGED_GRADING_START = 12


def _grading(bad, n):
    """the graded sub-blocks: list of (first row, width w).  w = 32 except in a bad block narrower than 32 columns, whose only sub-block
    is ragged.  The device pads that one with the identity before it takes the norms, so for a 1 x 1 block holding u it sees
    kappa_F^2 = (31 + u^2) (31 + 1 / u^2): the grading of a ragged sub-block therefore starts at 2^-12 (5.2e8 for one column)."""
    out = []
    for b, isbad in enumerate(bad):
        if isbad:
            width = min(BW, n - b * BW)
            r0 = b * BW + SB * bad_sub_block(b, width)
            out.append((r0, min(SB, n - r0)))
    return out


def grading_exponents(w):
    """family E: log2 of 1 / d over a graded sub-block of w columns"""
    return np.arange(SB) if w == SB else RAGGED_GRADING_START + np.arange(w)


def grading_scale(w):
    """family R: the row scaling of a graded sub-block of w columns"""
    return np.logspace(0, -8, SB) if w == SB else np.logspace(-6, -8, w)


@functools.lru_cache(maxsize=2)
def _family_e_master(m, n, bad, seed):
    """-> (Uhat int8 n x n with unit diagonal, log2 of 1 / d per row, X0 int8 m x n)"""
    rng = np.random.default_rng(seed)
    Uhat = np.zeros((n, n), dtype=np.int8)
    for j in range(SB, n):
        top = (j // SB) * SB
        Uhat[rng.integers(0, top, 2), j] = rng.choice(np.array([-1, 1], dtype=np.int8), 2)
    for s0 in range(0, n, SB):
        w = min(SB, n - s0)
        if w > 16:
            Uhat[s0:s0 + 16, s0 + 16:s0 + w] = rng.integers(-1, 2, (16, w - 16), dtype=np.int8)
    Uhat[np.arange(n), np.arange(n)] = 1
    e = np.zeros(n, dtype=np.int64)
    for r0, w in _grading(bad, n):
        e[r0:r0 + w] = grading_exponents(w)
    X0 = rng.choice(np.array([-3, -2, -1, 1, 2, 3], dtype=np.int8), (m, n))
    return Uhat, e, X0


@dataclass
class TrsmInput:
    U: np.ndarray                # the triangle the solve means: upper, zero below, the diagonal as used (ones for Diag::Unit)
    A: np.ndarray                # what is stored: poison strictly below the diagonal (and on it for Diag::Unit)
    B: np.ndarray
    alpha: float
    expect: np.ndarray           # family E: alpha X, exact; family R: the float64 solution (for orientation, never asserted bitwise)
    bad: tuple


def poison_lower(U, prec, unit):
    A = np.array(U, dtype=NPDT[prec], order="C")
    n = A.shape[0]
    mask = np.tri(n, k=0 if unit else -1, dtype=bool)
    A.view(UINT[prec])[mask] = POISON[prec]
    return A


def family_e(m, n, bad, prec, unit, alpha, seed):
    T = NPDT[prec]
    Uhat, e, X0 = _family_e_master(m, n, tuple(bad), seed)
    assert not (unit and any(bad)), "a unit diagonal cannot be graded"
    d = np.ldexp(T(1), -e).astype(T)
    U = Uhat.astype(T) * d[:, None]
    B = X0.astype(T) @ Uhat.astype(T)                                         # = X U: the grading cancels
    X = X0.astype(T) * np.ldexp(T(1), e).astype(T)[None, :]
    return TrsmInput(U, poison_lower(U, prec, unit), B, alpha, (T(alpha) * X).astype(T), tuple(bad))


def family_r_triangle(n, bad, prec, seed):
    rng = np.random.default_rng(seed + 1)
    U = np.triu(rng.standard_normal((n, n))) / np.sqrt(n) + 2.0 * np.eye(n)
    for r0, w in _grading(bad, n):
        U[r0:r0 + w] *= grading_scale(w)[:, None]
    return U.astype(NPDT[prec])


def solve_reference(U, B, alpha):
    """X = alpha B inv(U) by column substitution in float64"""
    U = np.asarray(U, dtype=np.float64)
    X = alpha * np.asarray(B, dtype=np.float64)
    for j in range(U.shape[0]):
        X[:, j] = (X[:, j] - X[:, :j] @ U[:j, j]) / U[j, j]
    return X


def family_r(m, n, bad, prec, unit, seed, nan_at=None):
    rng = np.random.default_rng(seed + 2)
    U = family_r_triangle(n, bad, prec, seed)
    if unit:
        U[np.arange(n), np.arange(n)] = 1
    if nan_at is not None:
        U[nan_at] = np.nan
    B = rng.standard_normal((m, n)).astype(NPDT[prec])
    with np.errstate(invalid="ignore"):
        X = solve_reference(U, B, ALPHA_R)
    return TrsmInput(U, poison_lower(U, prec, unit), B, ALPHA_R, X, tuple(bad))


def trsm_input(case, fam, prec):
    if fam == "E":
        return family_e(case.m, case.n, case.bad, prec, case.unit, case.alpha_e, _seed(case.name))
    if case is NAN_CASE:                                                      # no grading: the NaN alone must raise the block's flag
        inp = family_r(case.m, case.n, (False,) * case.nblk, prec, case.unit, _seed(case.name), NAN_AT)
        inp.bad = case.bad
        return inp
    return family_r(case.m, case.n, case.bad, prec, case.unit, _seed(case.name))


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulation in the working precision, and the bound
# ---------------------------------------------------------------------------------------------------------------------------------------
def inverse_by_columns(P):
    """trsm_blk_pack_kernel: column j of the inverse of the upper triangle P by back substitution, in P's precision"""
    T = P.dtype.type
    w = P.shape[0]
    D = np.zeros_like(P)
    for j in range(w):
        for i in range(j, -1, -1):
            acc = T(1) if i == j else T(0)
            for l in range(i + 1, j + 1):
                acc = T(acc - P[i, l] * D[l, j])
            D[i, j] = T(acc / P[i, i])
    return D


def emulate_trsm(U, B, alpha, prec, inverse_blocks):
    """The algorithm of tri.hip in the working precision: per 32-column sub-block T_s = alpha B_s - X_<s U_<s,s, then column substitution
    with the reciprocal of the diagonal, or -- in the 256-blocks named by inverse_blocks -- X_s = T_s Dh_s with the inverse by columns."""
    T = NPDT[prec]
    U = np.asarray(U, dtype=T)
    X = np.array(B, dtype=T)
    n = U.shape[0]
    a = T(alpha)
    for s0 in range(0, n, SB):
        s1 = min(s0 + SB, n)
        t = (a * X[:, s0:s1]).astype(T)
        if s0:
            t = (t - X[:, :s0] @ U[:s0, s0:s1]).astype(T)
        if inverse_blocks[s0 // BW]:
            X[:, s0:s1] = t @ inverse_by_columns(U[s0:s1, s0:s1])
            continue
        for j in range(s0, s1):
            x = t[:, j - s0]
            for i in range(s0, j):
                x = (x - X[:, i] * U[i, j]).astype(T)
            X[:, j] = x * T(T(1) / U[j, j])
    return X


def routes_of(case):
    """one letter per 256-block: the signature without its suffix"""
    return case.sig.split("+")[0]


def inverse_blocks_of(case):
    """which 256-blocks go through explicit inverses on the device: the F, K and Q letters of the signature"""
    return tuple(ch in "FKQ" for ch in routes_of(case))


def residual_rows(m):
    """the rows family R's residual is evaluated on: all of them below 65536 rows; beyond, the first 512, the last 512 and 2048 random ones"""
    if m < 65536:
        return np.arange(m)
    return np.unique(np.r_[0:512, m - 512:m, np.random.default_rng(m).integers(512, m - 512, 2048)])


def _gamma(t, u):
    return t * u / (1.0 - t * u)


def residual_ratio(U, B, alpha, X, prec, routes):
    """max over the entries of |X U - alpha B| / bound (module docstring) per route: routes holds one letter per 256-block (S, K, Q, F:
    the signature), the result one entry per letter present.  F, K and Q columns carry the term of the explicit inverses.
    An entry whose bound is zero must have a zero residual (-> inf otherwise)."""
    u = UNIT_ROUNDOFF[prec]
    U = np.asarray(U, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    aB = np.abs(alpha * np.asarray(B, dtype=np.float64))
    n = U.shape[0]
    R = np.abs(X @ U - alpha * np.asarray(B, dtype=np.float64))
    bound = _gamma(n + 2, u) * (np.abs(X) @ np.abs(U)) + u * aB
    assert len(routes) == _cdiv(n, BW) and set(routes) <= set("SKQF")
    for s0 in range(0, n, SB):
        if routes[s0 // BW] == "S":
            continue
        s1 = min(s0 + SB, n)
        aU = np.abs(U[s0:s1, s0:s1])
        W = np.abs(np.linalg.inv(U[s0:s1, s0:s1])) @ aU
        bound[:, s0:s1] += _gamma(66, u) * ((np.abs(X[:, s0:s1]) @ aU) @ (W + W @ W))
    if prec == "f64":
        bound *= 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, R / bound, np.where(R > 0, np.inf, 0.0))
    letter = np.array(list(routes))[np.arange(n) // BW]
    return {ch: float(ratio[:, letter == ch].max(initial=0.0)) for ch in sorted(set(routes))}


# ---------------------------------------------------------------------------------------------------------------------------------------
# out-of-place cases (family E unless stated)
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GatherCase:
    name: str
    m: int
    n: int
    perm: bool
    counts: tuple                # the expected counter deltas, as sorted (counter, increment) pairs
    verdicts: str = ""
    nsrc: int = 0                # source columns (0: n)

    @property
    def bad(self):
        v = self.verdicts or "G" * _cdiv(self.n, BW)
        return tuple(ch == "B" for ch in v)


def _c(**kw):
    names = dict(fused=FUSED, subst=SUBST, oop=OOP, blk1=BLK1, ident=IDENT, gather=GATHER)
    return tuple(sorted((names[k], v) for k, v in kw.items()))


GATHER_CASES = [
    GatherCase("staged-pivot", 16421, 512, True, _c(oop=1)),
    GatherCase("identity-twin", 16421, 512, False, _c(oop=1, ident=1)),
    GatherCase("copy-ragged-n-perm", 16421, 582, True, _c(gather=1, fused=1, blk1=1)),
    GatherCase("copy-ragged-n", 16421, 582, False, _c(gather=1, fused=1, blk1=1)),
    GatherCase("copy-short", 900, 256, True, _c(gather=1, blk1=1)),
    GatherCase("copy-refused", 16421, 512, True, _c(gather=1, fused=1, subst=8), "GB"),
]
RANGE_M, RANGE_N, RANGE_NSRC_WIDE = 16421, 512, 600


def gather_input(m, n, bad, prec, name, perm, nsrc=0, alpha=-0.5):
    """-> (TrsmInput, Bsrc m x nsrc, 1-based pivot vector or None): column c of the right-hand side is column perm[c] - 1 of Bsrc; source
    columns no pivot names hold poison"""
    inp = family_e(m, n, bad, prec, False, alpha, _seed(name))
    nsrc = nsrc or n
    if not perm:
        assert nsrc == n
        return inp, inp.B, None
    p = np.random.default_rng(_seed(name) + 3).permutation(nsrc)[:n].astype(np.int64) + 1
    Bsrc = np.empty((m, nsrc), dtype=NPDT[prec])
    Bsrc.view(UINT[prec])[:] = POISON[prec]
    Bsrc[:, p - 1] = inp.B
    return inp, Bsrc, p


# ---------------------------------------------------------------------------------------------------------------------------------------
# trmm cases
# ---------------------------------------------------------------------------------------------------------------------------------------
TRMM_SHAPES = ((7, 7), (40, 300), (257, 33), (1000, 256))
TRMM_FORMS = (("R", "N"), ("L", "N"), ("L", "T"))
TRMM_ALPHA = -0.5


def trmm_ids():
    return [(side, trans, m, n, diag, prec) for side, trans in TRMM_FORMS for m, n in TRMM_SHAPES for diag in "NU" for prec in PRECS]


def trmm_input(side, trans, m, n, diag, prec):
    """-> (U as meant, A as stored, B, the exact result)"""
    T = NPDT[prec]
    k = n if side == "R" else m
    rng = np.random.default_rng(_seed(f"trmm-{side}{trans}{m}x{n}{diag}"))
    U = np.triu(rng.integers(-2, 3, (k, k))).astype(np.float64)
    if diag == "U":
        U[np.arange(k), np.arange(k)] = 1.0
    B = rng.integers(-3, 4, (m, n)).astype(np.float64)
    if side == "R":
        C = TRMM_ALPHA * (B @ U)
    else:
        C = TRMM_ALPHA * ((U.T if trans == "T" else U) @ B)
    assert np.abs(C).max(initial=0) < 2 ** 22
    return U.astype(T), poison_lower(U, prec, diag == "U"), B.astype(T), C.astype(T)
