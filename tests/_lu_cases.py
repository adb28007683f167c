"""Cases of test_gpu_lu.py, their input builders, the float64 references and a plain-Python replay of the host-side route decisions of
lu.hip (rlhip::getrf, rlhip::laswp, rlhip::luqrcp_piv).

Routes and their counters (rlhip_lu_path_count, counted on the host where the launch is enqueued; 7 is read through rlhip_path_count):

  a panel [j0, j0 + pb)   lds      fewer than 1024 rows on and below the diagonal: getrf_panel_kernel                            60
                          fast     rows >= 1024 and at most 64 workgroups of 256 RPT rows (RPT = 2 fp64 / 4 fp32:
                                   32768 / 65536 rows): the fast step of the type (lu_f64.hip / lu_f32.hip)                      61
                          general  more than 64 workgroups, within the resident capacity: getrf_panel_reg_kernel                62
                          column   more workgroups than the resident capacity reg_cap (and than 64): column-at-a-time launches    7
  a getrf call            outer    m >= 49152 and n >= 256: outer blocks of 128 columns (else of one panel)                      63
  right of an outer block solve    one unit_lower_solve_kernel launch per panel of an outer block wider than a panel            64
                          (an outer block of ONE panel -- `one_panel` -- folds the substitution into its interchange launch)
  luqrcp_piv              walk     min(sd, cols) <= 2048 (and cols < 2^31): luqrcp_piv_lds_kernel                                65
                          serial   otherwise: luqrcp_piv_kernel                                                                  66

reg_cap is an occupancy query at run time (workgroups of getrf_panel_reg_kernel resident at once); the replay takes it as a parameter.
Its smallest possible value is one workgroup per compute unit: REG_CAP_MIN = 256 on the MI355X.  Every case of GETRF needs fewer
workgroups than that, so its route does not depend on the query; the one column-at-a-time case is asserted through counter 7 alone.

Inputs.  Gaussian entries times logspace(0, -2, n) per column, rounded to the type under test.  Tall cases carry two duplicate-row GROUPS:
one source row is copied (some copies negated) to other positions, and its entry in one column is raised so that the group wins the pivot
search there.  Members of a group are exact duplicates up to sign, and elimination treats them alike in any arithmetic (round to nearest
is symmetric in sign), so they tie exactly in every column until the first of them is chosen -- after which the others are zero to
rounding right of that column and never compete again (the tall cases keep full column rank: m >= 2 n + 16).  Which member must win is LAPACK's first-maximum rule on CURRENT positions: group B holds row 1, which an earlier
interchange has moved away by the time the group competes.
"Alike in any arithmetic" needs one qualification, and it concerns the REFERENCE: a blocked host LAPACK updates rows with different
micro-kernels depending on where they sit (edge tiles, thread slabs), so copies that were updated by nonzero multipliers can come to
differ in the last bit there, and its choice among them is then arbitrary (seen on 4096 x 96 fp64: the member at position 4094 chosen
over the ones at 70, 326 and 2506).  A group that competes in a column c > 0 therefore holds exact zeros in the columns before c: its
multipliers are exactly zero, every update subtracts an exact zero in every arithmetic and order, and the members reach column c
bit-identical on the host as on the device.  The device's tie logic sees the same exact ties either way."""
import functools
from dataclasses import dataclass

import numpy as np

NPDT = {"f64": np.float64, "f32": np.float32}
UINT = {"f64": np.uint64, "f32": np.uint32}
UNIT_ROUNDOFF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
RPT = {"f64": 2, "f32": 4}                      # rows per thread of the register kernels (LU_RPT_BIG)
PRECS = ("f64", "f32")
PB = 32
NBO = 128
LDS, FAST, GENERAL, OUTER, SOLVE, WALK, SERIAL, COLUMN = 60, 61, 62, 63, 64, 65, 66, 7
GETRF_COUNTERS = (LDS, FAST, GENERAL, OUTER, SOLVE, COLUMN)
REG_CAP_MIN = 256                               # one resident workgroup on each of the 256 compute units
LQ_MAX = 2048


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# replay of rlhip::getrf's host-side decisions
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Replay:
    counts: dict                 # counter -> increment (only the ones that move)
    panels: list                 # (j0, pb, rows, G_reg, route name, workgroups launched) per panel
    nbo: int
    one_panel: bool              # every outer block is a single panel
    right_launches: int          # outer blocks with columns to their right

    @property
    def sig(self):
        """the routes of the panels in order, runs collapsed: 'fast>lds'"""
        out = []
        for p in self.panels:
            if not out or out[-1] != p[4]:
                out.append(p[4])
        return ">".join(out) + ("+outer" if self.nbo > PB else "")


def getrf_replay(prec, m, n, reg_cap=REG_CAP_MIN):
    counts = {w: 0 for w in GETRF_COUNTERS}
    panels = []
    mn = min(m, n)
    nbo = NBO if (m >= 49152 and n >= 256) else PB
    if mn > 0 and nbo > PB:
        counts[OUTER] += 1
    use_tag = m < 2 ** 31
    rights = 0
    for J0 in range(0, mn, nbo):
        Jend = min(J0 + nbo, mn)
        Cin = min(J0 + nbo, n)
        for j0 in range(J0, Jend, PB):
            pb = min(Jend - j0, PB)
            rows = m - j0
            G_reg = _cdiv(rows, 256 * RPT[prec])
            if G_reg > reg_cap and G_reg > 64:
                route, G, w = "column", 0, COLUMN
            elif use_tag and rows >= 1024:
                route, G, w = ("fast", G_reg, FAST) if G_reg <= 64 else ("general", G_reg, GENERAL)
            else:
                route, G, w = "lds", _cdiv(rows, 256), LDS            # rpw = max(ceil(rows / num_cu), 256) = 256 below 1024 rows
            counts[w] += 1
            panels.append((j0, pb, rows, G_reg, route, G))
        if n - Cin > 0:
            rights += 1
            if Jend - J0 > PB:                                        # not one_panel
                counts[SOLVE] += _cdiv(Jend - J0, PB)
    return Replay({w: c for w, c in counts.items() if c}, panels, nbo, nbo == PB, rights)


def luqrcp_replay(sd, cols):
    if cols <= 0:
        return {}
    return {WALK: 1} if (min(sd, cols) <= LQ_MAX and cols < 2 ** 31) else {SERIAL: 1}


# ---------------------------------------------------------------------------------------------------------------------------------------
# getrf cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GetrfCase:
    m: int
    n: int
    sig: str                     # the route the case is listed under (Replay.sig)
    precs: tuple = PRECS
    pads: tuple = (0, 7)         # lda = m + pad; pad 7 also offsets the first element 3 words into the allocation
    zero_col: int = -1           # this column is exactly zero (-0.0 in the row that reaches the diagonal)
    seed: int = 0

    @property
    def name(self):
        return f"{self.m}x{self.n}" + ("-zero" if self.zero_col >= 0 else "")

    def groups(self, prec):
        return dup_groups(self.m, self.n, prec)


def off_of(pad):
    return 3 if pad else 0


GETRF = [
    # LDS kernel only
    GetrfCase(40, 40, "lds"), GetrfCase(1, 1, "lds"), GetrfCase(2, 1, "lds"), GetrfCase(1, 5, "lds"),
    GetrfCase(257, 33, "lds"),                       # two workgroups and a ragged second panel
    GetrfCase(1023, 70, "lds"),
    GetrfCase(64, 100, "lds"), GetrfCase(300, 700, "lds"),          # wide
    # fast step
    GetrfCase(1024, 32, "fast"), GetrfCase(4096, 96, "fast"),
    GetrfCase(1025, 33, "fast>lds"),                 # (its one-column second panel has 993 rows)
    GetrfCase(32768, 40, "fast", precs=("f64",)), GetrfCase(65536, 40, "fast", precs=("f32",)),
    # fast -> LDS within one call
    GetrfCase(1040, 64, "fast>lds"),
    GetrfCase(1100, 1300, "fast>lds"),               # wide: the one_panel route right of every outer block
    # general register kernel
    GetrfCase(32769, 40, "general>fast", precs=("f64",)),           # (the second panel has 32737 rows)
    GetrfCase(65537, 40, "general>fast", precs=("f32",)),
    GetrfCase(32790, 64, "general>fast", precs=("f64",)),
    GetrfCase(65560, 64, "general>fast", precs=("f32",)),
    # outer block 128
    GetrfCase(49152, 256, "general+outer", precs=("f64",), pads=(0,)),
    GetrfCase(49152, 256, "fast+outer", precs=("f32",), pads=(0,)),
    GetrfCase(49152, 300, "general+outer", precs=("f64",), pads=(7,)),       # ragged third block of 44 columns
    GetrfCase(49152, 300, "fast+outer", precs=("f32",), pads=(7,)),
    GetrfCase(66000, 256, "general+outer", precs=("f32",), pads=(7,)),   # the general register kernel under the outer block
    # the other side of the outer-block gate
    GetrfCase(49151, 256, "general", precs=("f64",), pads=(7,)), GetrfCase(49151, 256, "fast", precs=("f32",), pads=(7,)),
    GetrfCase(49152, 255, "general", precs=("f64",), pads=(0,)), GetrfCase(49152, 255, "fast", precs=("f32",), pads=(0,)),
    # zero pivot in column 40 (second panel), one case per panel kernel
    GetrfCase(300, 64, "lds", zero_col=40),
    GetrfCase(1100, 64, "fast", zero_col=40),
    GetrfCase(32810, 64, "general", precs=("f64",), zero_col=40, pads=(7,)),
    GetrfCase(65580, 64, "general", precs=("f32",), zero_col=40, pads=(7,)),
]
# the column-at-a-time panel: the guard-row variant of test_gpu_kernels.py::test_getrf_very_tall_panels_match_lapack, fp32
COLUMN_CASE = GetrfCase(300000, 40, "column", precs=("f32",), pads=(7,))


def getrf_ids():
    return [(c, prec, pad) for c in GETRF for prec in c.precs for pad in c.pads]


def id_of(t):
    c, prec, pad = t
    return f"{c.name}-{prec}-pad{pad}"


@dataclass(frozen=True)
class DupGroup:
    col: int                     # the column whose entry is raised: the group wins the pivot search there (or earlier)
    rows: tuple                  # member rows (original indices); rows[0] is the source
    signs: tuple                 # +1 / -1 per member


def dup_groups(m, n, prec):
    """Duplicate-row groups of an m x n case: none unless the matrix is tall enough to stay of full column rank (m >= 2 n + 16).
    Group A competes in column 0, before any interchange: source row 5, copies in the same thread's next register slot (5 + 256),
    in another wave (5 + 64), in another workgroup of every register kernel (5 + 3072 + 64), and in the last row.
    Group B competes in column cB > 1 (in the second panel when there is one): row 1 -- index < n, displaced by the interchange of
    column 1 before it competes -- with copies at 70 (another wave), 70 + 256 (that thread's next slot), 70 + 4096 and the row
    before the last."""
    if m < 2 * n + 16 or n < 3:
        return ()
    out = []
    a = [5, 5 + 64, 5 + 256, 5 + 3072 + 64, m - 1]
    b = [1, 70, 70 + 256, 70 + 4096, m - 2]
    cB = 35 if n > 40 else n // 2 + 1
    used = set()
    for col, rows in ((0, a), (cB, b)):
        rows = [r for r in dict.fromkeys(rows) if 0 <= r < m and r not in used]
        used |= set(rows)
        if len(rows) >= 2:
            signs = tuple(1 if i % 3 != 1 else -1 for i in range(len(rows)))      # +, -, +, +, -
            out.append(DupGroup(col, tuple(rows), signs))
    return tuple(out)


@functools.lru_cache(maxsize=2)
def getrf_input(case, prec):
    """the m x n matrix of the case in the type under test (read-only)"""
    m, n = case.m, case.n
    rng = np.random.default_rng([case.seed, m, n, 0 if prec == "f64" else 1])
    A = (rng.standard_normal((m, n)) * np.logspace(0, -2, n)).astype(NPDT[prec])
    for g in case.groups(prec):
        A[g.rows[0], :g.col] = 0.0                                     # multipliers of exactly zero: see the module docstring
        A[g.rows[0], g.col] = 16.0 * np.logspace(0, -2, n)[g.col]      # (Gaussian maxima of 3e5 samples stay below 5.5)
        for r, s in zip(g.rows[1:], g.signs[1:]):
            A[r] = s * A[g.rows[0]]
    if case.zero_col >= 0:
        A[:, case.zero_col] = 0.0
        # the row that reaches the diagonal: the interchanges of the columns before do not depend on this column's values
        _, piv, _ = lapack_getrf(A[:, :case.zero_col], prec)
        where = positions_after(piv, m)
        A[where[case.zero_col], case.zero_col] = -0.0
    A.setflags(write=False)
    return A


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
def lapack_getrf(A, prec):
    """-> (lu, 0-based pivots, info) of scipy's {d,s}getrf"""
    import scipy.linalg.lapack as ll

    if A.shape[1] == 0:
        return A.copy(), np.zeros(0, dtype=np.int64), 0
    lu, piv, info = (ll.dgetrf if prec == "f64" else ll.sgetrf)(np.asfortranarray(A))
    return lu, piv.astype(np.int64), int(info)


def positions_after(piv0, m, upto=None):
    """where[p] = the original row that sits at position p after the interchanges piv0[:upto] (0-based)"""
    where = np.arange(m)
    for j, p in enumerate(piv0[:upto]):
        where[j], where[p] = where[p], where[j]
    return where


def first_maximum_violations(m, piv0, groups):
    """Check 2, no LAPACK involved: walk the interchanges, tracking which original row sits where.  When the row chosen in column j belongs
    to a duplicate group, no position in [j, chosen) may hold a member of that group that was not chosen before: it ties with the chosen row
    exactly, and the first maximum is the one at the smallest CURRENT position.  (That the chosen row is a maximum at all is check 4,
    |L| <= 1.)  -> list of (column, chosen position, earlier position, its original row)"""
    where = np.arange(m)
    at = {r: r for g in groups for r in g.rows}                       # original row -> current position
    group_of = {r: g for g in groups for r in g.rows}
    picked = set()
    bad = []
    for j, p in enumerate(piv0):
        p = int(p)
        chosen = int(where[p])
        g = group_of.get(chosen)
        if g is not None:
            for r in g.rows:
                if r != chosen and r not in picked and j <= at[r] < p:
                    bad.append((j, p, at[r], r))
            picked.add(chosen)
        a, b = int(where[j]), chosen
        where[j], where[p] = b, a
        if a in at:
            at[a] = p
        if b in at:
            at[b] = j
    return bad


def split_lu(LU):
    m, n = LU.shape
    k = min(m, n)
    L = np.tril(LU[:, :k].astype(np.float64), -1)
    L[np.arange(k), np.arange(k)] = 1.0
    U = np.triu(LU[:k].astype(np.float64))
    return L, U


def backward_ratio(A, LU, piv0, prec):
    """Check 3 (Higham, Accuracy and Stability, Theorem 9.3): max over the entries of |P A - L U| / (gamma_(k+2) (|L| |U|)), k = min(i, j) + 1,
    gamma_t = t u / (1 - t u); +2 for the multiply by the reciprocal of the pivot.  Evaluated in float64; for float64 data the evaluation
    obeys the same bound, so the bound is doubled.  An entry whose bound is zero must have a zero residual (-> inf otherwise)."""
    m, n = A.shape
    u = UNIT_ROUNDOFF[prec]
    L, U = split_lu(LU)
    PA = A[positions_after(piv0, m)].astype(np.float64)
    R = np.abs(PA - L @ U)
    t = (np.minimum.outer(np.arange(m), np.arange(n)) + 3).astype(np.float64)
    bound = t * u / (1.0 - t * u) * (np.abs(L) @ np.abs(U)) * (2.0 if prec == "f64" else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, R / bound, np.where(R > 0, np.inf, 0.0))
    return float(ratio.max(initial=0.0)), float(np.abs(L).max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# laswp cases
# ---------------------------------------------------------------------------------------------------------------------------------------
LASWP_ROWS = 140                                                           # rows of the matrix: 100 interchanges, far rows up to 139
LASWP_PAD = 3
LASWP_NS = (1, 3, 4, 5, 1000, 70000)                                       # (the grid is capped at 16384 workgroups of 4 columns)
LASWP_RANGES = ((1, 1), (1, 32), (1, 33), (5, 37), (33, 64), (1, 100), (3, 2))
LASWP_PATTERNS = ("identity", "rotate", "same_far", "distinct_far", "far_again", "random")


def laswp_ipiv(pattern, k1, k2):
    """1-based pivots for rows 1 .. 100 (entries outside [k1, k2] hold 1-based garbage-free identities); ipiv[i] >= i + 1 as in an LU"""
    K = 100
    ip = np.arange(1, K + 1, dtype=np.int64)
    lo, hi = k1 - 1, max(k2, k1 - 1)
    idx = np.arange(lo, hi)
    if pattern == "identity" or len(idx) == 0:
        return ip
    if pattern == "rotate":
        ip[idx] = idx + 2 + 1                                              # ipiv[i] = i + 2 (0-based): a rotation inside the panel
    elif pattern == "same_far":
        ip[idx] = 120 + 1                                                  # one far row for every interchange
    elif pattern == "distinct_far":
        ip[idx] = 101 + (idx - lo) % 32 + (idx - lo) // 32 + 1             # 32 distinct far rows per panel of 32: 64 rows move
    elif pattern == "far_again":
        ip[idx] = np.where((idx - lo) % 3 == 0, 130, np.where((idx - lo) % 3 == 1, idx, 131)) + 1      # far row, none, another far row
    elif pattern == "random":
        rng = np.random.default_rng([k1, k2])
        ip[idx] = np.array([rng.integers(i, LASWP_ROWS) for i in idx]) + 1
    assert ip.max() <= LASWP_ROWS and np.all(ip >= np.arange(1, K + 1))
    return ip


def laswp_matrix(n, prec):
    """rows x n, distinct integers (below 2^24: exact in fp32)"""
    M = (np.arange(LASWP_ROWS)[:, None] + LASWP_ROWS * np.arange(n)[None, :] + 1).astype(NPDT[prec])
    assert M.max() < 2 ** 24
    return M


def laswp_reference(M, k1, k2, ipiv):
    """lapack::laswp with incx = 1 as a serial loop"""
    M = M.copy()
    for i in range(k1 - 1, k2):
        p = int(ipiv[i]) - 1
        if p != i:
            M[[i, p]] = M[[p, i]]
    return M


# ---------------------------------------------------------------------------------------------------------------------------------------
# luqrcp_piv cases
# ---------------------------------------------------------------------------------------------------------------------------------------
LUQRCP_SHAPES = ((2048, 2048), (2049, 2049), (2049, 5000), (5000, 3000), (0, 7), (3, 1))
LUQRCP_ROUTE = {(2048, 2048): "walk", (2049, 2049): "serial", (2049, 5000): "serial", (5000, 3000): "serial", (0, 7): "walk", (3, 1): "walk"}


def lq_hash(a):
    """the hash of luqrcp_piv_lds_kernel: ((uint32) a * 2654435761) >> 20, 12 bits"""
    return ((np.asarray(a, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)


def luqrcp_random_ipiv(sd, cols, seed=3):
    rng = np.random.default_rng([seed, sd, cols])
    lim = min(sd, cols)
    ip = np.array([rng.integers(i, cols) if rng.random() < 0.8 else i for i in range(lim)], dtype=np.int64) + 1
    out = np.arange(1, max(sd, 1) + 1, dtype=np.int64)                     # (entries beyond lim are never read)
    out[:lim] = ip
    return out


ADV_COLS = 400000


def _far_with_hash(h, count, cols=ADV_COLS):
    a = np.arange(LQ_MAX, cols)
    hit = a[lq_hash(a) == h]
    assert len(hit) >= count
    return hit[:count]


def luqrcp_adversarial(kind):
    """-> (sd, cols, 1-based ipiv).  'chain': 48 far positions of one hash value, chosen in order and then all again, so that the second
    visit finds its key up to 47 probes deep; 'wrap': four positions hashing to 4094, four to 4095, three to 0, chosen twice: the probe
    runs past slot 4095 into slots 0 .. and finds other keys there."""
    sd = LQ_MAX
    ip = np.arange(1, sd + 1, dtype=np.int64)
    if kind == "chain":
        far = _far_with_hash(1234, 48)
    else:
        far = np.concatenate([_far_with_hash(4094, 4), _far_with_hash(4095, 4), _far_with_hash(0, 3)])
    seq = np.concatenate([far, far, far[::-1]])
    ip[10:10 + len(seq)] = seq + 1
    return sd, ADV_COLS, ip


def luqrcp_reference(sd, cols, ipiv):
    J = np.arange(1, cols + 1, dtype=np.int64)
    for i in range(min(sd, cols)):
        a = int(ipiv[i]) - 1
        J[a], J[i] = J[i], J[a]
    return J


def lds_walk_probes(sd, cols, ipiv):
    """a model of the open-addressing table of luqrcp_piv_lds_kernel (4096 slots, linear probing): -> (longest probe sequence, number of
    probe steps that went from slot 4095 to slot 0, number of lookups that found their key behind at least 40 others)"""
    lim = min(sd, cols)
    key = [-1] * (2 * LQ_MAX)
    longest = wraps = deep = 0
    for i in range(lim):
        a = int(ipiv[i]) - 1
        if a < lim:
            continue
        h = int(lq_hash(a))
        steps = 0
        while key[h] != -1 and key[h] != a:
            if h == 2 * LQ_MAX - 1:
                wraps += 1
            h = (h + 1) & (2 * LQ_MAX - 1)
            steps += 1
        if key[h] == a and steps >= 40:
            deep += 1
        key[h] = a
        longest = max(longest, steps)
    return longest, wraps, deep
