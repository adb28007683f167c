"""The column-pivoted Householder QR kernels (csrc/qrcp.hip) behind rlhip_geqp3_*, rlhip_geqp3_steps_* and rlhip_qrp_partial_*, called
through the C ABI in fp64 AND fp32 and compared with float64 references on the same (upcast) values:

  geqp3          scipy's dgeqp3 / sgeqp3: J exactly, R and tau (signs included) to a multiple of eps, A P = Q R to backward error
  geqp3_steps    _laqp2 below, a numpy restatement of LAPACK's dlaqp2 (the algorithm the kernels follow step by step), stopped after
  qrp_partial    `steps` columns; qrp_partial with HQRRP's (1 + t)(1 - t) norm down-date

Two persistent kernels sit behind the three entry points: the tag-exchange kernel (columns in LDS) and the rendezvous kernel (columns in
LDS, or in the matrix with the reflector staged in LDS, or read from its published slot).  No path counter tells them apart, so _route()
restates qr_core's choice and every case names its route in its id; the test asserts that the device really takes that route.

Cases per route and precision: well-separated norms, exact ties (first maximum by current position), zero matrix / zero columns / a
column that becomes exactly zero, a +0.0 / -0.0 pivot entry, the sqrt(eps / 2) norm-recomputation safeguard, rank deficiency, lda > m
with guard rows, garbage jpvt / tau on entry, the argument codes, and the exponent range (A 2^e: J and tau bitwise those of A, R
bitwise 2^e R).  The CPU test at the end checks _laqp2 itself against dgeqp3."""
import numpy as np
import pytest
import scipy.linalg.lapack as ll

gpu = pytest.mark.gpu
PRECS = ["f64", "f32"]
EPS = {"f64": np.finfo(np.float64).eps, "f32": np.finfo(np.float32).eps}
NP = {"f64": np.float64, "f32": np.float32}
SENT = 7.25                                        # guard value of rows a call must not touch
GARBAGE_J, GARBAGE_TAU = -987654321, -3.5          # jpvt / tau contents on entry: must be ignored


def _tol3z(p):
    return np.sqrt(EPS[p] / 2)                     # SQRT(DLAMCH('Epsilon')), LAPACK's eps being the rounding unit


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
def _laqp2(A, steps=None, hq=False, tol3z=None, recompute=True):
    """LAPACK's dlaqp2 in float64 on the values of A, stopped after `steps` columns.  Returns (A out, jpvt 1-based, tau of length min(m, n)).
    Pivot: the first maximum of the partial norms over the current positions >= k.  Reflector: dlarfg, beta = -copysign(hypot(alpha,
    xnorm), alpha), tau = 0 when xnorm == 0.  Down-date: 1 - t^2 (hq: (1 + t)(1 - t)), skipped when vn1 == 0, replaced by the recomputed
    norm when temp2 <= tol3z (recompute = False drops that safeguard: a model of a broken kernel, used to check that a case can see it)."""
    A = np.array(A, dtype=np.float64)
    m, n = A.shape
    kmin = min(m, n)
    steps = kmin if steps is None else min(steps, kmin)
    tol3z = np.sqrt(np.finfo(np.float64).eps / 2) if tol3z is None else tol3z
    jp = np.arange(1, n + 1, dtype=np.int64)
    vn1 = np.sqrt((A * A).sum(axis=0))
    vn2 = vn1.copy()
    tau = np.zeros(kmin)
    for k in range(steps):
        p = k + int(np.argmax(vn1[k:]))
        if p != k:
            A[:, [k, p]] = A[:, [p, k]]
            jp[[k, p]] = jp[[p, k]]
            vn1[p], vn2[p] = vn1[k], vn2[k]
        alpha = A[k, k]
        xnorm = np.sqrt(np.dot(A[k + 1:, k], A[k + 1:, k]))
        if xnorm != 0.0:
            beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
            tau[k] = (beta - alpha) / beta
            A[k + 1:, k] *= 1.0 / (alpha - beta)
            A[k, k] = beta
        if k + 1 < n and tau[k] != 0.0:
            v = np.concatenate(([1.0], A[k + 1:, k]))
            w = v @ A[k:, k + 1:]
            A[k:, k + 1:] -= np.outer(v, tau[k] * w)
        for j in range(k + 1, n):
            if vn1[j] == 0.0:
                continue
            t = abs(A[k, j]) / vn1[j]
            temp = max((1.0 + t) * (1.0 - t) if hq else 1.0 - t * t, 0.0)
            temp2 = temp * (vn1[j] / vn2[j]) ** 2
            if recompute and temp2 <= tol3z:
                vn1[j] = np.sqrt(np.dot(A[k + 1:, j], A[k + 1:, j]))
                vn2[j] = vn1[j]
            else:
                vn1[j] *= np.sqrt(temp)
    return A, jp, tau


def _lapack_geqp3(A, p):
    """scipy's dgeqp3 / sgeqp3 (jpvt zero on entry: every column free), result upcast to float64"""
    f = ll.dgeqp3 if p == "f64" else ll.sgeqp3
    qr, jp, tau, _, info = f(np.asfortranarray(A.astype(NP[p])))
    assert info == 0
    return qr.astype(np.float64), jp.astype(np.int64), tau.astype(np.float64)


def _route(m, n, p, num_cu, cols=0):
    """which kernel qr_core (qrcp.hip) runs for a pivoted m x n problem: 'tag' (tag exchange, columns in LDS), 'rdv_cols' (rendezvous,
    columns in LDS), 'rdv_v' (rendezvous, columns in the matrix, reflector in LDS), 'rdv_slot' (reflector read from its published slot)"""
    isz = 8 if p == "f64" else 4
    G = max(1, min((n + 7) // 8, num_cu))
    use_lds = -(-n // G) * m * isz + m * isz <= 140 * 1024
    if not use_lds and (-(-n // num_cu) + 1) * m * isz <= 140 * 1024:
        G, use_lds = num_cu, True
    if use_lds:
        g = cols if cols > 0 else 4
        Gt = max(1, min(-(-n // g), num_cu, 256))
        c = -(-n // Gt)
        if c * 8 + (2 * c + m) * isz + c * m * isz <= 150 * 1024:
            return "tag"
        return "rdv_cols"
    return "rdv_v" if (2 * -(-n // G) + m) * isz <= 140 * 1024 else "rdv_slot"


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _unit_max(A):
    """A scaled by a power of two so that max |a_ij| lies in [1, 2): the exponent-range guard leaves it alone"""
    mx = np.abs(A).max()
    return A * 2.0 ** (-np.frexp(mx)[1] + 1) if mx > 0 else A


def _separated(m, n, rng, p):
    """well-separated column norms (logspace over three decades, permuted), values representable in p, max |a| in [1, 2)"""
    return _unit_max(rng.standard_normal((m, n)) * np.logspace(0, -3, n)[rng.permutation(n)]).astype(NP[p])


def _ties(m, n, rng, p, G):
    """columns c_j e_{r_j} with c_j in {1, 2, 4} (signed): every reflector swaps two rows, every norm stays exact, so the pivot order is
    decided by the tie rule alone.  Tied pairs are planted inside one workgroup's columns (positions j, j + G) and across workgroups."""
    mags = rng.choice([1.0, 2.0, 4.0], size=n)
    for j in range(0, n - G, max(1, n // 8)):
        mags[j] = mags[j + G] = 4.0                 # same workgroup
        mags[(j + 1) % n] = 4.0                      # next workgroup
    rows = rng.permutation(m)[:n] if n <= m else rng.integers(0, m, size=n)
    A = np.zeros((m, n))
    A[rows, np.arange(n)] = mags * rng.choice([-1.0, 1.0], size=n)
    return A.astype(NP[p])


def _with_zeros(m, n, rng, p):
    """separated columns with exact zero columns among them (m > n: every nonzero column is pivoted before them)"""
    A = _separated(m, n, rng, p)
    A[:, rng.choice(n, size=max(1, n // 6), replace=False)] = 0
    return A


def _exact_duplicate(m, n, rng, p):
    """single-support columns (power-of-two magnitudes: every reflector is exact) plus exact duplicates of some of them: a duplicate
    becomes exactly zero below row k once its twin is pivoted (the recomputed norm is 0) and must then be treated as a zero column"""
    A = np.zeros((m, n))
    nd = max(1, n // 5)
    base = n - nd
    rows = rng.permutation(m)[:base]
    A[rows, np.arange(base)] = rng.choice([1.0, 2.0, 4.0, 8.0], size=base) * rng.choice([-1.0, 1.0], size=base)
    A[:, base:] = A[:, rng.choice(base, size=nd, replace=False)]
    return A[:, rng.permutation(n)].astype(NP[p])


def _signed_zero_pivot(m, n, rng, p, sign, later):
    """a pivot entry that is exactly +0.0 / -0.0 with nonzeros below it.  later = False: at step 0 (the largest column's first entry);
    later = True: after r identity reflectors (a positive diagonal block pivoted first: tau = 0, nothing else is touched), at step r"""
    z = np.copysign(0.0, sign)
    r = min(4, n // 4) if later else 0
    B = _separated(m - r, n - r, rng, p).astype(np.float64)
    top = int(np.argmax(np.sqrt((B * B).sum(axis=0))))
    B[:, top] *= 2                                   # clearly the largest, also without its first entry
    B[0, top] = z
    A = np.zeros((m, n))
    A[:r, :r] = np.diag(np.linspace(16.0 * np.sqrt(m), 8.0 * np.sqrt(m), r)) if r else A[:r, :r]
    A[r:, r:] = B
    return A.astype(NP[p])


def _near_dependent(m, n, rng, p):
    """pairs x, x + delta y: once x is pivoted the down-dated norm of its twin is cancellation (temp2 <= sqrt(eps/2)) and only the
    recomputed norm ranks it correctly against filler columns whose norms interleave the residuals"""
    deltas = [3e-8, 1e-8] if p == "f64" else [6e-4, 2e-4]
    npair = max(1, min(4, n // 6))
    cols, k = [], 0
    for i in range(npair):
        x = rng.standard_normal(m)
        x *= (2.0 - 0.1 * i) / np.linalg.norm(x)
        y = rng.standard_normal(m) / np.sqrt(m)
        cols += [x, x + deltas[i % 2] * (1 + 0.3 * i) * y]
    lo, hi = min(deltas) * 0.3, max(deltas) * 3
    while len(cols) < n:
        f = rng.standard_normal(m)
        cols.append(f * (np.geomspace(lo, hi, 9)[k % 9] * (1 + 0.05 * (k // 9))) / np.linalg.norm(f))
        k += 1
    A = np.stack(cols[:n], axis=1)
    return A[:, rng.permutation(n)].astype(NP[p])


def _low_rank(m, n, rng, p, r):
    return _unit_max(rng.standard_normal((m, r)) @ (rng.standard_normal((r, n)) * np.logspace(0, -2, n)[rng.permutation(n)])).astype(NP[p])


# ---------------------------------------------------------------------------------------------------------------------------------------
# device calls
# ---------------------------------------------------------------------------------------------------------------------------------------
def _torch_dt(p):
    import torch

    return torch.float64 if p == "f64" else torch.float32


def _num_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _call(ctx, name, p, A, lda=None, steps=None, rc_expected=0):
    """run rlhip_<name>_<p> on A (m x n, values of precision p) stored with leading dimension lda (guard rows SENT); jpvt / tau hold
    garbage on entry.  Returns (the whole lda x n buffer, jpvt, tau with its guard entry) as numpy."""
    import torch

    from randlapack_amd import device as d

    m, n = A.shape
    lda = lda or max(m, 1)
    buf = np.full((lda, n), SENT, dtype=NP[p])
    buf[:m] = A
    Ad = d.cm_from_numpy(buf) if n else torch.zeros(1, dtype=_torch_dt(p), device="cuda")
    Jd = torch.full((n + 1,), GARBAGE_J, dtype=torch.int64, device="cuda")
    td = torch.full((min(m, n) + 1,), GARBAGE_TAU, dtype=_torch_dt(p), device="cuda")
    fn = getattr(ctx.lib, f"rlhip_{name}_{p}")
    args = (ctx.h, m, n) + (() if steps is None else (steps,)) + (Ad.data_ptr(), lda, Jd.data_ptr(), td.data_ptr())
    assert fn(*args) == rc_expected
    ctx.sync()
    out = d.cm_to_numpy(Ad) if n else np.zeros((lda, 0), dtype=NP[p])
    J, tau = Jd.cpu().numpy(), td.cpu().numpy()
    assert J[n] == GARBAGE_J and tau[min(m, n)] == GARBAGE_TAU, "wrote past the end of jpvt / tau"
    if lda > m:
        assert np.array_equal(_bits(out[m:]), _bits(np.full((lda - m, n), SENT, dtype=NP[p]))), "guard rows below m were written"
    return out, J[:n], tau[:min(m, n)]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _relerr(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    s = np.abs(ref).max() if ref.size else 0.0
    return np.abs(got - ref).max() / (s if s > 0 else 1.0) if ref.size else 0.0


def _check(got, ref, p, units, what):
    e = _relerr(got, ref)
    assert e <= units * EPS[p], f"{what}: error {e / EPS[p]:.1f} eps > {units:.1f} eps"


def _units(m, n):
    return 16.0 * np.sqrt(max(m, 1)) * np.sqrt(max(min(m, n), 1))


def _by_column(R, J):
    """the columns of R put back in the order of A's columns (J 1-based)"""
    return R[:, np.argsort(J)]


def _compare(got, ref, A, p, what, rows=None, pivots=None):
    """got / ref = (A out, J, tau).  J exact (all of it, or the first `pivots`); R (rows < `rows`, upper part) and tau with their signs to a
    multiple of eps; the signs of R's diagonal exactly where it is not rounding noise.  Where only the first pivots are pinned, the rows of
    R are compared column by column of A (the columns beyond them may sit in another order)."""
    (Ag, Jg, tg), (Ar, Jr, tr) = got, ref
    m, n = A.shape
    k = min(m, n)
    rows = k if rows is None else rows
    npv = n if pivots is None else pivots
    np.testing.assert_array_equal(Jg[:npv], Jr[:npv], err_msg=f"{what}: pivots differ")
    assert sorted(Jg.tolist()) == list(range(1, n + 1)), f"{what}: jpvt is not a permutation"
    u = _units(m, n)
    _check(_by_column(np.triu(Ag[:rows, :n]), Jg), _by_column(np.triu(Ar[:rows, :n]), Jr), p, u, f"{what}: R")
    _check(tg[:rows], tr[:rows], p, u, f"{what}: tau")
    dg, dr = np.diag(Ag[:rows, :n]).astype(np.float64), np.diag(Ar[:rows, :n])
    big = np.abs(dr) > 1e3 * u * EPS[p] * np.abs(dr).max()
    np.testing.assert_array_equal(np.signbit(dg[big]), np.signbit(dr[big]), err_msg=f"{what}: signs of diag(R)")


def _backward(Aout, J, tau, A, p, what):
    """|| A P - Q R || / || A || to a multiple of eps, Q applied from the returned reflectors in float64 (dormqr)"""
    m, n = A.shape
    k = min(m, n)
    Ao = Aout[:m, :n].astype(np.float64)
    R = np.triu(Ao)
    QR, _, info = ll.dormqr("L", "N", Ao[:, :k], tau.astype(np.float64), R, max(1, 64 * n))
    assert info == 0
    AP = A.astype(np.float64)[:, J - 1]
    e = np.linalg.norm(AP - QR) / max(np.linalg.norm(AP), 1e-300)
    assert e <= _units(m, n) * EPS[p], f"{what}: backward error {e / EPS[p]:.1f} eps"


def _assert_route(m, n, p, route, cols=0):
    got = _route(m, n, p, _num_cu(), cols)
    assert got == route, f"{p} {m}x{n}: qr_core takes the {got} route on this device, the case is named for {route}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. geqp3 against LAPACK, generic input, on every route
# ---------------------------------------------------------------------------------------------------------------------------------------
GENERIC = [
    ("f64", 1280, 1024, "tag"), ("f64", 200, 300, "tag"), ("f64", 50, 20, "tag"), ("f64", 1, 5, "tag"), ("f64", 5, 1, "tag"),
    ("f64", 4000, 96, "rdv_cols"), ("f64", 9600, 96, "rdv_v"), ("f64", 3000, 2000, "rdv_v"), ("f64", 20000, 96, "rdv_slot"),
    ("f64", 40000, 24, "rdv_slot"),
    ("f32", 1280, 1024, "tag"), ("f32", 2560, 2048, "tag"), ("f32", 4000, 96, "tag"), ("f32", 9600, 96, "rdv_cols"),
    ("f32", 17000, 64, "rdv_cols"), ("f32", 20000, 96, "rdv_v"), ("f32", 36000, 64, "rdv_slot"), ("f32", 40000, 24, "rdv_slot"),
    ("f32", 512, 8192, "tag"),                   # BQRRP's qrcp_wide = geqp3 sketch class: 32 columns per workgroup
]


@gpu
@pytest.mark.parametrize("p,m,n,route", GENERIC, ids=[f"{p}-{m}x{n}-{r}" for p, m, n, r in GENERIC])
def test_geqp3_matches_lapack(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    rng = np.random.default_rng(m * 7 + n)
    A = _separated(m, n, rng, p)
    got = _call(ctx, "geqp3", p, A)
    ref = _lapack_geqp3(A, p)
    _compare(got, ref, A, p, f"{p} {m}x{n}")
    _backward(*got, A, p, f"{p} {m}x{n}")
    dg = np.abs(np.diag(got[0][:min(m, n), :n]).astype(np.float64))
    assert np.all(dg[1:] <= dg[:-1] * (1 + 64 * EPS[p])), "|R_ii| increases"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2-8. edge cases, one shape per route and precision
# ---------------------------------------------------------------------------------------------------------------------------------------
ROUTE_SHAPES = [
    ("f64", 300, 200, "tag"), ("f64", 4000, 96, "rdv_cols"), ("f64", 9600, 96, "rdv_v"), ("f64", 40000, 24, "rdv_slot"),
    ("f32", 4000, 96, "tag"), ("f32", 9600, 96, "rdv_cols"), ("f32", 20000, 96, "rdv_v"), ("f32", 40000, 24, "rdv_slot"),
]
RS_IDS = [f"{p}-{m}x{n}-{r}" for p, m, n, r in ROUTE_SHAPES]


def _G(m, n, p, route):
    """workgroups of the route (positions j and j + G share a workgroup)"""
    ncu = _num_cu()
    if route == "tag":
        return max(1, min(-(-n // 4), ncu, 256))
    G = max(1, min((n + 7) // 8, ncu))
    isz = 8 if p == "f64" else 4
    return ncu if route == "rdv_cols" and -(-n // G) * m * isz + m * isz > 140 * 1024 else G


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_exact_ties_first_maximum_by_current_position(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    A = _ties(m, n, np.random.default_rng(n + 1), p, _G(m, n, p, route))
    got = _call(ctx, "geqp3", p, A)
    ref = _lapack_geqp3(A, p)
    _compare(got, ref, A, p, "ties")
    lq = _laqp2(A, tol3z=_tol3z(p))
    np.testing.assert_array_equal(got[1], lq[1])
    # the arithmetic is exact: R and tau bitwise
    np.testing.assert_array_equal(np.triu(got[0][:, :n]).astype(np.float64), np.triu(lq[0]))
    np.testing.assert_array_equal(got[2].astype(np.float64), lq[2])


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_zero_matrix(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    Aout, J, tau = _call(ctx, "geqp3", p, np.zeros((m, n), dtype=NP[p]))
    np.testing.assert_array_equal(J, np.arange(1, n + 1))
    assert not np.isnan(Aout).any() and not np.isnan(tau).any()
    assert np.array_equal(Aout, np.zeros_like(Aout)) and np.array_equal(tau, np.zeros_like(tau))


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_zero_columns(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    A = _with_zeros(m, n, np.random.default_rng(n + 2), p)
    got = _call(ctx, "geqp3", p, A)
    _compare(got, _lapack_geqp3(A, p), A, p, "zero columns")
    assert not np.isnan(got[0]).any()


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_column_becomes_exactly_zero(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    A = _exact_duplicate(m, n, np.random.default_rng(n + 3), p)
    got = _call(ctx, "geqp3", p, A)
    lq = _laqp2(A, tol3z=_tol3z(p))
    _compare(got, _lapack_geqp3(A, p), A, p, "exact duplicate")
    np.testing.assert_array_equal(got[1], lq[1])
    np.testing.assert_array_equal(np.triu(got[0][:, :n]).astype(np.float64), np.triu(lq[0]))


@gpu
@pytest.mark.parametrize("later", [False, True], ids=["step0", "later"])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus0", "minus0"])
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_signed_zero_pivot_entry(ctx, p, m, n, route, sign, later):
    """alpha = +0.0 gives beta = -xnorm, alpha = -0.0 gives beta = +xnorm (dlarfg's copysign)"""
    _assert_route(m, n, p, route)
    A = _signed_zero_pivot(m, n, np.random.default_rng(n + 4), p, sign, later)
    got = _call(ctx, "geqp3", p, A)
    ref = _lapack_geqp3(A, p)
    _compare(got, ref, A, p, "signed zero pivot")
    r = min(4, n // 4) if later else 0
    assert np.signbit(got[0][r, r]) == (sign > 0) == np.signbit(ref[0][r, r]), "R_rr does not carry dlarfg's sign"


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_norm_recomputation_safeguard(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    A = _near_dependent(m, n, np.random.default_rng(n + 5), p)
    got = _call(ctx, "geqp3", p, A)
    lq = _laqp2(A, tol3z=_tol3z(p))
    np.testing.assert_array_equal(got[1], lq[1], err_msg="pivots differ from dlaqp2 with the recomputation")
    # R: the near-dependent twins leave rows of size delta; an absolute eps multiple of ||A|| is what a backward-stable QR promises
    _check(np.triu(got[0][:, :n]), np.triu(lq[0]), p, _units(m, n), "R")
    _backward(*got, A, p, "safeguard")


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_rank_deficient(ctx, p, m, n, route):
    _assert_route(m, n, p, route)
    r = max(2, n // 3)
    A = _low_rank(m, n, np.random.default_rng(n + 6), p, r)
    got = _call(ctx, "geqp3", p, A)
    ref = _lapack_geqp3(A, p)
    _compare(got, ref, A, p, "rank deficient", rows=r, pivots=r)         # only the leading r pivots are pinned
    _backward(*got, A, p, "rank deficient")


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_lda_guard_rows(ctx, p, m, n, route):
    """lda > m: the guard rows come back bitwise untouched (checked in _call; the tag route copies back with a 2-D copy), the result
    equals the lda == m call bitwise"""
    _assert_route(m, n, p, route)
    A = _separated(m, n, np.random.default_rng(n + 7), p)
    a = _call(ctx, "geqp3", p, A)
    b = _call(ctx, "geqp3", p, A, lda=m + 13)
    assert np.array_equal(_bits(a[0]), _bits(b[0][:m])) and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))


@gpu
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("name", ["geqp3", "geqp3_steps", "qrp_partial"])
def test_argument_codes_and_empty(ctx, p, name):
    steps = None if name == "geqp3" else 2
    for m, n in [(0, 5), (5, 0), (0, 0)]:
        _call(ctx, name, p, np.zeros((m, n), dtype=NP[p]), lda=max(m, 1), steps=steps)       # returns 0, writes nothing (checked)
    import torch

    fn = getattr(ctx.lib, f"rlhip_{name}_{p}")
    buf = torch.full((4, 6), SENT, dtype=_torch_dt(p), device="cuda")
    J = torch.full((5,), GARBAGE_J, dtype=torch.int64, device="cuda")
    t = torch.full((5,), GARBAGE_TAU, dtype=_torch_dt(p), device="cuda")
    st = () if steps is None else (steps,)
    for m, n, lda, rc in [(-1, 4, 6, -2), (6, -1, 6, -3), (6, 4, 5, -5), (6, 4, 0, -5), (1, 4, 0, -5)]:
        assert fn(ctx.h, m, n, *st, buf.data_ptr(), lda, J.data_ptr(), t.data_ptr()) == rc, (m, n, lda)
    ctx.sync()
    assert bool((buf == SENT).all()) and bool((J == GARBAGE_J).all()) and bool((t == GARBAGE_TAU).all())
    # m = 1 and n = 1
    for m, n in [(1, 7), (7, 1), (1, 1)]:
        B = _separated(m, n, np.random.default_rng(m + n), p)
        got = _call(ctx, name, p, B, steps=None if steps is None else min(m, n))
        _compare(got, _lapack_geqp3(B, p), B, p, f"{name} {m}x{n}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# exponent range: the guard of geqrf, on the pivoted routes
# ---------------------------------------------------------------------------------------------------------------------------------------
SCALES = {"f32": [-90, 70], "f64": [-560, 530]}


@gpu
@pytest.mark.parametrize("p,m,n,route", ROUTE_SHAPES, ids=RS_IDS)
def test_geqp3_scaled_input_is_bitwise_scaled(ctx, p, m, n, route):
    """A 2^e with the squares of A's entries outside the exponent range: J and tau bitwise those of A, R bitwise 2^e times A's R"""
    _assert_route(m, n, p, route)
    A = _separated(m, n, np.random.default_rng(n + 8), p)               # max |a| in [1, 2): the guard leaves A itself alone
    a = _call(ctx, "geqp3", p, A)
    for e in SCALES[p]:
        As = (A.astype(np.float64) * 2.0 ** e).astype(NP[p])
        assert np.array_equal(As.astype(np.float64), A.astype(np.float64) * 2.0 ** e)
        b = _call(ctx, "geqp3", p, As)
        np.testing.assert_array_equal(b[1], a[1], err_msg=f"2^{e}: pivots")
        assert np.array_equal(_bits(b[2]), _bits(a[2])), f"2^{e}: tau not bitwise"
        R_exp = (np.triu(a[0]).astype(np.float64) * 2.0 ** e).astype(NP[p])
        assert np.array_equal(_bits(np.triu(b[0])), _bits(R_exp)), f"2^{e}: R not bitwise 2^e R"
        assert np.array_equal(_bits(np.tril(b[0], -1)), _bits(np.tril(a[0], -1))), f"2^{e}: reflectors"


@gpu
@pytest.mark.parametrize("route_shape", [("f32", 300, 200, "tag"), ("f32", 9600, 96, "rdv_cols")], ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}-{r[3]}")
def test_sgeqp3_tiny_input(ctx, route_shape):
    """1e-22 A (not a power of two): pivots of sgeqp3, R and tau to rounding"""
    p, m, n, route = route_shape
    _assert_route(m, n, p, route)
    A = (_separated(m, n, np.random.default_rng(9), p).astype(np.float64) * 1e-22).astype(np.float32)
    got = _call(ctx, "geqp3", p, A)
    _compare(got, _lapack_geqp3(A, p), A, p, "1e-22 A")


@gpu
@pytest.mark.parametrize("name", ["geqp3_steps", "qrp_partial"])
@pytest.mark.parametrize("p,m,n,route", [("f64", 300, 200, "tag"), ("f32", 20000, 96, "rdv_v")], ids=["f64-tag", "f32-rdv_v"])
def test_partial_scaled_input_is_bitwise_scaled(ctx, name, p, m, n, route):
    """a partial factorization of A 2^e: the trailing block (matrix data) comes back scaled too"""
    _assert_route(m, n, p, route)
    A = _separated(m, n, np.random.default_rng(n + 10), p)
    steps = n // 3
    a = _call(ctx, name, p, A, steps=steps)
    for e in SCALES[p]:
        b = _call(ctx, name, p, (A.astype(np.float64) * 2.0 ** e).astype(NP[p]), steps=steps)
        np.testing.assert_array_equal(b[1], a[1])
        assert np.array_equal(_bits(b[2][:steps]), _bits(a[2][:steps]))
        exp = a[0].astype(np.float64).copy()
        iu = np.triu(np.ones((m, n), dtype=bool)) | (np.add.outer(np.arange(m) >= steps, np.zeros(n, dtype=bool)) & (np.arange(n) >= steps))
        exp[iu] *= 2.0 ** e
        assert np.array_equal(_bits(b[0]), _bits(exp.astype(NP[p]))), f"2^{e}: R / trailing block not bitwise 2^e"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. columns per workgroup of the tag kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("p", PRECS)
def test_geqp3_qrcp_cols_is_the_same_factorization(ctx, p):
    """rlhip_set_qrcp_cols in {1, 2, 8, 64}: other workgroup counts, identical J -- and R, tau bitwise (every column's sums are formed by
    the same wavefront reductions whatever the workgroup count)"""
    m, n = 300, 200
    A = _separated(m, n, np.random.default_rng(11), p)
    base = _call(ctx, "geqp3", p, A)
    try:
        for cols in [1, 2, 8, 64]:
            _assert_route(m, n, p, "tag", cols)
            assert ctx.lib.rlhip_set_qrcp_cols(ctx.h, cols) == 0
            got = _call(ctx, "geqp3", p, A)
            np.testing.assert_array_equal(got[1], base[1], err_msg=f"cols={cols}: pivots")
            assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(_bits(got[2]), _bits(base[2])), f"cols={cols}"
    finally:
        assert ctx.lib.rlhip_set_qrcp_cols(ctx.h, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 10. geqp3_steps
# ---------------------------------------------------------------------------------------------------------------------------------------
STEPS_SHAPES = [("f64", 300, 200, "tag"), ("f64", 9600, 96, "rdv_v"), ("f32", 4000, 96, "tag"), ("f32", 40000, 24, "rdv_slot")]


@gpu
@pytest.mark.parametrize("which", ["1", "half", "min-1", "min", "over"])
@pytest.mark.parametrize("p,m,n,route", STEPS_SHAPES, ids=[f"{p}-{m}x{n}-{r}" for p, m, n, r in STEPS_SHAPES])
def test_geqp3_steps_matches_laqp2(ctx, p, m, n, route, which):
    _assert_route(m, n, p, route)
    k = min(m, n)
    steps = {"1": 1, "half": k // 2, "min-1": k - 1, "min": k, "over": k + 5}[which]
    A = _separated(m, n, np.random.default_rng(n + 12), p)
    got = _call(ctx, "geqp3_steps", p, A, steps=steps)
    s = min(steps, k)
    lq = _laqp2(A, steps=s, tol3z=_tol3z(p))
    full = _call(ctx, "geqp3", p, A)
    u = _units(m, n)
    np.testing.assert_array_equal(got[1], lq[1], err_msg="permutation differs from dlaqp2's after `steps` steps")
    np.testing.assert_array_equal(got[1][:s], full[1][:s], err_msg="leading pivots differ from geqp3's")
    _check(got[0][:s], lq[0][:s], p, u, "finished rows of R (and the reflectors in them)")
    _check(_by_column(np.triu(got[0][:s]), got[1]), _by_column(np.triu(full[0][:s]), full[1]), p, u, "finished rows against geqp3")
    _check(got[0][s:, s:], lq[0][s:, s:], p, u, "trailing block")
    _check(np.tril(got[0][:, :s], -1), np.tril(lq[0][:, :s], -1), p, u, "reflectors")
    _check(got[2][:s], lq[2][:s], p, u, "tau")


@gpu
@pytest.mark.parametrize("m,n,h", [(1280, 1024, 512), (700, 300, 100)])
def test_geqp3_in_two_halves_is_geqp3_f32(ctx, m, n, h):
    """fp32 twin of test_gpu_fullsize.py::test_geqp3_in_two_halves_is_geqp3: geqp3_steps (h steps) + geqp3 of the trailing block, its
    pivots applied to the finished rows and composed into jpvt == geqp3 (pivots identical, R and tau to rounding)"""
    import torch

    from randlapack_amd import device as d

    rng = np.random.default_rng(m + n + h)
    A0 = _separated(m, n, rng, "f32")
    f32 = torch.float32
    Af = d.cm_from_numpy(A0); Jf = torch.zeros(n, dtype=torch.int64, device="cuda"); tf = torch.zeros(n, dtype=f32, device="cuda")
    assert ctx.lib.rlhip_geqp3_f32(ctx.h, m, n, Af.data_ptr(), m, Jf.data_ptr(), tf.data_ptr()) == 0
    As = d.cm_from_numpy(A0); Js = torch.zeros(n, dtype=torch.int64, device="cuda"); ts = torch.zeros(n, dtype=f32, device="cuda")
    assert ctx.lib.rlhip_geqp3_steps_f32(ctx.h, m, n, h, As.data_ptr(), m, Js.data_ptr(), ts.data_ptr()) == 0
    part, refh = d.cm_to_numpy(As), d.cm_to_numpy(Af)
    assert np.array_equal(Js.cpu().numpy()[:h], Jf.cpu().numpy()[:h])
    _check(np.triu(part[:h, :h]), np.triu(refh[:h, :h]), "f32", _units(m, n), "leading block of R")
    J2 = torch.zeros(n - h, dtype=torch.int64, device="cuda")
    es = 4
    assert ctx.lib.rlhip_geqp3_f32(ctx.h, m - h, n - h, As.data_ptr() + (h + h * m) * es, m, J2.data_ptr(), ts.data_ptr() + h * es) == 0
    assert ctx.lib.rlhip_col_swap_f32(ctx.h, h, n - h, n - h, As.data_ptr() + h * m * es, m, J2.data_ptr()) == 0
    assert ctx.lib.rlhip_col_swap_i64(ctx.h, n - h, n - h, Js.data_ptr() + h * 8, J2.data_ptr()) == 0
    assert np.array_equal(Js.cpu().numpy(), Jf.cpu().numpy())
    got, ref = d.cm_to_numpy(As), d.cm_to_numpy(Af)
    k = min(m, n)
    _check(np.triu(got)[:k], np.triu(ref)[:k], "f32", _units(m, n), "R")
    _check(ts.cpu().numpy()[:k], tf.cpu().numpy()[:k], "f32", _units(m, n), "tau")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 11. qrp_partial at HQRRP's call shapes (rl_hqrrp.hh: m_Y x n_R with b steps, b x b with lda = nb_alg, m_AB1 x b)
# ---------------------------------------------------------------------------------------------------------------------------------------
HQ_SHAPES = [(72, 900, 64, None), (40, 40, 40, 64), (64, 64, 64, 128), (900, 64, 64, None), (3000, 32, 32, None)]


@gpu
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,steps,lda", HQ_SHAPES, ids=[f"{m}x{n}-b{s}-lda{l or m}" for m, n, s, l in HQ_SHAPES])
def test_qrp_partial_matches_laqp2_hq(ctx, p, m, n, steps, lda):
    A = _separated(m, n, np.random.default_rng(m + n + steps), p)
    got = _call(ctx, "qrp_partial", p, A, lda=lda, steps=steps)
    s = min(steps, m, n)
    lq = _laqp2(A, steps=s, hq=True, tol3z=_tol3z(p))
    u = _units(m, n)
    np.testing.assert_array_equal(got[1], lq[1], err_msg="whole permutation (swapped-out indices beyond `steps` included)")
    _check(got[2][:s], lq[2][:s], p, u, "tau")
    _check(got[0][:s, :n], lq[0][:s], p, u, "finished rows of R")
    _check(got[0][s:m, s:], lq[0][s:, s:], p, u, "updated trailing block")
    _check(np.tril(got[0][:m, :s], -1), np.tril(lq[0][:, :s], -1), p, u, "reflectors")


@gpu
@pytest.mark.parametrize("p", PRECS)
def test_qrp_partial_safeguard_and_ties(ctx, p):
    m, n = 300, 200
    for A in (_near_dependent(m, n, np.random.default_rng(13), p), _ties(m, n, np.random.default_rng(14), p, 50)):
        got = _call(ctx, "qrp_partial", p, A, steps=64)
        lq = _laqp2(A, steps=64, hq=True, tol3z=_tol3z(p))
        np.testing.assert_array_equal(got[1], lq[1])
        _check(got[0][:64], lq[0][:64], p, _units(m, n), "finished rows")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference itself (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n", [(60, 40), (40, 60), (200, 100), (1, 5), (5, 1)])
def test_laqp2_reference_reproduces_lapack(p, m, n):
    """_laqp2(hq=False) == dgeqp3 on well-separated inputs (pivots exactly, R and tau to rounding), on exact ties and exact duplicates
    (bitwise: the arithmetic is exact), on a +-0.0 pivot entry (dlarfg's sign); the near-dependent case does trigger the safeguard
    (dropping it changes the pivots), and _route reproduces the route table of qr_core on 256 CUs"""
    rng = np.random.default_rng(m + n)
    A = _separated(m, n, rng, p).astype(np.float64)
    qr, jp, tau = _lapack_geqp3(A, "f64")
    lq = _laqp2(A)
    np.testing.assert_array_equal(lq[1], jp)
    assert _relerr(np.triu(lq[0]), np.triu(qr)) < 1e3 * EPS["f64"] and _relerr(lq[2], tau) < 1e3 * EPS["f64"]
    assert _relerr(np.tril(lq[0], -1), np.tril(qr, -1)) < 1e3 * EPS["f64"]
    if m >= n > 4:
        for B in (_ties(m, n, rng, p, 3), _exact_duplicate(m, n, rng, p)):
            B = B.astype(np.float64)
            qr, jp, tau = _lapack_geqp3(B, "f64")
            lq = _laqp2(B)
            np.testing.assert_array_equal(lq[1], jp)
            np.testing.assert_array_equal(np.triu(lq[0]), np.triu(qr))
            np.testing.assert_array_equal(lq[2], tau)
        for sign in (1.0, -1.0):
            for later in (False, True):
                B = _signed_zero_pivot(m, n, rng, p, sign, later).astype(np.float64)
                qr, jp, tau = _lapack_geqp3(B, "f64")
                lq = _laqp2(B)
                np.testing.assert_array_equal(lq[1], jp)
                r = min(4, n // 4) if later else 0
                assert np.signbit(lq[0][r, r]) == np.signbit(qr[r, r]) == (sign > 0)


@pytest.mark.parametrize("p", ["f64"])
@pytest.mark.parametrize("m,n", [(300, 200), (4000, 96), (40000, 24)])
def test_near_dependent_case_needs_the_safeguard(p, m, n):
    """without the recomputation the reference ranks the twins differently: the case can tell a kernel that drops it.  (fp64 only: the
    float64 reference down-dates the fp32 case's norms accurately where an fp32 kernel cancels, so only a device run can show it there)"""
    A = _near_dependent(m, n, np.random.default_rng(n + 5), p)
    a = _laqp2(A, tol3z=_tol3z(p))
    b = _laqp2(A, tol3z=_tol3z(p), recompute=False)
    assert not np.array_equal(a[1], b[1])
    if p == "f64" and n <= 200:
        np.testing.assert_array_equal(_lapack_geqp3(A, "f64")[1][:8], a[1][:8])


def test_route_table_on_256_cus():
    for p, m, n, r in GENERIC + ROUTE_SHAPES + STEPS_SHAPES:
        assert _route(m, n, p, 256) == r, (p, m, n)
    for cols in [1, 2, 8, 64]:
        assert _route(300, 200, "f64", 256, cols) == "tag" and _route(300, 200, "f32", 256, cols) == "tag"
