"""-m gpu: the device SVDs (rlhip_gesdd_*, rlhip_gesvdj_*; svd.hip, jacobi.hip) through the C ABI in fp64 and fp32 on every route they
can take, against numpy.linalg.svd of the same input in float64.

Every case asserts by path-counter delta (include/rlhip.h: 6, 10, 16 .. 25) the route it was written for.  The inputs that steer gesdd
come from tests/_svd_inputs.py, where a CPU test replays the route decisions and holds each to a factor 10 from its threshold.

Tolerances are those of the existing SVD tests in test_gpu_kernels.py, as multiples of the quantities they bound:
  fp64  |S - S_ref| <= 1e-13 sqrt(n) sigma_1,  ||U S VT - A||_F <= 1e-13 sqrt(n) ||A||_F,  ||U^T U - I||_F, ||VT VT^T - I||_F <= 1e-12 sqrt(n)
  fp32  5 eps32 sigma_1,  20 eps32 ||A||_F,  10 sqrt(n) eps32
Routes that are known to cost eps cond (one pass, recovered V) or eps cond^2 (Gram) in the orthogonality of U add exactly that term, with the
condition number of the spectrum the input was built from."""
import ctypes as C

import numpy as np
import pytest

import _svd_inputs as si

pytestmark = pytest.mark.gpu
E64, E32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
GUARD = -777.25                                     # what the rows beyond m / n of every buffer hold
ROUTE_SLOTS = (10, 16, 17, 18, 19, 20)              # gesdd: Gram, two passes, one pass, recovered V, Jacobi on A, undo
SWEEP_SLOTS = (6, 21, 22, 23, 24, 25)               # gesvdj: persistent, 16 x 256, 16 x 512, 32 wide, per round, fp32 widened
ROUTE_OF = {"a": 10, "b": 16, "c": 17, "d": 18, "e": 19, "f": 20}


def _dev():
    from randlapack_amd import device

    return device


def _tdt(prec):
    import torch

    return torch.float64 if prec == "f64" else torch.float32


def _tol(prec, n):
    if prec == "f64":
        return dict(s=1e-13 * np.sqrt(n), rec=1e-13 * np.sqrt(n), orth=1e-12 * np.sqrt(n), eps=E64)
    return dict(s=5 * E32, rec=20 * E32, orth=10 * np.sqrt(n) * E32, eps=E32)


def _padded(A, ld, prec):
    """device buffer of ld rows holding A on top of GUARD rows (column-major, ld = leading dimension)"""
    buf = np.full((ld, A.shape[1]), GUARD, dtype=si.NPDT[prec])
    buf[:A.shape[0]] = A
    return _dev().cm_from_numpy(buf)


def _counts(ctx, slots):
    return {k: ctx.path_count(k) for k in slots}


def _delta(ctx, before):
    return {k: ctx.path_count(k) - v for k, v in before.items()}


def gesdd(ctx, A, prec, lda=None, ldu=None, ldvt=None):
    """-> info, sweeps, U, S, VT (float64 copies), the route-counter deltas, and the three buffers as they came back (ld rows each)"""
    import torch

    d = _dev()
    m, n = A.shape
    lda, ldu, ldvt = lda or max(m, 1), ldu or max(m, 1), ldvt or max(n, 1)
    Ad = _padded(A.astype(si.NPDT[prec]), lda, prec)
    Ud = _padded(np.full((m, n), np.nan), ldu, prec)
    VTd = _padded(np.full((n, n), np.nan), ldvt, prec)
    S = torch.full((max(n, 1),), float("nan"), dtype=_tdt(prec), device="cuda")
    sw = C.c_int(-1)
    before = _counts(ctx, ROUTE_SLOTS + SWEEP_SLOTS)
    info = getattr(ctx.lib, f"rlhip_gesdd_{prec}")(ctx.h, m, n, Ad.data_ptr(), lda, S.data_ptr(), Ud.data_ptr(), ldu, VTd.data_ptr(), ldvt, C.byref(sw))
    took = _delta(ctx, before)
    raw = (d.cm_to_numpy(Ad), d.cm_to_numpy(Ud), d.cm_to_numpy(VTd))
    return info, sw.value, raw[1][:m].astype(np.float64), S.cpu().numpy()[:n].astype(np.float64), raw[2][:n].astype(np.float64), took, raw


def gesvdj(ctx, A, prec, want_vt=True, lda=None, ldvt=None):
    import torch

    d = _dev()
    m, n = A.shape
    lda, ldvt = lda or max(m, 1), ldvt or max(n, 1)
    Ad = _padded(A.astype(si.NPDT[prec]), lda, prec)
    VTd = _padded(np.full((n, n), np.nan), ldvt, prec)
    S = torch.full((max(n, 1),), float("nan"), dtype=_tdt(prec), device="cuda")
    sw = C.c_int(-1)
    before = _counts(ctx, ROUTE_SLOTS + SWEEP_SLOTS)
    info = getattr(ctx.lib, f"rlhip_gesvdj_{prec}")(ctx.h, m, n, Ad.data_ptr(), lda, S.data_ptr(), VTd.data_ptr() if want_vt else None, ldvt, C.byref(sw))
    took = _delta(ctx, before)
    raw = (d.cm_to_numpy(Ad), d.cm_to_numpy(VTd))
    return info, sw.value, raw[0][:m].astype(np.float64), S.cpu().numpy()[:n].astype(np.float64), raw[1][:n].astype(np.float64), took, raw


def check_svd(A, U, S, VT, prec, u_extra=0.0, rank=None, scale=1.0):
    """the assertions of the module docstring on A = U S VT (A: the float64 copy of what the device was given, divided by `scale`; S is
    compared after the same exact division).  rank: the rank-deficiency contract of include/rlhip.h instead of a fully orthonormal U."""
    m, n = A.shape
    t = _tol(prec, n)
    sref = np.linalg.svd(A, compute_uv=False)
    S = S / scale
    print(f"  sigma err {np.abs(S - sref).max() / max(sref[0], 1e-300):.2e} (<= {t['s']:.1e}), recon {np.linalg.norm((U * S) @ VT - A) / max(np.linalg.norm(A), 1e-300):.2e} "
          f"(<= {t['rec']:.1e}), U orth {np.linalg.norm(U.T @ U - np.eye(n)):.2e}, VT orth {np.linalg.norm(VT @ VT.T - np.eye(n)):.2e} (<= {t['orth']:.1e} + {u_extra:.1e})")
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(VT))
    assert np.all(S >= 0) and np.all(np.diff(S) <= 0)
    assert np.abs(S - sref).max() <= t["s"] * sref[0]
    assert np.linalg.norm((U * S) @ VT - A) <= t["rec"] * np.linalg.norm(A)
    assert np.linalg.norm(VT @ VT.T - np.eye(n)) <= t["orth"]
    if rank is None:
        assert np.linalg.norm(U.T @ U - np.eye(n)) <= t["orth"] + u_extra
    else:
        c_s = 1e-13 / E64 if prec == "f64" else 5.0          # the sigma tolerance above as a multiple of eps
        assert np.all(S[rank:] <= c_s * n * t["eps"] * sref[0])
        assert np.linalg.norm(U[:, :rank].T @ U[:, :rank] - np.eye(rank)) <= t["orth"]
        assert np.all(np.linalg.norm(U[:, rank:], axis=0) <= 1.0 + t["orth"])


def expected_sweep_driver(m, n, prec, want_vt):
    exp = dict.fromkeys(SWEEP_SLOTS, 0)
    if prec == "f32":
        exp[25] = 1
    if n > 1:
        if m > 512:
            exp[24] = 1
        elif m > 256:
            exp[22] = 1
        elif n <= 32:
            exp[23] = 1
        elif not want_vt:
            exp[6] = 1
        else:
            exp[21] = 1
    return exp


def route_counts(routes):
    exp = dict.fromkeys(ROUTE_SLOTS, 0)
    for r in routes:
        exp[ROUTE_OF[r]] = 1
    return exp


def _only(took, slots):
    return {k: took[k] for k in slots}


# ---------------------------------------------------------------------------------------------------
# gesdd: every route that data can reach, in the precisions the CPU replay vouches for
# ---------------------------------------------------------------------------------------------------
def _cond_of(A):
    s = np.linalg.svd(A, compute_uv=False)
    return s[0] / s[-1] if s[-1] > 0 else np.inf


def _u_extra(routes, A, prec, n):
    eps = E64 if prec == "f64" else E32
    if "a" in routes:
        return eps * _cond_of(A) ** 2 * np.sqrt(n)
    if "c" in routes or "d" in routes:
        return eps * _cond_of(A) * np.sqrt(n)
    return 0.0


@pytest.mark.parametrize("name,prec", [(name, prec) for name, spec in si.ROUTE_CASES.items() for prec in spec[1]])
def test_gesdd_routes(ctx, name, prec):
    build, _, gram, routes = si.ROUTE_CASES[name]
    A = build().astype(si.NPDT[prec]).astype(np.float64)
    m, n = A.shape
    ctx.set_option("gesdd_gram", 1 if gram else 0)
    info, sw, U, S, VT, took, _ = gesdd(ctx, A, prec)
    print(name, prec, "routes", routes, "counters", took, "sweeps", sw)
    assert info == 0
    assert _only(took, ROUTE_SLOTS) == route_counts(routes)
    assert 0 < sw < 60
    rank = n - 1 if name in ("duplicate_column", "zero_column") else None
    check_svd(A, U, S, VT, prec, u_extra=_u_extra(routes, A, prec, n), rank=rank)


# ---------------------------------------------------------------------------------------------------
# gesvdj: every sweep driver, with and without VT
# ---------------------------------------------------------------------------------------------------
SWEEP_SHAPES = [(200, 24), (256, 100), (64, 64), (400, 70), (300, 33), (700, 50), (600, 9), (200, 7), (10, 2), (50, 1), (1, 1)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("want_vt", [True, False])
@pytest.mark.parametrize("m,n", SWEEP_SHAPES)
def test_gesvdj_sweep_drivers(ctx, m, n, want_vt, prec):
    """m <= 256 with n <= 32 (32-wide panels) and n > 32 (16-wide; without VT the persistent launch), 256 < m <= 512 (512-row panels),
    m > 512 (one launch per round), odd n (a phantom column pairs with the last one), n = 2, n = 1 (no sweep at all) and m = n = 1"""
    A = si.with_spectrum(m, n, np.logspace(0, -3, n), 100 * m + n).astype(si.NPDT[prec]).astype(np.float64)
    info, sw, U, S, VT, took, _ = gesvdj(ctx, A, prec, want_vt)
    print((m, n), prec, "VT" if want_vt else "no VT", "counters", took, "sweeps", sw)
    assert info == 0
    assert _only(took, SWEEP_SLOTS) == expected_sweep_driver(m, n, prec, want_vt) and not any(took[k] for k in ROUTE_SLOTS)
    assert (0 < sw < 60) if n > 1 else sw == 0
    t = _tol(prec, n)
    if want_vt:
        check_svd(A, U, S, VT, prec)
    else:
        sref = np.linalg.svd(A, compute_uv=False)
        B = U.T @ A                                        # = S VT for the VT that was not asked for
        assert np.all(np.diff(S) <= 0) and np.abs(S - sref).max() <= t["s"] * sref[0]
        assert np.linalg.norm(U.T @ U - np.eye(n)) <= t["orth"]
        assert np.linalg.norm(U @ B - A) <= t["rec"] * np.linalg.norm(A)
        assert np.linalg.norm(B @ B.T - np.diag(S ** 2)) <= t["orth"] * sref[0] ** 2


def test_gesvdj_one_by_one_keeps_the_sign_in_u(ctx):
    for prec in ("f64", "f32"):
        info, sw, U, S, VT, took, _ = gesvdj(ctx, np.array([[-3.0]]), prec)
        assert (info, sw, U[0, 0], S[0], VT[0, 0]) == (0, 0, -1.0, 3.0, 1.0)
        assert _only(took, SWEEP_SLOTS) == expected_sweep_driver(1, 1, prec, True)


# ---------------------------------------------------------------------------------------------------
# leading dimensions
# ---------------------------------------------------------------------------------------------------
LD_CASES = ["gram_wellcond", "onepass_small", "onepass_recover_n2", "twopass_cond3e3", "twopass_cond160_f32", "graded_ratio", "graded_ratio_f32", "zero_column"]


@pytest.mark.parametrize("name,prec", [(name, prec) for name in LD_CASES for prec in si.ROUTE_CASES[name][1]])
def test_gesdd_leading_dimensions_and_guard_rows(ctx, name, prec):
    """lda > m, ldu > m, ldvt > n on each route: the rows beyond m of A (which gesdd destroys) and of U and beyond n of VT come back bitwise"""
    build, precs, gram, routes = si.ROUTE_CASES[name]
    A = build().astype(si.NPDT[prec]).astype(np.float64)
    m, n = A.shape
    ctx.set_option("gesdd_gram", 1 if gram else 0)
    info, sw, U, S, VT, took, (Ar, Ur, VTr) = gesdd(ctx, A, prec, lda=m + 3, ldu=m + 5, ldvt=n + 2)
    assert info == 0 and _only(took, ROUTE_SLOTS) == route_counts(routes)
    assert np.all(Ar[m:] == GUARD) and np.all(Ur[m:] == GUARD) and np.all(VTr[n:] == GUARD)
    check_svd(A, U, S, VT, prec, u_extra=_u_extra(routes, A, prec, n), rank=n - 1 if name == "zero_column" else None)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("rows,cols", [(64, 32), (32, 32)])
def test_gesdd_block_of_a_larger_matrix_as_abrik_passes_it(ctx, rows, cols, prec):
    """ABRIK hands gesdd the leading end_rows x end_cols block of its n-row R or S factor with lda = n: block upper triangular, the rest
    of the big matrix must not change"""
    rng = np.random.default_rng(rows + cols)
    big = rng.standard_normal((500, cols))
    blk = np.triu(rng.standard_normal((rows, cols)), -15) + 4.0 * np.eye(rows, cols)
    big[:rows] = blk
    big = big.astype(si.NPDT[prec])
    d = _dev()
    import torch

    Bd = d.cm_from_numpy(big)
    U, VT = d.cm_empty(rows, cols, dtype=_tdt(prec)), d.cm_empty(cols, cols, dtype=_tdt(prec))
    S = torch.empty(cols, dtype=_tdt(prec), device="cuda")
    before = _counts(ctx, ROUTE_SLOTS)
    info = getattr(ctx.lib, f"rlhip_gesdd_{prec}")(ctx.h, rows, cols, Bd.data_ptr(), 500, S.data_ptr(), U.data_ptr(), rows, VT.data_ptr(), cols, None)
    took = _delta(ctx, before)
    assert info == 0
    assert took[16] + took[17] + took[19] == 1 and took[10] == took[20] == 0          # n <= 32: never the Gram route
    assert np.array_equal(d.cm_to_numpy(Bd)[rows:], big[rows:])
    check_svd(big[:rows].astype(np.float64), d.cm_to_numpy(U).astype(np.float64), S.cpu().numpy().astype(np.float64), d.cm_to_numpy(VT).astype(np.float64), prec,
              u_extra=(E64 if prec == "f64" else E32) * _cond_of(blk) * np.sqrt(cols))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("want_vt", [True, False])
@pytest.mark.parametrize("m,n", [(200, 24), (256, 100), (400, 70), (700, 50)])
def test_gesvdj_leading_dimensions_and_guard_rows(ctx, m, n, want_vt, prec):
    A = si.with_spectrum(m, n, np.logspace(0, -2, n), 7 * m + n).astype(si.NPDT[prec]).astype(np.float64)
    info, sw, U, S, VT, took, (Ar, VTr) = gesvdj(ctx, A, prec, want_vt, lda=m + 3, ldvt=n + 2)
    assert info == 0 and _only(took, SWEEP_SLOTS) == expected_sweep_driver(m, n, prec, want_vt)
    assert np.all(Ar[m:] == GUARD) and np.all(VTr[n:] == GUARD)
    if want_vt:
        check_svd(A, U, S, VT, prec)
    else:
        assert np.all(np.isnan(VTr[:n]))                  # VT == NULL: nothing written
        t = _tol(prec, n)
        assert np.abs(S - np.linalg.svd(A, compute_uv=False)).max() <= t["s"] * S[0] and np.linalg.norm(U.T @ U - np.eye(n)) <= t["orth"]


# ---------------------------------------------------------------------------------------------------
# scaled inputs: A 2^e
# ---------------------------------------------------------------------------------------------------
EXPONENTS = {"f64": [498, -498, 531, -531, -515], "f32": [60, -60, 66, -66]}     # entries ~1e+-150, 1e+-160, 1e-155 / 1e+-18, 1e+-20
SCALED = [("gesvdj", (200, 24)), ("gesvdj", (700, 50)), ("gesvdj", (50, 1)), ("gesdd", "gram_wellcond"), ("gesdd", "onepass_recover"), ("gesdd", "onepass_recover_n2"),
          ("gesdd", "twopass_cond3e3"), ("gesdd", "twopass_cond160_f32"), ("gesdd", "graded_ratio"), ("gesdd", "graded_ratio_f32")]


def _scaled_params():
    for which, what in SCALED:
        for prec in (("f64", "f32") if which == "gesvdj" else si.ROUTE_CASES[what][1]):
            for e in EXPONENTS[prec]:
                yield which, what, prec, e


@pytest.mark.parametrize("which,what,prec,e", list(_scaled_params()))
def test_scaled_inputs(ctx, which, what, prec, e):
    """Scaling by 2^e is exact, so S must be 2^e S_ref and U, VT must meet the tolerances of the unscaled call -- on the same route.
    1e+-150 .. 1e+-160 (fp64) and 1e+-18 .. 1e+-20 (fp32) put every plain sum of squares out of range; 2^-515 and 2^-66 put the Gram
    matrix among the subnormals, where a Cholesky factorization may succeed on garbage."""
    if which == "gesvdj":
        m, n = what
        A = si.with_spectrum(m, n, np.logspace(0, -3, n), 100 * m + n)
        run = lambda M: gesvdj(ctx, M, prec)
        slots, exp = SWEEP_SLOTS, expected_sweep_driver(m, n, prec, True)
        extra = 0.0
    else:
        build, precs, gram, routes = si.ROUTE_CASES[what]
        A = build()
        ctx.set_option("gesdd_gram", 1 if gram else 0)
        run = lambda M: gesdd(ctx, M, prec)
        slots, exp = ROUTE_SLOTS, route_counts(routes)
        extra = _u_extra(routes, A, prec, A.shape[1])
    A = A.astype(si.NPDT[prec]).astype(np.float64)
    f = 2.0 ** e
    assert np.all(np.isfinite((A * f).astype(si.NPDT[prec]))) and np.array_equal((A * f).astype(si.NPDT[prec]).astype(np.float64) / f, A)   # exact, no entry lost
    info0, sw0, U0, S0, VT0, took0, _ = run(A)
    info, sw, U, S, VT, took, _ = run(A * f)
    bitwise = np.array_equal(U, U0) and np.array_equal(VT, VT0) and np.array_equal(S, S0 * f)
    print(which, what, prec, f"2^{e}", "counters", took, "sweeps", sw, sw0, "bitwise 2^e times the unscaled result:", bitwise)
    assert info0 == 0 and info == 0
    assert _only(took0, slots) == exp and _only(took, slots) == exp
    check_svd(A, U, S, VT, prec, u_extra=extra, scale=f)


# ---------------------------------------------------------------------------------------------------
# rank deficiency (the contract in include/rlhip.h)
# ---------------------------------------------------------------------------------------------------
def _rank_inputs():
    dup = si.rank_deficient(300, 20, 20, 5)
    dup[:, 11] = dup[:, 3]
    dup[:, 19] = dup[:, 3]
    zc = si.rank_deficient(300, 20, 20, 6)
    zc[:, 7] = 0.0
    return {"product_r5": (si.rank_deficient(300, 20, 5, 3), 5), "product_r10_n48": (si.rank_deficient(600, 48, 10, 4), 10), "zero_matrix": (np.zeros((100, 8)), 0),
            "zero_column": (zc, 19), "duplicated_columns": (dup, 18), "product_r3_tall": (si.rank_deficient(700, 12, 3, 7), 3)}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("which", ["gesdd", "gesvdj"])
@pytest.mark.parametrize("name", ["product_r5", "product_r10_n48", "zero_matrix", "zero_column", "duplicated_columns", "product_r3_tall"])
def test_rank_deficient(ctx, name, which, prec):
    """exact rank r < n (integer factors: the product is exact in both precisions).  info == 0, everything finite, S_j <= c n eps sigma_1
    for j >= r, the reconstruction and VT as for full rank, the leading r columns of U orthonormal and the others of norm <= 1 -- LAPACK
    would make those orthonormal too; this library leaves a zero column of U beside an exactly zero singular value.  gesdd gets there
    through the Jacobi-on-A route: the first Cholesky factorization fails or shows its diagonal ratio."""
    A, r = _rank_inputs()[name]
    m, n = A.shape
    if which == "gesdd":
        info, sw, U, S, VT, took, _ = gesdd(ctx, A, prec)
        assert _only(took, ROUTE_SLOTS) == route_counts("e")
    else:
        info, sw, U, S, VT, took, _ = gesvdj(ctx, A, prec)
        assert _only(took, SWEEP_SLOTS) == expected_sweep_driver(m, n, prec, True)
    print(name, which, prec, "counters", took, "sweeps", sw, "S tail", S[r:][:4])
    assert info == 0 and 0 < sw < 60
    check_svd(A, U, S, VT, prec, rank=r)
    if name == "zero_matrix":
        assert np.all(S == 0) and np.all(U == 0) and np.array_equal(np.abs(VT), np.eye(n))


# ---------------------------------------------------------------------------------------------------
# argument codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,lda,ldu,ldvt,code", [(-1, 3, 8, 8, 3, -2), (8, -1, 8, 8, 3, -3), (2, 3, 8, 8, 3, -2), (8, 3, 7, 8, 3, -5), (8, 3, 8, 7, 3, -8),
                                                   (8, 3, 8, 8, 2, -10), (0, 0, 0, 1, 1, -5), (0, 0, 1, 0, 1, -8), (0, 0, 1, 1, 0, -10), (8, 0, 8, 8, 1, 0), (0, 0, 1, 1, 1, 0)])
def test_gesdd_argument_codes(ctx, m, n, lda, ldu, ldvt, code, prec):
    """LAPACK's positions of gesdd(jobz, m, n, A, lda, S, U, ldu, VT, ldvt); a refused call and n == 0 write nothing and count no route"""
    import torch

    A = torch.full((64,), 2.5, dtype=_tdt(prec), device="cuda")
    U, VT, S = (torch.full((64,), float("nan"), dtype=_tdt(prec), device="cuda") for _ in range(3))
    sw = C.c_int(-1)
    before = _counts(ctx, ROUTE_SLOTS + SWEEP_SLOTS)
    rc = getattr(ctx.lib, f"rlhip_gesdd_{prec}")(ctx.h, m, n, A.data_ptr(), lda, S.data_ptr(), U.data_ptr(), ldu, VT.data_ptr(), ldvt, C.byref(sw))
    assert rc == code
    assert not any(_delta(ctx, before).values())
    assert bool(torch.all(A == 2.5)) and all(bool(torch.all(torch.isnan(x))) for x in (U, VT, S))
    assert sw.value == (0 if code == 0 else -1)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,lda,ldvt,vt,code", [(-1, 3, 8, 3, True, -2), (8, -1, 8, 3, True, -3), (2, 3, 8, 3, True, -2), (8, 3, 7, 3, True, -5), (8, 3, 8, 2, True, -8),
                                                  (0, 0, 0, 1, True, -5), (0, 0, 1, 0, True, -8), (8, 0, 8, 1, True, 0), (0, 0, 1, 1, False, 0)])
def test_gesvdj_argument_codes(ctx, m, n, lda, ldvt, vt, code, prec):
    import torch

    A = torch.full((64,), 2.5, dtype=_tdt(prec), device="cuda")
    VT, S = (torch.full((64,), float("nan"), dtype=_tdt(prec), device="cuda") for _ in range(2))
    sw = C.c_int(-1)
    before = _counts(ctx, ROUTE_SLOTS + SWEEP_SLOTS)
    rc = getattr(ctx.lib, f"rlhip_gesvdj_{prec}")(ctx.h, m, n, A.data_ptr(), lda, S.data_ptr(), VT.data_ptr() if vt else None, ldvt, C.byref(sw))
    assert rc == code
    assert not any(_delta(ctx, before).values())
    assert bool(torch.all(A == 2.5)) and all(bool(torch.all(torch.isnan(x))) for x in (VT, S))
    assert sw.value == (0 if code == 0 else -1)


def test_path_counter_range(ctx):
    assert ctx.path_count(32) >= 0 and ctx.path_count(42) >= 0 and ctx.path_count(43) == -1 and ctx.path_count(-1) == -1


# ---------------------------------------------------------------------------------------------------
# repeated and clustered singular values in fp32 (test_gpu_kernels.py has the fp64 ones)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["gesdd", "gesvdj"])
@pytest.mark.parametrize("m,n,kind", [(400, 32, "cluster"), (2000, 64, "cluster"), (256, 256, "identity-like"), (3000, 128, "two-clusters"), (700, 40, "identity-like")])
def test_clustered_singular_values_f32(ctx, m, n, kind, which):
    """nearly multiple singular values (a cluster 1e3 eps32 wide, exact copies, two clusters): tiny cosines still rotate by large angles"""
    rng = np.random.default_rng(m + n)
    if kind == "cluster":
        s = 1.0 - 1e-4 * rng.random(n)
    elif kind == "identity-like":
        s = np.ones(n)
    else:
        s = np.concatenate([np.full(n // 2, 3.0), 1.0 + 1e-5 * rng.random(n - n // 2)])
    A = si.with_spectrum(m, n, np.sort(s)[::-1], m - n).astype(np.float32).astype(np.float64)
    if which == "gesdd":
        info, sw, U, S, VT, took, _ = gesdd(ctx, A, "f32")
        assert took[16] + took[17] == 1 and took[19] == took[20] == took[10] == 0        # Cholesky-QR, then Jacobi on the clustered R^T
        extra = E32 * _cond_of(A) * np.sqrt(n)
    else:
        info, sw, U, S, VT, took, _ = gesvdj(ctx, A, "f32")
        assert _only(took, SWEEP_SLOTS) == expected_sweep_driver(m, n, "f32", True)
        extra = 0.0
    print((m, n), kind, which, "counters", took, "sweeps", sw)
    assert info == 0 and 0 < sw < 60
    check_svd(A, U, S, VT, "f32", u_extra=extra)
