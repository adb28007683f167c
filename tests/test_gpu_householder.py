"""-m gpu: the block-Householder kernels under BQRRP, HQRRP, ABRIK and the BLAS-3 geqrf (csrc/house.hip, csrc/qr_blk.hip), called
through the C ABI in fp64 AND fp32 and compared with float64 LAPACK / numpy on the same (upcast) values:

  orhr_col      Householder reconstruction: sign-modified LU of the top block (LDS panel kernel for n <= 32, the cooperative lunp_blk
                for n <= 2048, the panel loop beyond), the solve below it and the T factor -- against LAPACK's dorhr_col, D exactly
  gemqrt        Left/Trans against the LAPACK blocks applied one at a time; Right/NoTrans against C (I - V T V^T); the head / tail split
  larft         against the dlarft recurrence, zero tau included (H = I: a zero row and column of T)
  tau_from_t, row_sign, vrows_explicit   exact
  end to end    a tall matrix with an exactly zero row gives an exact +0 pivot in the top block of Q: geqrf, geqrf_q, BQRRP (cholqr)
                and HQRRP (qr_type 2) must return LAPACK's signs (dlaorhr_col_getrfnp: D(i) = -sign(a_ii), -1 for +0.0)

Tolerances are multiples of the working precision's eps; every one of them is far below the O(1) change a dropped block, a transposed
T or a wrong sign makes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PRECS = ["f64", "f32"]
EPS64 = np.finfo(np.float64).eps
EPS32 = np.finfo(np.float32).eps
SENT = 7.25                                        # guard value of rows / columns a call must not touch


def _d():
    from randlapack_amd import device

    return device


def _prec(p):
    import torch

    return (np.float64, torch.float64, EPS64) if p == "f64" else (np.float32, torch.float32, EPS32)


def _fn(ctx, name, p):
    return getattr(ctx.lib, f"rlhip_{name}_{p}")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _maxerr(got, ref):
    """max |got - ref| / max(1, max |ref|), in float64"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0


def _check(got, ref, eps, units, what):
    e = _maxerr(got, ref)
    assert e <= units * eps, f"{what}: error {e / eps:.1f} eps > {units:.1f} eps"


def _orth(m, n, rng, npdt, zero_row=None):
    """m x n orthonormal columns in npdt; zero_row: that row exactly zero (the other rows are orthonormal columns of one row fewer)"""
    if zero_row is None:
        return np.linalg.qr(rng.standard_normal((m, n)))[0].astype(npdt)
    Q = np.zeros((m, n))
    rows = [i for i in range(m) if i != zero_row]
    Q[rows] = np.linalg.qr(rng.standard_normal((m - 1, n)))[0]
    return Q.astype(npdt)


def _wy(orc, m, k, nb, rng, npdt):
    """LAPACK's compact-WY blocks (V m x k unit lower, T nb x k) of a random orthonormal m x k, rounded to npdt"""
    Q = np.linalg.qr(rng.standard_normal((m, k)))[0]
    info, Ao, To, _ = orc.lapack_orhr_col(Q, nb)
    assert info == 0
    V = (np.tril(Ao, -1) + np.eye(m, k)).astype(npdt)
    return V, To.astype(npdt)


def _apply_lt_ref(V, Tm, nb, C):
    """C <- Q^T C with Q = H_1 ... H_k in blocks of nb: block b at a time, (I - V_b T_b^T V_b^T), float64, O(m n k)"""
    V, Tm, C = V.astype(np.float64), Tm.astype(np.float64), C.astype(np.float64).copy()
    k = V.shape[1]
    for j0 in range(0, k, nb):
        jb = min(nb, k - j0)
        Vb = V[j0:, j0:j0 + jb]
        C[j0:] -= Vb @ (Tm[:jb, j0:j0 + jb].T @ (Vb.T @ C[j0:]))
    return C


# ---------------------------------------------------------------------------------------------------------------------------------------
# orhr_col
# ---------------------------------------------------------------------------------------------------------------------------------------
def _run_orhr(ctx, orc, p, Q, nb, lda=None, ldt=None):
    d = _d()
    npdt, tdt, eps = _prec(p)
    m, n = Q.shape
    lda = lda or m
    nbe = min(nb, n)
    ldt = ldt or nbe
    buf = np.full((lda, n), SENT, dtype=npdt)
    buf[:m] = Q
    Ad = d.cm_from_numpy(buf)
    Td = d.cm_from_numpy(np.full((ldt, n), SENT, dtype=npdt))
    import torch

    Dd = torch.full((n,), SENT, dtype=tdt, device="cuda")
    lu0 = ctx.path_count(9)
    assert _fn(ctx, "orhr_col", p)(ctx.h, m, n, nb, Ad.data_ptr(), lda, Td.data_ptr(), ldt, Dd.data_ptr()) == 0
    ctx.sync()
    blk = ctx.path_count(9) - lu0
    info, Ao, To, Do = orc.lapack_orhr_col(Q.astype(np.float64), nbe)
    assert info == 0
    A_out, T_out = d.cm_to_numpy(Ad), d.cm_to_numpy(Td)
    return dict(A=A_out, T=T_out, D=Dd.cpu().numpy(), Ao=Ao, To=To, Do=Do, blk=blk, eps=eps)


def _orhr_asserts(r, m, n, nbe, what):
    eps = r["eps"]
    np.testing.assert_array_equal(r["D"], r["Do"], err_msg=f"{what}: sign vector D differs from dorhr_col's")
    units = 64 * np.sqrt(n)
    _check(np.tril(r["A"][:m], -1), np.tril(r["Ao"], -1), eps, units, f"{what}: V")
    _check(np.triu(r["A"][:n]), np.triu(r["Ao"][:n]), eps, units, f"{what}: S-modified U on and above the diagonal")
    _check(r["T"][:nbe], r["To"], eps, units, f"{what}: T")


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,nb", [
    (40, 1, 1), (200, 7, 3), (300, 31, 40), (500, 32, 32), (32, 32, 5),          # LDS panel kernel (n <= 32); nb > n clamps
    (1000, 100, 7), (64, 64, 64), (600, 300, 1), (2100, 2048, 256),              # cooperative lunp_blk (33 <= n <= 2048); m == n
    (2600, 2080, 256),                                                            # n > 2048: 32-column panels + trsm + GEMM
])
def test_orhr_col_matches_dorhr_col(ctx, orc, p, m, n, nb):
    npdt = _prec(p)[0]
    rng = np.random.default_rng(m + 3 * n + nb)
    r = _run_orhr(ctx, orc, p, _orth(m, n, rng, npdt), nb)
    assert r["blk"] == (1 if 32 < n <= 2048 else 0), "route of the sign-modified LU"
    _orhr_asserts(r, m, n, min(nb, n), f"{p} {m}x{n} nb={nb}")


@pytest.mark.parametrize("p", PRECS)
def test_orhr_col_leading_dimensions_leave_guard_rows(ctx, orc, p):
    npdt = _prec(p)[0]
    m, n, nb, lda, ldt = 300, 100, 40, 311, 45
    r = _run_orhr(ctx, orc, p, _orth(m, n, np.random.default_rng(4), npdt), nb, lda=lda, ldt=ldt)
    _orhr_asserts(r, m, n, nb, f"{p} lda={lda} ldt={ldt}")
    assert np.all(r["A"][m:] == npdt(SENT)) and np.all(r["T"][nb:] == npdt(SENT)), "rows past m of A / past nb of T were written"


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,zero_row", [(200, 20, 0), (200, 20, 5), (500, 100, 0), (500, 100, 5), (121, 120, 0), (2600, 2080, 5)])
def test_orhr_col_zero_row_gives_lapack_signs(ctx, orc, p, m, n, zero_row):
    """an exactly zero row in the top block -> an exact +0 pivot: dlaorhr_col_getrfnp takes D = -sign(+0) = -1"""
    npdt = _prec(p)[0]
    Q = _orth(m, n, np.random.default_rng(m + n + zero_row), npdt, zero_row=zero_row)
    r = _run_orhr(ctx, orc, p, Q, 32)
    _orhr_asserts(r, m, n, 32, f"{p} {m}x{n} zero row {zero_row}")


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n", [(4, 4), (40, 4), (40, 40)])
@pytest.mark.parametrize("neg", [False, True])
def test_orhr_col_permuted_identity(ctx, orc, p, m, n, neg):
    """Q = I(:, [2 1 3 4 ...]): pivots +0.0 (LAPACK: D = -1) and, for -Q, -0.0 (D = +1)"""
    npdt = _prec(p)[0]
    perm = [1, 0] + list(range(2, n))
    Q = np.eye(m, dtype=npdt)[:, perm]
    if neg:
        Q = -Q
    r = _run_orhr(ctx, orc, p, Q, 32)
    assert r["Do"][0] == (1 if neg else -1)                                          # the oracle's LAPACK itself
    if (m, n) == (4, 4) and not neg:
        np.testing.assert_array_equal(r["Do"], [-1, 1, -1, -1])
    _orhr_asserts(r, m, n, min(32, n), f"{p} permuted identity {m}x{n} neg={neg}")


@pytest.mark.parametrize("p", PRECS)
def test_orhr_col_argument_codes_write_nothing(ctx, p):
    import torch

    d = _d()
    npdt, tdt, _ = _prec(p)
    m, n = 50, 20
    Ad = d.cm_from_numpy(np.full((m, n + 40), SENT, dtype=npdt))
    Td = d.cm_from_numpy(np.full((40, n + 40), SENT, dtype=npdt))
    Dd = torch.full((n + 40,), SENT, dtype=tdt, device="cuda")
    f = _fn(ctx, "orhr_col", p)
    for args, code in [((m, m + 1, 8, m, 8), -3), ((m, n, 0, m, 8), -4), ((m, n, 8, m - 1, 8), -6), ((m, n, 8, m, 7), -8),
                       ((m, n, 30, m, 19), -8)]:           # nb clamps to n = 20 first: ldt 19 is still short
        mm, nn, nb, lda, ldt = args
        assert f(ctx.h, mm, nn, nb, Ad.data_ptr(), lda, Td.data_ptr(), ldt, Dd.data_ptr()) == code, args
    ctx.sync()
    assert torch.all(Ad == SENT) and torch.all(Td == SENT) and torch.all(Dd == SENT)


# ---------------------------------------------------------------------------------------------------------------------------------------
# gemqrt, Left / Trans
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,k,nb,ldc", [
    (300, 9, 5, 16, 300),            # k < nb
    (500, 33, 100, 32, 500),         # k % nb = 4: ragged last block
    (128, 7, 128, 40, 128),          # k == m: the last block has no rows below it
    (400, 1, 64, 16, 400),           # n = 1
    (350, 20, 50, 24, 361),          # ldc > m: guard rows
])
def test_gemqrt_lt_blockwise_lapack(ctx, orc, p, m, n, k, nb, ldc):
    d = _d()
    npdt, _, eps = _prec(p)
    rng = np.random.default_rng(m + n + k + nb)
    V, Tm = _wy(orc, m, k, nb, rng, npdt)
    C0 = rng.standard_normal((m, n)).astype(npdt)
    buf = np.full((ldc, n), SENT, dtype=npdt)
    buf[:m] = C0
    Cd = d.cm_from_numpy(buf)
    Vd, Td = d.cm_from_numpy(V), d.cm_from_numpy(Tm)
    assert _fn(ctx, "gemqrt", p)(ctx.h, b"L", b"T", m, n, k, nb, Vd.data_ptr(), m, Td.data_ptr(), Tm.shape[0], Cd.data_ptr(), ldc) == 0
    got = d.cm_to_numpy(Cd)
    _check(got[:m], _apply_lt_ref(V, Tm, min(nb, k), C0), eps, 32 * np.sqrt(m), f"{p} gemqrt L/T {m}x{n} k={k} nb={nb}")
    assert np.all(got[m:] == npdt(SENT)), "rows past m of C were written"


@pytest.mark.parametrize("p", PRECS)
def test_gemqrt_lt_stream_k_shape(ctx, orc, p):
    """C2 -= V2 W2 at 39744 x n x 256 passes the persistent stream-K kernel's work gate (path counter 0 / 1)"""
    d = _d()
    npdt, _, eps = _prec(p)
    m, n, k = 40000, (1024 if p == "f64" else 2048), 256
    rng = np.random.default_rng(17)
    V, Tm = _wy(orc, m, k, k, rng, npdt)
    C0 = rng.standard_normal((m, n)).astype(npdt)
    Cd, Vd, Td = d.cm_from_numpy(C0), d.cm_from_numpy(V), d.cm_from_numpy(Tm)
    sk = 0 if p == "f64" else 1
    before = ctx.path_count(sk)
    assert _fn(ctx, "gemqrt", p)(ctx.h, b"L", b"T", m, n, k, k, Vd.data_ptr(), m, Td.data_ptr(), k, Cd.data_ptr(), m) == 0
    ctx.sync()
    assert ctx.path_count(sk) > before, "the persistent stream-K GEMM did not run"
    _check(d.cm_to_numpy(Cd), _apply_lt_ref(V, Tm, k, C0), eps, 32 * np.sqrt(m), f"{p} gemqrt L/T stream-K shape")


# ---------------------------------------------------------------------------------------------------------------------------------------
# gemqrt, Right / NoTrans (HQRRP's update of the sketching matrix)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,k,nb", [(50, 300, 40, 40), (7, 64, 64, 64), (200, 1000, 1, 5), (33, 500, 100, 128)])
def test_gemqrt_rn_matches_c_times_h(ctx, orc, p, m, n, k, nb):
    d = _d()
    npdt, _, eps = _prec(p)
    rng = np.random.default_rng(m + n + k)
    V, Tm = _wy(orc, n, k, k, rng, npdt)
    ldt = k
    C0 = rng.standard_normal((m, n)).astype(npdt)
    Cd, Vd, Td = d.cm_from_numpy(C0), d.cm_from_numpy(V), d.cm_from_numpy(Tm)
    assert _fn(ctx, "gemqrt", p)(ctx.h, b"R", b"N", m, n, k, nb, Vd.data_ptr(), n, Td.data_ptr(), ldt, Cd.data_ptr(), m) == 0
    V64, T64, C64 = V.astype(np.float64), Tm.astype(np.float64), C0.astype(np.float64)
    ref = C64 - ((C64 @ V64) @ T64) @ V64.T
    _check(d.cm_to_numpy(Cd), ref, eps, 32 * np.sqrt(n), f"{p} gemqrt R/N {m}x{n} k={k}")


@pytest.mark.parametrize("p", PRECS)
def test_gemqrt_argument_codes_leave_c(ctx, orc, p):
    d = _d()
    npdt = _prec(p)[0]
    m, n, k = 30, 80, 20
    rng = np.random.default_rng(3)
    V, Tm = _wy(orc, n, k, k, rng, npdt)
    C0 = rng.standard_normal((m, n)).astype(npdt)
    Cd, Vd, Td = d.cm_from_numpy(C0), d.cm_from_numpy(V), d.cm_from_numpy(Tm)
    f = _fn(ctx, "gemqrt", p)
    assert f(ctx.h, b"R", b"N", m, n, k, k - 1, Vd.data_ptr(), n, Td.data_ptr(), k, Cd.data_ptr(), m) == -7    # one block on this side
    assert f(ctx.h, b"L", b"N", n, m, k, k, Vd.data_ptr(), n, Td.data_ptr(), k, Cd.data_ptr(), n) == -3
    assert f(ctx.h, b"R", b"T", m, n, k, k, Vd.data_ptr(), n, Td.data_ptr(), k, Cd.data_ptr(), m) == -2
    ctx.sync()
    assert np.array_equal(_bits(d.cm_to_numpy(Cd)), _bits(C0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# gemqrt_head + gemqrt_tail (BQRRP's look-ahead split)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _head_tail(ctx, p, V, Tm, C0, ldc, avoid):
    import torch

    d = _d()
    npdt, tdt, _ = _prec(p)
    m, k = V.shape
    n = C0.shape[1]
    buf = np.full((ldc, n), SENT, dtype=npdt)
    buf[:m] = C0
    Cd, Vd, Td = d.cm_from_numpy(buf), d.cm_from_numpy(V), d.cm_from_numpy(Tm)
    W2 = torch.full((n, k), SENT, dtype=tdt, device="cuda")                   # k x n, ld k
    keep = ctx.lib.rlhip_avoid_persistent(ctx.h, int(avoid))
    try:
        assert _fn(ctx, "gemqrt_head", p)(ctx.h, m, n, k, Vd.data_ptr(), m, Td.data_ptr(), k, Cd.data_ptr(), ldc, W2.data_ptr()) == 0
        C_head = d.cm_to_numpy(Cd)
        assert _fn(ctx, "gemqrt_tail", p)(ctx.h, m, n, k, Vd.data_ptr(), m, W2.data_ptr(), Cd.data_ptr(), ldc) == 0
        C_tail = d.cm_to_numpy(Cd)
        Cf = d.cm_from_numpy(buf)
        assert _fn(ctx, "gemqrt", p)(ctx.h, b"L", b"T", m, n, k, k + 3, Vd.data_ptr(), m, Td.data_ptr(), k, Cf.data_ptr(), ldc) == 0
        C_full = d.cm_to_numpy(Cf)
    finally:
        ctx.lib.rlhip_avoid_persistent(ctx.h, keep)
    return C_head, W2.cpu().numpy().T.copy(), C_tail, C_full


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n,k,ldc", [(600, 50, 40, 600), (1000, 129, 128, 1003), (64, 16, 64, 64)])
def test_gemqrt_head_tail_split(ctx, orc, p, m, n, k, ldc):
    npdt, _, eps = _prec(p)
    rng = np.random.default_rng(m + n + k)
    V, Tm = _wy(orc, m, k, k, rng, npdt)
    C0 = rng.standard_normal((m, n)).astype(npdt)
    C_head, W2, C_tail, C_full = _head_tail(ctx, p, V, Tm, C0, ldc, avoid=True)
    ref = _apply_lt_ref(V, Tm, k, C0)
    units = 32 * np.sqrt(m)
    # head: rows k.. untouched, W2 = T^T V^T C, rows 0..k-1 final
    assert np.array_equal(_bits(C_head[k:m]), _bits(C0[k:])), "gemqrt_head wrote rows below the block"
    V64 = V.astype(np.float64)
    _check(W2, Tm.astype(np.float64).T @ (V64.T @ C0.astype(np.float64)), eps, units, f"{p} W2")
    _check(C_head[:k], ref[:k], eps, units, f"{p} head rows")
    # tail: rows 0..k-1 untouched, all rows final
    assert np.array_equal(_bits(C_tail[:k]), _bits(C_head[:k])), "gemqrt_tail wrote the block rows"
    _check(C_tail[:m], ref, eps, units, f"{p} head + tail")
    # with the persistent kernel kept out, head + tail is gemqrt_lt with nb >= k bit for bit; nothing written past row m
    assert np.array_equal(_bits(C_tail), _bits(C_full)), "head + tail differs from gemqrt_lt (avoid_persistent on)"
    assert np.all(C_tail[m:] == npdt(SENT))


@pytest.mark.parametrize("p", PRECS)
def test_gemqrt_head_tail_stream_k_shape(ctx, orc, p):
    """where gemqrt_lt's C2 -= V2 W2 goes to the persistent kernel and the tail does not: equal to rounding, not bitwise"""
    npdt, _, eps = _prec(p)
    m, n, k = 40000, (1024 if p == "f64" else 2048), 256
    rng = np.random.default_rng(23)
    V, Tm = _wy(orc, m, k, k, rng, npdt)
    C0 = rng.standard_normal((m, n)).astype(npdt)
    sk = 0 if p == "f64" else 1
    before = ctx.path_count(sk)
    _, _, C_tail, C_full = _head_tail(ctx, p, V, Tm, C0, m, avoid=False)
    assert ctx.path_count(sk) > before, "the persistent stream-K GEMM did not run"
    units = 32 * np.sqrt(m)
    _check(C_tail, C_full, eps, units, f"{p} head + tail vs gemqrt_lt")
    _check(C_tail, _apply_lt_ref(V, Tm, k, C0), eps, units, f"{p} head + tail vs reference")


# ---------------------------------------------------------------------------------------------------------------------------------------
# larft
# ---------------------------------------------------------------------------------------------------------------------------------------
def _larft_ref(V, tau):
    """dlarft (Forward, Columnwise) in float64: tau(i) == 0 -> column i of T zero (and so its row)"""
    m, k = V.shape
    T = np.zeros((k, k))
    for i in range(k):
        if tau[i] == 0:
            continue
        T[:i, i] = -tau[i] * (T[:i, :i] @ (V[:, :i].T @ V[:, i]))
        T[i, i] = tau[i]
    return T


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,k,zeros", [(50, 1, ()), (50, 1, (0,)), (40, 40, ()), (300, 40, ()), (600, 256, ()),
                                       (300, 40, (7,)), (300, 40, (3, 20)), (600, 256, (0, 130))])
def test_larft_matches_recurrence(ctx, p, m, k, zeros):
    import scipy.linalg as sl
    import torch

    d = _d()
    npdt, tdt, eps = _prec(p)
    rng = np.random.default_rng(m + k + len(zeros))
    (qr_, tau), _ = sl.qr(rng.standard_normal((m, k)), mode="raw")
    tau = tau.astype(npdt)
    tau[list(zeros)] = 0
    V = (np.tril(qr_, -1)[:, :k] + np.eye(m, k)).astype(npdt)
    ldt = k + 2
    Vd = d.cm_from_numpy(np.where(np.tri(m, k, -1, dtype=bool), V, npdt(SENT)))       # only the strictly lower part may be read
    Td = d.cm_from_numpy(np.full((ldt, k), SENT, dtype=npdt))
    assert _fn(ctx, "larft", p)(ctx.h, m, k, Vd.data_ptr(), m, torch.from_numpy(tau).to(tdt).cuda().data_ptr(), Td.data_ptr(), ldt) == 0
    Tfull = d.cm_to_numpy(Td)
    assert np.all(Tfull[k:] == npdt(SENT))
    Tg = Tfull[:k].astype(np.float64)
    assert np.all(np.isfinite(Tg)), f"{p}: T is not finite at {np.argwhere(~np.isfinite(Tg))[:4].tolist()}"
    V64 = V.astype(np.float64)
    Tr = _larft_ref(V64, tau.astype(np.float64))
    units = 32 * np.sqrt(m)
    _check(np.triu(Tg), Tr, eps, units, f"{p} larft T")
    assert np.all(np.tril(Tg, -1) == 0), "strictly lower part of T not zero"
    for j in zeros:
        assert np.all(Tg[j] == 0) and np.all(Tg[:, j] == 0), f"{p}: row / column {j} of T (tau = 0) is not exactly zero"
    # the block reflector itself: I - V T V^T = H_1 ... H_k applied to a few vectors
    X = rng.standard_normal((m, 5))
    ref = X.copy()
    for i in reversed(range(k)):
        ref -= tau[i].astype(np.float64) * np.outer(V64[:, i], V64[:, i] @ ref)
    _check(X - V64 @ (Tg @ (V64.T @ X)), ref, eps, units, f"{p} I - V T V^T")


# ---------------------------------------------------------------------------------------------------------------------------------------
# tau_from_t, row_sign, vrows_explicit: exact
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
def test_tau_from_t_rank_deficient_last_block(ctx, p):
    """k < n and nb not dividing k: BQRRP's rank-deficient last block"""
    import torch

    d = _d()
    npdt, tdt, _ = _prec(p)
    n, nb, k, ldt = 64, 16, 50, 19
    Tm = np.random.default_rng(1).standard_normal((ldt, n)).astype(npdt)
    tau = torch.full((n,), SENT, dtype=tdt, device="cuda")
    assert _fn(ctx, "tau_from_t", p)(ctx.h, k, nb, d.cm_from_numpy(Tm).data_ptr(), ldt, tau.data_ptr()) == 0
    got = tau.cpu().numpy()
    assert np.array_equal(_bits(got[:k]), _bits(np.array([Tm[i % nb, i] for i in range(k)], dtype=npdt)))
    assert np.all(got[k:] == npdt(SENT))


@pytest.mark.parametrize("p", PRECS)
def test_row_sign_scales_only_the_upper_triangle(ctx, p):
    import torch

    d = _d()
    npdt, tdt, _ = _prec(p)
    n, ldr = 77, 80
    rng = np.random.default_rng(2)
    R = rng.standard_normal((ldr, n + 1)).astype(npdt)
    D = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(npdt)
    Rd = d.cm_from_numpy(R)
    assert _fn(ctx, "row_sign", p)(ctx.h, n, Rd.data_ptr(), ldr, torch.from_numpy(D).cuda().data_ptr()) == 0
    got = d.cm_to_numpy(Rd)
    ref = R.copy()
    up = np.triu(np.ones((n, n), dtype=bool))
    ref[:n, :n] = np.where(up, D[:, None] * R[:n, :n], R[:n, :n])
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("br,toff,tcnt,ldo", [(40, 0, 10, 13), (40, 30, 10, 12), (40, 17, 1, 4), (33, 0, 33, 35)])
def test_vrows_explicit(ctx, p, br, toff, tcnt, ldo):
    d = _d()
    npdt = _prec(p)[0]
    ldv = br + 3
    Vtop = np.random.default_rng(br + toff).standard_normal((ldv, br)).astype(npdt)     # upper part and guard rows: must not show
    out = d.cm_from_numpy(np.full((ldo, br), SENT, dtype=npdt))
    assert _fn(ctx, "vrows_explicit", p)(ctx.h, br, toff, tcnt, d.cm_from_numpy(Vtop).data_ptr(), ldv, out.data_ptr(), ldo) == 0
    got = d.cm_to_numpy(out)
    L = (np.tril(Vtop[:br], -1) + np.eye(br)).astype(npdt)
    assert np.array_equal(_bits(got[:tcnt]), _bits(L[toff:toff + tcnt]))
    assert np.all(got[tcnt:] == npdt(SENT))


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: a zero row -> an exact +0 pivot in the top block of Q -> LAPACK's signs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _zero_row_gauss(m, n, row, seed, npdt):
    A = np.random.default_rng(seed).standard_normal((m, n))
    A[row] = 0
    return A.astype(npdt)


def _signed(got, ref, eps, units, what):
    """a signed comparison; the message also gives the error after aligning row signs (the rounding part of a sign mismatch)"""
    e = _maxerr(got, ref)
    if e > units * eps:
        s = np.where(np.sum(got.astype(np.float64) * ref, axis=1) < 0, -1.0, 1.0)[:, None] if got.ndim == 2 else np.sign(got) * np.sign(ref)
        ea = _maxerr(s * got, ref)
        bad = np.argwhere(np.abs(got - ref) > units * eps * max(1.0, np.abs(ref).max()))[:6].tolist()
        raise AssertionError(f"{what}: error {e / eps:.1f} eps > {units:.1f} eps (after aligning signs {ea / eps:.1f} eps); first at {bad}")


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("row", [0, 5])
def test_geqrf_cholqr_route_zero_row_signs(ctx, p, row):
    import scipy.linalg.lapack as ll
    import torch

    d = _d()
    npdt, tdt, eps = _prec(p)
    m, n = 20000, 64
    A = _zero_row_gauss(m, n, row, 100 + row, npdt)
    Ad = d.cm_from_numpy(A)
    tau = torch.zeros(n, dtype=tdt, device="cuda")
    lu0 = ctx.path_count(9)
    assert _fn(ctx, "geqrf", p)(ctx.h, m, n, Ad.data_ptr(), m, tau.data_ptr()) == 0
    ctx.sync()
    assert ctx.path_count(9) == lu0 + 1, "geqrf did not take the Cholesky-QR + orhr_col route"
    qr_ref, tau_ref, _, _ = ll.dgeqrf(A.astype(np.float64))
    got = d.cm_to_numpy(Ad).astype(np.float64)
    units = 4 * np.sqrt(m)
    _signed(np.triu(got[:n]), np.triu(qr_ref[:n]), eps, units, f"{p} R")
    _signed(tau.cpu().numpy(), tau_ref, eps, units, f"{p} tau")
    Qg = ll.dorgqr(np.asfortranarray(got[:, :n]), tau.cpu().numpy().astype(np.float64))[0]
    Qr = ll.dorgqr(qr_ref[:, :n], tau_ref)[0]
    _signed(Qg.T, Qr.T, eps, units, f"{p} Q (columns)")


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("row", [0, 5])
def test_geqrf_q_zero_row_signs(ctx, p, row):
    import scipy.linalg.lapack as ll

    d = _d()
    npdt, tdt, eps = _prec(p)
    m, n = 20000, 64
    A = _zero_row_gauss(m, n, row, 200 + row, npdt)
    Ad = d.cm_from_numpy(A)
    Rd = d.cm_zeros(n, n, dtype=tdt)
    assert _fn(ctx, "geqrf_q", p)(ctx.h, m, n, Ad.data_ptr(), m, Rd.data_ptr(), n) == 0
    qr_ref, tau_ref, _, _ = ll.dgeqrf(A.astype(np.float64))
    Qr = ll.dorgqr(qr_ref[:, :n], tau_ref)[0]
    units = 4 * np.sqrt(m)
    _signed(d.cm_to_numpy(Rd), np.triu(qr_ref[:n]), eps, units, f"{p} R")
    _signed(d.cm_to_numpy(Ad).T, Qr.T, eps, units, f"{p} Q (columns)")


def _graded(m, n, rng, decades):
    return rng.standard_normal((m, n)) * np.logspace(0, -decades, n)[rng.permutation(n)]


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("row", [0, 5])
def test_bqrrp_cholqr_zero_row_vs_oracle(ctx, orc, p, row):
    d = _d()
    npdt, _, eps = _prec(p)
    m, n, b = 2048, 512, 128
    rng = np.random.default_rng(40 + row)
    A = _graded(m, n, rng, 4.0)
    A[row] = 0
    A = A.astype(npdt)
    Ad = d.cm_from_numpy(A)
    r = d.drv_bqrrp(ctx, Ad, m, n, b, 1.0, want_sketch=True, key=(13, 0), qrcp_wide=0, qr_tall=1, apply_trans_q=1)
    assert r["rc"] == 0
    sk = d.cm_to_numpy(r["sketch"])
    o = orc.bqrrp(A, b, 1.0, qrcp_wide=0, qr_tall=1, apply_trans_q=1, sketch=sk)                    # the same precision's oracle
    o64 = o if p == "f64" else orc.bqrrp(A.astype(np.float64), b, 1.0, qrcp_wide=0, qr_tall=1, apply_trans_q=1, sketch=sk.astype(np.float64),
                                         tol=float(eps))
    J = r["J"].cpu().numpy()
    assert r["rank"] == o["rank"] == n
    np.testing.assert_array_equal(J, o["J"])
    np.testing.assert_array_equal(J, o64["J"])
    F = d.cm_to_numpy(Ad).astype(np.float64)
    Ro = np.triu(o64["A"])[:n]
    # BQRRP's Cholesky-QR panel is A_panel R_sk^-1 R_chol^-1: the zero row comes out of two triangular solves as a zero whose SIGN BIT is
    # that of the solve's arithmetic (LAPACK's substitution: -0.0 after a negative diagonal; the MFMA solve: +0.0), and D = -sign(pivot)
    # reads that bit.  So the one row of R at the zero pivot may carry the other sign (the same factorization, the other reflector);
    # every other row is signed like the oracle's.
    s = np.where(np.sum(np.triu(F)[:n] * Ro, axis=1) < 0, -1.0, 1.0)
    assert set(np.flatnonzero(s < 0).tolist()) <= {row}, f"{p}: rows of R with the other sign: {np.flatnonzero(s < 0).tolist()}"
    err = np.linalg.norm(s[:, None] * np.triu(F)[:n] - Ro) / np.linalg.norm(Ro)
    assert err <= eps ** 0.6, f"{p}: R differs from the oracle's by {err:.2e}"
    keep = s > 0
    tau = r["tau"].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(tau[keep], o64["tau"][keep], atol=eps ** 0.5, rtol=0)
    Q = orc.ungqr(F, tau)
    A64 = A.astype(np.float64)
    assert np.linalg.norm(A64[:, J - 1] - Q @ np.triu(F)[:n]) <= 32 * np.sqrt(n) * eps * np.linalg.norm(A64)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 32 * np.sqrt(n) * eps * np.sqrt(n)


@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("row", [0, 5])
def test_hqrrp_cholqr_zero_row_vs_oracle(ctx, orc, p, row):
    d = _d()
    npdt, _, eps = _prec(p)
    m, n, nb, pp = 1200, 300, 64, 8
    rng = np.random.default_rng(60 + row)
    A = _graded(m, n, rng, 4.0)
    A[row] = 0
    A = A.astype(npdt)
    Ad = d.cm_from_numpy(A)
    r = d.drv_hqrrp(ctx, Ad, m, n, nb, pp, 0, 2, key=(7, 0), want_G=True)
    o = orc.hqrrp(A.astype(np.float64), nb, pp, 0, 2, key=(7, 0), G=d.cm_to_numpy(r["G"]).astype(np.float64))
    assert r["rc"] == o["rc"] == 0
    np.testing.assert_array_equal(r["J"].cpu().numpy(), o["J"])
    F = d.cm_to_numpy(Ad).astype(np.float64)
    Ro = np.triu(o["A"])[:n]
    err = np.linalg.norm(np.triu(F)[:n] - Ro) / np.linalg.norm(Ro)
    assert err <= eps ** 0.55, f"{p}: R differs from the oracle's by {err:.2e} (row 0 of R: {F[0, :3]} vs {Ro[0, :3]})"
    np.testing.assert_allclose(r["tau"].cpu().numpy(), o["tau"], atol=eps ** 0.5, rtol=0)
