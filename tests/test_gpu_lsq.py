"""The matrix-vector layer, pcg_saddle and the sketched least-squares preconditioners on the device (randlapack_amd/csrc/lsq.hip,
include/RandLAPACK_amd/rl_determiter.hh, rl_preconditioners.hh, rl_lstsq.hh) in fp64 and fp32: the kernels exactly on small integers on
every route, the argument codes, the solver step by step against the numpy model (tests/_lsq_model.py), convergence with the model as the
yardstick, the preconditioner by the reference's own checks (test/comps/test_preconditioners.cc), the edges, and sap_lstsq."""

import numpy as np
import pytest

import _lsq_model as lm

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
FUSED_MAX = {"f64": 1024, "f32": 2048}          # RLHIP_NORMAL_FUSED_MAX_N_F64 / _F32 (include/rlhip.h)
FUSED_DEFAULT_MAX = {"f64": 1024, "f32": 256}  # RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_*: the widest n that takes the one-pass kernel unasked
NAN = float("nan")


def _mat(a, T):
    """(rows, cols) numpy -> column-major device tensor (cols, rows)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=T).T)).to("cuda:0")


def _vec(a, T, pad=0, fill=99.0):
    import torch

    v = np.concatenate([np.asarray(a, dtype=T).ravel(), np.full(pad, fill, dtype=T)])
    return torch.from_numpy(v).to("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _counts(ctx):
    return [ctx.lsq_path_count(i) for i in (46, 47, 48, 49)]


# ---------------------------------------------------------------------------------------------------
# 1. gemv and the normal matvec, exactly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n_kind", [1, 3, 33, 64, 100, "limit", "limit+1"])
def test_matvec_kernels_exact(ctx, n_kind, prec):
    """A and d in {-1, 0, 1}, delta in {0, 1/2}: every sum is an integer or a half-integer below 2^23 in absolute value (checked below on
    the data), so either precision must give numpy's float64 result bit for bit, whatever the order of summation.  Rows m .. lda - 1 of A
    hold NaN (never read), outputs sit in longer buffers whose tail must survive."""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    n = {"limit": FUSED_MAX[prec], "limit+1": FUSED_MAX[prec] + 1}.get(n_kind, n_kind)
    for m in (1, 15, 16, 17, 255, 257, 4099):
        assert m * n < 2 ** 24
        rng = np.random.default_rng(100000 * n + m)
        lda = m + 5
        Af = np.full((lda, n), NAN)
        Af[:m] = rng.integers(-1, 2, size=(m, n))
        A = Af[:m]
        d = rng.integers(-1, 2, size=n).astype(np.float64)
        xm = rng.integers(-1, 2, size=m).astype(np.float64)
        y0n, y0m = rng.integers(-3, 4, size=n).astype(np.float64), rng.integers(-3, 4, size=m).astype(np.float64)
        Ad, dd, xmd = _mat(Af, T), _vec(d, T), _vec(xm, T)
        # ---- gemv
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (2.0, -0.5)):
            before = _counts(ctx)
            yN = _vec(np.full(m, NAN) if beta == 0.0 else y0m, T, pad=3)
            dev.gemv(ctx, "N", m, n, alpha, Ad, dd, beta, yN, lda=lda)
            want = alpha * (A @ d) + (beta * y0m if beta != 0.0 else 0.0)
            got = _np(yN)
            assert np.array_equal(got[:m], want.astype(T)) and np.all(got[m:] == 99.0), ("N", m, n, alpha, beta)
            yT = _vec(np.full(n, NAN) if beta == 0.0 else y0n, T, pad=3)
            dev.gemv(ctx, "T", m, n, alpha, Ad, xmd, beta, yT, lda=lda)
            want = alpha * (A.T @ xm) + (beta * y0n if beta != 0.0 else 0.0)
            got = _np(yT)
            assert np.array_equal(got[:n], want.astype(T)) and np.all(got[n:] == 99.0), ("T", m, n, alpha, beta)
            assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 0, 1, 1]
        # ---- the normal matvec
        t_want = A @ d
        for delta in (0.0, 0.5):
            q_want = A.T @ t_want + delta * d
            dq_want = float(d @ q_want)
            assert max(np.sum(np.abs(d * q_want)), np.max(np.abs(q_want)) if n else 0.0, n) < 2 ** 23
            first = None
            # option lsq_normal_fused: 1 the one-pass kernel wherever n is within its limit, 0 the two gemv calls, -1 the measured default
            for force, max_wg in ((1, 0), (1, 1), (1, 2), (1, 3), (0, 0), (-1, 0)):
                ctx.set_option("lsq_normal_fused", force)
                fused = n <= (FUSED_DEFAULT_MAX[prec] if force < 0 else FUSED_MAX[prec] if force else 0)
                before = _counts(ctx)
                q, t = _vec(np.full(n, NAN), T, pad=3), _vec(np.full(m, NAN), T, pad=3)
                dq = dev.normal_matvec(ctx, m, n, Ad, dd, delta, q, t=t, want_dq=True, max_wg=max_wg, lda=lda)
                gq, gt = _np(q), _np(t)
                assert np.array_equal(gq[:n], q_want.astype(T)) and np.all(gq[n:] == 99.0), (m, n, delta, force, max_wg)
                assert np.array_equal(gt[:m], t_want.astype(T)) and np.all(gt[m:] == 99.0), (m, n, delta, force, max_wg)
                assert float(dq.item()) == dq_want, (m, n, delta, force, max_wg)
                # neither optional output requested: the same q
                q2 = _vec(np.full(n, NAN), T, pad=3)
                assert dev.normal_matvec(ctx, m, n, Ad, dd, delta, q2, max_wg=max_wg, lda=lda) is None
                assert torch.equal(q2, q)
                moved = [a - b for a, b in zip(_counts(ctx), before)]
                assert moved == ([2, 0, 0, 0] if fused else [0, 2, 2, 2]), (m, n, force, moved)
                first = q if first is None else first
                assert torch.equal(first, q)
        assert np.array_equal(_np(Ad).T, Af.astype(T), equal_nan=True)
    assert ctx.lsq_path_count(45) == -1 and ctx.lsq_path_count(50) == -1 and ctx.lsq_path_count(0) == -1
    assert ctx.path_count(46) == -1 and ctx.pcg_path_count(46) == -1


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(4099, 33), (5000, 300), (3000, 1500), (1000, 2100)])
def test_matvec_kernels_reproducible_and_close(ctx, m, n, prec):
    """Gaussian data: two runs give the same bits on every route, and the result is within the rounding bound of its sums of numpy's;
    the forced one-pass route (option lsq_normal_fused = 1) and the forced composed route (0) agree to the same rounding"""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    rng = np.random.default_rng(m + n)
    A, d = rng.standard_normal((m, n)).astype(T), rng.standard_normal(n).astype(T)
    Ad, dd = _mat(A, T), _vec(d, T)
    A64, d64 = A.astype(np.float64), d.astype(np.float64)
    q_want = A64.T @ (A64 @ d64) + 0.25 * d64
    # each q_j is a sum of m products of a_ij with a sum of n products, plus one term: (m + n + 2) eps times the sum of the absolute values
    bound = (m + n + 2) * float(np.finfo(T).eps)
    scale = float(np.max(np.abs(A64).T @ (np.abs(A64) @ np.abs(d64)) + 0.25 * np.abs(d64)))
    for force in (1, 0):
        ctx.set_option("lsq_normal_fused", force)
        before = _counts(ctx)
        runs = []
        for _ in range(2):
            q, t = _vec(np.zeros(n), T), _vec(np.zeros(m), T)
            dq = dev.normal_matvec(ctx, m, n, Ad, dd, 0.25, q, t=t, want_dq=True)
            runs.append((q, t, dq))
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
        moved = [a - b for a, b in zip(_counts(ctx), before)]
        fused = force != 0 and n <= FUSED_MAX[prec]
        assert moved == ([2, 0, 0, 0] if fused else [0, 2, 2, 2])
        err = float(np.max(np.abs(_np(runs[0][0]).astype(np.float64) - q_want)))
        print(f"({m}, {n}) {prec} fused={fused}: max error {err:.3g}, allowed {bound * scale:.3g}")
        assert err <= bound * scale
    ctx.set_option("lsq_normal_fused", -1)


# ---------------------------------------------------------------------------------------------------
# 2. argument codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_argument_codes(ctx, prec):
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    T = DT[prec]
    lib, h = ctx.lib, ctx.h
    m, n = 7, 3
    A, x, y = _mat(np.ones((m, n)), T), _vec(np.ones(m), T), _vec(np.full(m, 5.0), T)
    p = lambda t: t.data_ptr()
    gemv = getattr(lib, f"rlhip_gemv_{prec}")
    assert gemv(h, b"X", m, n, 1.0, p(A), m, p(x), 0.0, p(y)) == -2
    assert gemv(h, b"N", -1, n, 1.0, p(A), m, p(x), 0.0, p(y)) == -3
    assert gemv(h, b"N", m, -1, 1.0, p(A), m, p(x), 0.0, p(y)) == -4
    assert gemv(h, b"N", m, n, 1.0, None, m, p(x), 0.0, p(y)) == -6
    assert gemv(h, b"T", m, n, 1.0, p(A), m - 1, p(x), 0.0, p(y)) == -7
    assert gemv(h, b"N", m, n, 1.0, p(A), m, None, 0.0, p(y)) == -8
    assert gemv(h, b"T", m, n, 1.0, p(A), m, p(x), 0.0, None) == -10
    before = _counts(ctx)
    for tr in (b"N", b"T"):                                            # BLAS's quick returns: nothing is written, nothing is launched
        assert gemv(h, tr, 0, n, 1.0, None, 1, None, 0.0, p(y)) == 0
        assert gemv(h, tr, m, 0, 1.0, None, m, None, 0.0, p(y)) == 0
        assert gemv(h, tr, m, n, 0.0, p(A), m, p(x), 1.0, p(y)) == 0
    assert _counts(ctx) == before and np.all(_np(y) == 5.0)
    assert gemv(h, b"n", m, n, 0.0, p(A), m, p(x), 2.0, p(y)) == 0      # alpha == 0 scales y
    assert np.all(_np(y) == 10.0)

    nm = getattr(lib, f"rlhip_normal_matvec_{prec}")
    d, q = _vec(np.arange(1, n + 1), T), _vec(np.full(n, 5.0), T)
    assert nm(h, -1, n, p(A), m, p(d), 0.0, p(q), None, None, 0) == -2
    assert nm(h, m, -1, p(A), m, p(d), 0.0, p(q), None, None, 0) == -3
    assert nm(h, m, n, None, m, p(d), 0.0, p(q), None, None, 0) == -4
    assert nm(h, m, n, p(A), m - 1, p(d), 0.0, p(q), None, None, 0) == -5
    assert nm(h, m, n, p(A), m, None, 0.0, p(q), None, None, 0) == -6
    assert nm(h, m, n, p(A), m, p(d), 0.0, None, None, None, 0) == -8
    assert nm(h, m, 0, None, m, None, 0.0, None, None, None, 0) == 0 and np.all(_np(q) == 5.0)
    dq = torch.zeros(1, dtype=q.dtype, device="cuda:0")
    assert nm(h, 0, n, None, 1, p(d), 0.5, p(q), None, p(dq), 0) == 0    # m == 0: q = delta d, d^T q = delta d^T d
    assert np.array_equal(_np(q), 0.5 * np.arange(1, n + 1)) and float(dq.item()) == 0.5 * 14.0

    one = _vec([2.0], T)
    sxr = getattr(lib, f"rlhip_pcg_saddle_step_xr_{prec}")
    assert sxr(h, -1, p(d), p(q), p(one), p(one), p(q), p(q)) == -2
    assert sxr(h, n, None, p(q), p(one), p(one), p(q), p(q)) == -3
    assert sxr(h, n, p(d), p(q), None, p(one), p(q), p(q)) == -5
    assert sxr(h, n, p(d), p(q), p(one), None, p(q), p(q)) == -6
    assert sxr(h, n, p(d), p(q), p(one), p(one), None, p(q)) == -7
    assert sxr(h, n, p(d), p(q), p(one), p(one), p(q), None) == -8
    assert sxr(h, 0, None, None, p(one), p(one), None, None) == 0
    srf = getattr(lib, f"rlhip_pcg_saddle_step_refresh_{prec}")
    assert srf(h, -1, p(d), p(d), 0.0, p(d), p(q)) == -2
    assert srf(h, n, None, p(d), 0.0, p(d), p(q)) == -3
    assert srf(h, n, p(d), None, 0.0, p(d), p(q)) == -4
    assert srf(h, n, p(d), p(d), 0.0, None, p(q)) == -6
    assert srf(h, n, p(d), p(d), 0.0, p(d), None) == -7
    sd = getattr(lib, f"rlhip_pcg_saddle_step_d_{prec}")
    assert sd(h, -1, p(d), p(d), p(one), p(one), p(q)) == -2
    assert sd(h, n, None, p(d), p(one), p(one), p(q)) == -3
    assert sd(h, n, p(d), None, p(one), p(one), p(q)) == -4
    assert sd(h, n, p(d), p(d), p(one), None, p(q)) == -6
    assert sd(h, n, p(d), p(d), p(one), p(one), None) == -7
    # the steps themselves on exact values: alpha = 2 / 2 = 1, x = q + d, r = q - q = 0; then r^T s and d = beta d + s
    xx, rr, qq = _vec([1.0, 1.0, 1.0], T), _vec([4.0, 5.0, 6.0], T), _vec([4.0, 5.0, 6.0], T)
    assert sxr(h, n, p(d), p(qq), p(one), p(one), p(xx), p(rr)) == 0
    assert np.array_equal(_np(xx), [2.0, 3.0, 4.0]) and np.array_equal(_np(rr), [0.0, 0.0, 0.0])
    assert srf(h, n, p(qq), p(d), 0.5, p(xx), p(rr)) == 0                # (4,5,6) - (1,2,3) - 0.5 (2,3,4)
    assert np.array_equal(_np(rr), [2.0, 1.5, 1.0])
    new, dd = _vec([0.0], T), _vec([1.0, 1.0, 1.0], T)
    assert sd(h, n, p(rr), p(d), p(one), p(new), p(dd)) == 0             # r^T s = 2 + 3 + 3 = 8, beta = 4, d = 4 + s
    assert float(new.item()) == 8.0 and np.array_equal(_np(dd), [5.0, 6.0, 7.0])
    assert sd(h, n, p(rr), p(d), None, p(new), None) == 0 and float(new.item()) == 8.0

    # the drivers refuse what the C++ layer refuses
    b, c, x0 = _vec(np.ones(m), T), _vec(np.zeros(n), T), _vec(np.zeros(n), T)
    M = _mat(np.eye(n), T)
    with pytest.raises(_lib.RlhipError):
        dev.pcg_saddle(ctx, A, m, n, b, c, 0.0, 5, 0.0, M, n, x0)        # tol must be > 0
    with pytest.raises(_lib.RlhipError):
        dev.pcg_saddle(ctx, A, m, n, b, c, -1.0, 5, 1e-3, M, n, x0)      # delta must be >= 0
    with pytest.raises(_lib.RlhipError):
        dev.rpc_data_svd_saso(ctx, A, m, n, n - 1, 2)                    # d >= n
    with pytest.raises(_lib.RlhipError):
        dev.make_right_orthogonalizer(ctx, M, _vec(np.ones(n), T), 0.0, cols_V=n + 1)
    with pytest.raises(_lib.RlhipError):
        dev.sap_lstsq(ctx, _mat(np.ones((2, n)), T), 2, n, b, c, 0.0, 4.0, 2, 1e-3, 5)   # m >= n


# ---------------------------------------------------------------------------------------------------
# 3. three iterations against the model
# ---------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), np.finfo(np.float64).tiny))


def _three_step_case(name, T):
    """(A, b, c, delta, M, x0)"""
    rng = np.random.default_rng(11)
    if name == "dense300":
        m, n = 300, 12
        return rng.standard_normal((m, n)), rng.standard_normal(m), np.zeros(n), 0.1, np.eye(n), np.zeros(n)
    m, n, d, delta = {"sketched4099": (4099, 33, 132, 0.0), "sketched2048": (2048, 128, 512, 0.1)}[name]
    A, b = lm.conv_case(m, n)
    S, _ = lm.saso(d, m, lm.CONV_NNZ, lm.CONV_KEY)
    V, sig = lm.rpc_data_svd(A.astype(T), S, T)
    M, rank = lm.make_right_orthogonalizer(V, sig, delta, T)
    if name == "sketched2048":                                         # c != 0 and x0 != 0
        return A, b, rng.standard_normal(n), delta, M[:, :rank], 1e-2 * rng.standard_normal(n)
    return A, b, np.zeros(n), delta, M[:, :rank], np.zeros(n)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["dense300", "sketched4099", "sketched2048"])
def test_three_steps_match_the_model(ctx, name, prec):
    """tol so small that nothing stops, three iterations: x, y and the residual history against the model in the same precision.  The
    allowance is DESIGN 4.19's: the model run again on the row-permuted problem differs from itself by rounding alone, and the device's
    order of summation differs from the model's at least as much as a permutation does; 100 times that difference, never less than 1000 eps."""
    from randlapack_amd import device as dev

    T = DT[prec]
    A, b, c, delta, M, x0 = (np.asarray(v, dtype=T) if not np.isscalar(v) else v for v in _three_step_case(name, T))
    m, n = A.shape
    tol = 1e-30
    xm, ym, itm, rm = lm.pcg_saddle(A, b, c, delta, 3, tol, M, x0, T)
    perm = np.random.default_rng(5).permutation(m)
    xp, yp, _, rp = lm.pcg_saddle(A[perm], b[perm], c, delta, 3, tol, M, x0, T)
    yp_back = np.empty_like(yp)
    yp_back[perm] = yp
    self_diff = max(_rel(xm, xp), _rel(ym, yp_back), _rel(rm, rp))
    allowed = max(100.0 * self_diff, 1000.0 * float(np.finfo(T).eps))
    r = dev.pcg_saddle(ctx, _mat(A, T), m, n, _vec(b, T), _vec(c, T), float(delta), 3, tol, _mat(M, T), M.shape[1], _vec(x0, T))
    dx, dy, dr = _rel(xm, _np(r["x"])), _rel(ym, _np(r["y"])), _rel(rm, r["resid"])
    print(f"{name} {prec}: model self-difference {self_diff:.3g}, allowed {allowed:.3g}; device x {dx:.3g} y {dy:.3g} resid {dr:.3g}")
    assert r["iters"] == itm == 3 and r["resid"].size == 4
    assert dx <= allowed and dy <= allowed and dr <= allowed


# ---------------------------------------------------------------------------------------------------
# 4. convergence
# ---------------------------------------------------------------------------------------------------
def _device_chain(ctx, A, b, c, delta, d, T, tol, iter_lim=lm.CONV_ITER_LIM, key=lm.CONV_KEY):
    """rpc_data_svd_saso -> make_right_orthogonalizer(mu = delta) -> pcg_saddle from x0 = 0 on the device"""
    from randlapack_amd import device as dev

    m, n = A.shape
    Ad = _mat(A, T)
    pc = dev.rpc_data_svd_saso(ctx, Ad, m, n, d, lm.CONV_NNZ, key=(key, 0))
    sigma = _np(pc["sigma"]).copy()
    rank = dev.make_right_orthogonalizer(ctx, pc["V"], pc["sigma"], float(delta))
    M = _np(pc["V"]).T[:, :rank].copy()
    r = dev.pcg_saddle(ctx, Ad, m, n, _vec(b, T), _vec(c, T), float(delta), iter_lim, tol, pc["V"], rank, _vec(np.zeros(n), T))
    r.update(M=M, rank=rank, sigma=sigma, next_ctr=pc["next_ctr"])
    return r


def _check_solution(r, A, b, c, delta, T, tol, model, label):
    m, n = A.shape
    x, y = _np(r["x"]), _np(r["y"])
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(r["M"]))
    ratio = lm.precond_residual(A, b, c, delta, x, r["M"])
    margin = 10.0 * max(tol, model["ratio"])
    print(f"{label}: device iters={r['iters']} rank={r['rank']} ratio={ratio:.3g}; model iters={model['iters']} rank={model['rank']} "
          f"ratio={model['ratio']:.3g}; margin {margin:.3g}")
    assert ratio <= margin
    assert abs(r["iters"] - model["iters"]) <= 2
    assert r["resid"].size == r["iters"] + 1
    A64, x64 = A.astype(np.float64), x.astype(np.float64)
    ybound = m * float(np.finfo(T).eps) * (np.linalg.norm(b) + np.linalg.norm(A64, 2) * np.linalg.norm(x64))
    assert np.linalg.norm(y.astype(np.float64) - (b.astype(np.float64) - A64 @ x64)) <= ybound


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,d", lm.CONV_SHAPES)
def test_convergence_with_the_model_as_yardstick(ctx, m, n, d, prec):
    """A = Gaussian diag(logspace(0, -6, n)): the true preconditioned residual, recomputed in float64 from the returned x and M, within
    10 max(tol, the model's ratio); the iteration count within 2 of the model's; y = b - A x.  fp32 runs with tol = 1e-4 (about 10^3 eps:
    the recursively updated residual of CG on a system of condition about 3 is good to roughly sqrt(n) eps, two orders below that)."""
    T = DT[prec]
    model = lm.conv_model(m, n, d, prec)
    tol = lm.CONV_TOL[T]
    r = _device_chain(ctx, model["A"], model["b"], model["c"], 0.0, d, T, tol)
    _check_solution(r, model["A"], model["b"], model["c"], 0.0, T, tol, model, f"({m}, {n}, {d}) {prec}")
    if prec == "f64":
        assert r["rank"] == model["rank"] == n


# ---------------------------------------------------------------------------------------------------
# 5. the preconditioner on the device
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("key", lm.PRECOND_KEYS)
@pytest.mark.parametrize("kind", ["noreg", "reg"])
def test_preconditioner_by_the_reference_checks(ctx, kind, key, prec):
    """test_preconditioners.cc through rpc_data_svd_saso + make_right_orthogonalizer: the rank the model finds (n in fp64), cond <= 10 on
    the columns that define the orthogonalizer, sigma equal to numpy's SVD of the same sketch to n eps sigma_1, the state advanced as the
    oracle's restatement of the operator advances it"""
    from randlapack_amd import device as dev

    T = DT[prec]
    sh = lm.PRECOND_SHAPE
    m, n, d, nnz = sh["m"], sh["n"], sh["d"], sh["nnz"]
    A64, mu = lm.precond_case(kind, key)
    A = A64.astype(T)
    S, nxt = lm.saso(d, m, nnz, key)
    Vm, sigm = lm.rpc_data_svd(A, S, T)
    _, rank_m = lm.make_right_orthogonalizer(Vm, sigm, mu, T)
    pc = dev.rpc_data_svd_saso(ctx, _mat(A, T), m, n, d, nnz, key=(key, 0))
    sig = _np(pc["sigma"]).astype(np.float64)
    V = _np(pc["V"]).T.astype(np.float64)
    assert pc["next_ctr"] == nxt
    serr = float(np.max(np.abs(sig - sigm.astype(np.float64))))
    print(f"{kind} key {key} {prec}: sigma error {serr:.3g}, allowed {n * np.finfo(T).eps * sig[0]:.3g}; |V^T V - I| {np.max(np.abs(V.T @ V - np.eye(n))):.3g}")
    assert serr <= n * float(np.finfo(T).eps) * sig[0]
    assert np.max(np.abs(V.T @ V - np.eye(n))) <= 100 * n * float(np.finfo(T).eps)
    rank = dev.make_right_orthogonalizer(ctx, pc["V"], pc["sigma"], mu)
    M = _np(pc["V"]).T.astype(np.float64)
    assert rank == rank_m and (prec == "f32" or rank == n)
    assert np.array_equal(M[:, rank:], V[:, rank:])                   # the columns beyond the rank are left alone
    A_aug = np.vstack([A.astype(np.float64), np.sqrt(mu) * np.eye(n)]) if mu > 0 else A.astype(np.float64)
    cnd = lm.cond(A_aug @ M[:, :rank])
    print(f"  rank {rank}, cond {cnd:.3g}")
    assert cnd <= 10.0


# ---------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_solver_edges(ctx, prec):
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(21)
    m, n = 300, 12
    A, b = rng.standard_normal((m, n)).astype(T), rng.standard_normal(m).astype(T)
    x0 = rng.standard_normal(n).astype(T)
    Ad, M, z = _mat(A, T), _mat(np.eye(n), T), _vec(np.zeros(n), T)
    # iter_lim = 0: x = x0, y = b - A x0, one residual recorded
    r = dev.pcg_saddle(ctx, Ad, m, n, _vec(b, T), z, 0.1, 0, 1e-6, M, n, _vec(x0, T))
    assert r["iters"] == 0 and r["resid"].size == 1 and r["resid"][0] > 0
    assert np.array_equal(_np(r["x"]), x0)
    yw = b.astype(np.float64) - A.astype(np.float64) @ x0.astype(np.float64)
    ybound = (n + 2) * eps * (np.abs(b).astype(np.float64) + np.abs(A).astype(np.float64) @ np.abs(x0).astype(np.float64))
    assert np.all(np.abs(_np(r["y"]) - yw) <= ybound)
    # b1 = A^T b - c = 0 and x0 = 0: delta_1 = 0, the loop does not start
    r = dev.pcg_saddle(ctx, Ad, m, n, _vec(np.zeros(m), T), z, 0.1, 10, 1e-6, M, n, z)
    assert r["iters"] == 0 and r["resid"].tolist() == [0.0]
    assert np.array_equal(_np(r["x"]), np.zeros(n)) and np.array_equal(_np(r["y"]), np.zeros(m))
    # the same call twice: the same bits
    a1 = dev.pcg_saddle(ctx, Ad, m, n, _vec(b, T), z, 0.1, 6, 1e-30, M, n, z)
    a2 = dev.pcg_saddle(ctx, Ad, m, n, _vec(b, T), z, 0.1, 6, 1e-30, M, n, z)
    assert a1["iters"] == 6 and torch.equal(a1["x"], a2["x"]) and torch.equal(a1["y"], a2["y"]) and np.array_equal(a1["resid"], a2["resid"])
    # m = n (square, well conditioned) and n = 1
    for mm, nn in ((40, 40), (500, 1)):
        Q = (rng.standard_normal((mm, nn)) + (3.0 * np.eye(mm, nn) if mm == nn else 0.0)).astype(T)
        bb = rng.standard_normal(mm).astype(T)
        model_M = np.eye(nn) / np.linalg.norm(Q.astype(np.float64), 2)
        tol = 1e-12 if T is np.float64 else 1e-5
        xmod, _, itm, _ = lm.pcg_saddle(Q, bb, np.zeros(nn), 0.0, 400, tol, model_M, np.zeros(nn), T)
        r = dev.pcg_saddle(ctx, _mat(Q, T), mm, nn, _vec(bb, T), _vec(np.zeros(nn), T), 0.0, 400, tol, _mat(model_M, T), nn, _vec(np.zeros(nn), T))
        ratio = lm.precond_residual(Q, bb, np.zeros(nn), 0.0, _np(r["x"]), model_M)
        rmod = lm.precond_residual(Q, bb, np.zeros(nn), 0.0, xmod, model_M)
        print(f"({mm}, {nn}) {prec}: device iters={r['iters']} ratio={ratio:.3g}; model iters={itm} ratio={rmod:.3g}")
        assert ratio <= 10 * max(tol, rmod) and r["iters"] < 400 and np.all(np.isfinite(_np(r["y"])))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_zero_column_without_regularization(ctx, prec):
    """an exactly zero column with delta = 0: the sketch has an exactly zero singular value, the orthogonalizer drops it (rank = n - 1 in
    fp64; what the model finds in fp32), everything stays finite and the preconditioned residual meets the convergence test's margin"""
    T = DT[prec]
    m, n, d = 4099, 33, 132
    model = lm.conv_model(m, n, d, prec, 0.0, 5)
    tol = lm.CONV_TOL[T]
    r = _device_chain(ctx, model["A"], model["b"], model["c"], 0.0, d, T, tol)
    assert r["sigma"][-1] <= n * float(np.finfo(T).eps) * r["sigma"][0]
    if prec == "f64":
        assert r["rank"] == model["rank"] == n - 1
    _check_solution(r, model["A"], model["b"], model["c"], 0.0, T, tol, model, f"zero column {prec}")


# ---------------------------------------------------------------------------------------------------
# 7. sap_lstsq
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_sap_lstsq(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    m, n, d = 4099, 33, 132
    model = lm.conv_model(m, n, d, prec)
    tol = lm.CONV_TOL[T]
    A, b, c = model["A"], model["b"], model["c"]
    Ad = _mat(A, T)
    r = dev.sap_lstsq(ctx, Ad, m, n, _vec(b, T), _vec(c, T), 0.0, 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0))
    pc = dev.rpc_data_svd_saso(ctx, Ad, m, n, d, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    assert r["next_ctr"] == pc["next_ctr"] == lm.saso(d, m, lm.CONV_NNZ, lm.CONV_KEY)[1]
    rank = dev.make_right_orthogonalizer(ctx, pc["V"], pc["sigma"], 0.0)
    assert rank == r["rank"]
    r["M"] = _np(pc["V"]).T[:, :rank].copy()
    _check_solution(r, A, b, c, 0.0, T, tol, model, f"sap_lstsq {prec}")
