"""Least squares with several right-hand sides on the device (randlapack_amd/csrc/lsq.hip, include/RandLAPACK_amd/rl_determiter.hh
pcg_saddle_block, rl_lstsq.hh) in fp64 and fp32: the normal product exactly on small integers on both routes, column
independence bit for bit, the two routes against each other, the block solver step by step against the model (tests/_lsq_block_model.py: the
single-column model column by column), convergence and freezing with the model as the yardstick, sap_lstsq with s right-hand sides against s
single calls, the argument codes and the edges.  Every test prints what it measured beside what it allows."""

import numpy as np
import pytest

import _lsq_block_model as bm
import _lsq_model as lm

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
EB = {"f64": 8, "f32": 4}
NAN = float("nan")
SENT = 99.5                                      # never the value of an integer-valued result


def _limit():
    from randlapack_amd import device as dev

    n = 1
    while dev.normal_matmat_fused(2 * n, 1, 8):
        n *= 2
    assert dev.normal_matmat_fused(n, 1, 4) and not dev.normal_matmat_fused(n + 1, 1, 4) and not dev.normal_matmat_fused(n + 1, 1, 8)
    return n                                     # RLHIP_NORMAL_MATMAT_FUSED_MAX_N (include/rlhip.h): a power of two


def _sc(prec):
    from randlapack_amd import device as dev

    return dev.normal_matmat_fused(1, 1000, EB[prec])


def _dev(a):
    """numpy (rows, cols) -> column-major device tensor (cols, rows)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda:0")


def _padded(a, ld, extra_cols, fill, T):
    """(rows, cols) -> device tensor (cols + extra_cols, ld), everything outside the block = fill"""
    rows, cols = a.shape
    full = np.full((ld, cols + extra_cols), fill, dtype=T)
    full[:rows, :cols] = a
    return _dev(full)


def _np(t):
    return t.detach().cpu().numpy()


def _counts(ctx):
    return [ctx.lsq_block_path_count(i) for i in (76, 77, 78)]


def _matmat(ctx, route, m, n, s, Ad, Dd, delta, T, lda, ldd, max_wg=0, want_t=True, pad=3):
    """one call on a forced route with sentinel-filled outputs that are wider and taller than the result.  Returns (Q, Tm, dq) as numpy
    arrays of the full buffers (transposed back to (ld, cols))."""
    import torch

    from randlapack_amd import device as dev

    ldq, ldt = n + pad, m + pad + 1
    Q = torch.full((s + 1, ldq), SENT, dtype=Ad.dtype, device="cuda:0")
    Tm = torch.full((s + 1, ldt), SENT, dtype=Ad.dtype, device="cuda:0") if want_t else None
    with ctx.normal_matmat_route(route):
        dq = dev.normal_matmat(ctx, m, n, s, Ad, Dd, delta, Q, T=Tm, want_dq=True, max_wg=max_wg, lda=lda, ldd=ldd, ldq=ldq, ldt=ldt)
    return _np(Q).T, (_np(Tm).T if want_t else None), _np(dq)


# ---------------------------------------------------------------------------------------------------
# 1. the normal product, exactly
# ---------------------------------------------------------------------------------------------------
N_KINDS = [1, 3, 33, 64, 100, "limit", "limit+1"]
M_VALUES = (1, 15, 16, 17, 255, 257, 4099)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n_kind", N_KINDS)
def test_normal_matmat_exact(ctx, n_kind, prec):
    """A and D in {-1, 0, 1}, delta = 2: every sum is an integer below 2^24 (checked on the data), so either precision must give numpy's
    float64 result bit for bit on either route.  Rows m .. lda - 1 of A and the slack of D hold NaN (never read); Q and T sit in wider and
    taller buffers whose sentinels must survive.  A covering subset of the grid: every m with every n; s walks {1, 2, 3, sc, sc + 1,
    2 sc + 1} and max_wg {1, 2, 3} so that over the n of this test every value of both meets both forced routes; the default route runs too."""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    limit, sc = _limit(), _sc(prec)
    n = {"limit": limit, "limit+1": limit + 1}.get(n_kind, n_kind)
    s_values = (1, 2, 3, sc, sc + 1, 2 * sc + 1)
    ni = N_KINDS.index(n_kind)
    for mi, m in enumerate(M_VALUES):
        s = s_values[(mi + ni) % len(s_values)]
        max_wg = (1, 2, 3)[(mi + ni) % 3]
        rng = np.random.default_rng(100000 * n + 10 * m + s)
        lda, ldd = m + 5, n + 2
        A = rng.integers(-1, 2, size=(m, n)).astype(np.float64)
        D = rng.integers(-1, 2, size=(n, s)).astype(np.float64)
        Ad, Dd = _padded(A, lda, 0, NAN, T), _padded(D, ldd, 1, NAN, T)
        t_want = A @ D
        q_want = A.T @ t_want + 2.0 * D
        dq_want = np.sum(D * q_want, axis=0)
        assert max(np.max(np.sum(np.abs(D * q_want), axis=0)), np.max(np.abs(q_want)), np.max(np.abs(t_want))) < 2 ** 24
        for route, wg in ((1, max_wg), (0, max_wg), (-1, 0), (1, 0)):
            one_pass = (route == 1 and n <= limit) or (route == -1 and bool(dev.normal_matmat_default(n, s, EB[prec])))
            before = _counts(ctx)
            Q, Tm, dq = _matmat(ctx, route, m, n, s, Ad, Dd, 2.0, T, lda, ldd, max_wg=wg)
            tag = (m, n, s, route, wg)
            assert np.array_equal(Q[:n, :s], q_want.astype(T)), tag
            assert np.array_equal(Tm[:m, :s], t_want.astype(T)), tag
            assert np.array_equal(dq.astype(np.float64), dq_want), tag
            assert np.all(Q[n:, :] == SENT) and np.all(Q[:, s:] == SENT) and np.all(Tm[m:, :] == SENT) and np.all(Tm[:, s:] == SENT), tag
            moved = [a - b for a, b in zip(_counts(ctx), before)]
            assert moved == ([1, 0, 0] if one_pass else [0, 1, 0]), (tag, moved)
        # neither optional output: the same Q
        for route in (1, 0):
            Q2 = torch.full((s, n), SENT, dtype=Ad.dtype, device="cuda:0")
            with ctx.normal_matmat_route(route):
                assert dev.normal_matmat(ctx, m, n, s, Ad, Dd, 2.0, Q2, lda=lda, ldd=ldd) is None
            assert np.array_equal(_np(Q2).T, q_want.astype(T)), (m, n, s, route)
        assert np.array_equal(_np(Ad).T[:m], A.astype(T))
    assert ctx.lsq_block_path_count(75) == -1 and ctx.lsq_block_path_count(79) == -1 and ctx.lsq_path_count(76) == -1


# ---------------------------------------------------------------------------------------------------
# 2. column independence, 3. the two routes against each other
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,s", [(4099, 33, 3), (1500, 300, 6), (700, 600, 3)])
def test_columns_are_independent_and_runs_repeat(ctx, m, n, s, prec):
    """Gaussian data: with column 1 of D set to NaN, the other columns of Q, T and dq keep the bits of the clean run on both routes
    (s = 6 spans two chunks of the one-pass route; n = 600 is beyond its limit, so both calls are composed); the same call twice gives
    the same bits"""
    T = DT[prec]
    rng = np.random.default_rng(m + n + s)
    A, D = rng.standard_normal((m, n)).astype(T), rng.standard_normal((n, s)).astype(T)
    Dn = D.copy()
    Dn[:, 1] = NAN
    Ad, Dd, Dnd = _dev(A), _dev(D), _dev(Dn)
    keep = [j for j in range(s) if j != 1]
    for route in (1, 0):
        clean = _matmat(ctx, route, m, n, s, Ad, Dd, 0.25, T, m, n)
        again = _matmat(ctx, route, m, n, s, Ad, Dd, 0.25, T, m, n)
        dirty = _matmat(ctx, route, m, n, s, Ad, Dnd, 0.25, T, m, n)
        for a, b, c in zip(clean, again, dirty):
            assert np.array_equal(a, b)
            assert np.array_equal(a[..., keep], c[..., keep]) and np.all(np.isfinite(a[..., keep][a[..., keep] != SENT]))
        assert np.all(np.isnan(dirty[0][:n, 1])) and np.isnan(dirty[2][1])
        print(f"({m}, {n}, {s}) {prec} route {route}: columns {keep} bit-identical with and without a NaN column 1")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n", [(4099, 33), (5000, 300), (3000, 512)])
def test_one_pass_against_composed(ctx, m, n, prec):
    """Gaussian data, s = 5: per column, both routes within the bound test_gpu_lsq.py::test_matvec_kernels_reproducible_and_close uses for
    the single-column pair: (m + n + 2) eps times the largest sum of absolute values of the column"""
    T = DT[prec]
    s = 5
    rng = np.random.default_rng(m + n)
    A, D = rng.standard_normal((m, n)).astype(T), rng.standard_normal((n, s)).astype(T)
    A64, D64 = A.astype(np.float64), D.astype(np.float64)
    q_want = A64.T @ (A64 @ D64) + 0.25 * D64
    bound = (m + n + 2) * float(np.finfo(T).eps)
    scale = np.max(np.abs(A64).T @ (np.abs(A64) @ np.abs(D64)) + 0.25 * np.abs(D64), axis=0)
    Ad, Dd = _dev(A), _dev(D)
    got = {}
    for route in (1, 0):
        before = _counts(ctx)
        Q, _, _ = _matmat(ctx, route, m, n, s, Ad, Dd, 0.25, T, m, n, want_t=False)
        assert [a - b for a, b in zip(_counts(ctx), before)] == ([1, 0, 0] if route else [0, 1, 0])
        got[route] = Q[:n, :s].astype(np.float64)
        err = np.max(np.abs(got[route] - q_want), axis=0)
        print(f"({m}, {n}) {prec} route {route}: max error per column {np.array2string(err, precision=3)}, allowed {np.array2string(bound * scale, precision=3)}")
        assert np.all(err <= bound * scale)
    diff = np.max(np.abs(got[1] - got[0]), axis=0)
    print(f"  one-pass against composed: {np.array2string(diff, precision=3)}, allowed {np.array2string(2 * bound * scale, precision=3)}")
    assert np.all(diff <= 2 * bound * scale)


# ---------------------------------------------------------------------------------------------------
# 4. three iterations against the model
# ---------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), np.finfo(np.float64).tiny))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["dense300", "sketched4099", "sketched2048"])
def test_three_steps_match_the_model(ctx, name, prec):
    """tol so small that nothing stops, three iterations, s = 3: x, y and the residual history of every column against the model in the
    same precision.  The allowance is that of test_gpu_lsq.py::test_three_steps_match_the_model, per column: 100 times the model's own
    difference under a row permutation, never less than 1000 eps.  On both routes; and s = 1 against pcg_saddle under the same allowance."""
    from randlapack_amd import device as dev

    T = DT[prec]
    A, B, C, delta, M, X0 = (np.asarray(v, dtype=T) if not np.isscalar(v) else v for v in bm.three_step_block(name, T))
    m, n = A.shape
    tol = 1e-30
    Xm, Ym, itm, rm = bm.pcg_saddle_block(A, B, C, delta, 3, tol, M, X0, T)
    perm = np.random.default_rng(5).permutation(m)
    Xp, Yp, _, rp = bm.pcg_saddle_block(A[perm], B[perm], C, delta, 3, tol, M, X0, T)
    Yp_back = np.empty_like(Yp)
    Yp_back[perm] = Yp
    allowed = []
    for j in range(3):
        self_diff = max(_rel(Xm[:, j], Xp[:, j]), _rel(Ym[:, j], Yp_back[:, j]), _rel(rm[j], rp[j]))
        allowed.append(max(100.0 * self_diff, 1000.0 * float(np.finfo(T).eps)))
    Ad, Md = _dev(A), _dev(M)
    for route in (-1, 1):
        before = _counts(ctx)
        with ctx.normal_matmat_route(route):
            r = dev.pcg_saddle_block(ctx, Ad, m, n, 3, _dev(B), _dev(C), float(delta), 3, tol, Md, M.shape[1], X0=_dev(X0))
        moved = [a - b for a, b in zip(_counts(ctx), before)]
        one_pass = route == 1 or bool(dev.normal_matmat_default(n, 3, EB[prec]))
        assert moved == ([5, 0, 3] if one_pass else [0, 5, 3]), moved                # products: x0, 3 iterations, 1 refresh
        assert r["iters"] == itm == [3, 3, 3] and r["resid"].shape == (3, 4)
        for j in range(3):
            dx, dy, dr = _rel(Xm[:, j], _np(r["x"])[j]), _rel(Ym[:, j], _np(r["y"])[j]), _rel(rm[j], r["resid"][j])
            print(f"{name} {prec} route {route} column {j}: allowed {allowed[j]:.3g}; device x {dx:.3g} y {dy:.3g} resid {dr:.3g}")
            assert dx <= allowed[j] and dy <= allowed[j] and dr <= allowed[j]
    one = dev.pcg_saddle_block(ctx, Ad, m, n, 1, _dev(B[:, :1]), _dev(C[:, :1]), float(delta), 3, tol, Md, M.shape[1], X0=_dev(X0[:, :1]))
    ref = dev.pcg_saddle(ctx, Ad, m, n, _dev(B[:, :1])[0], _dev(C[:, :1])[0], float(delta), 3, tol, Md, M.shape[1], _dev(X0[:, :1])[0])
    dx, dy, dr = _rel(_np(ref["x"]), _np(one["x"])[0]), _rel(_np(ref["y"]), _np(one["y"])[0]), _rel(ref["resid"], one["resid"][0])
    print(f"{name} {prec} s = 1 against pcg_saddle: allowed {allowed[0]:.3g}; x {dx:.3g} y {dy:.3g} resid {dr:.3g}")
    assert one["iters"] == [3] and ref["iters"] == 3 and dx <= allowed[0] and dy <= allowed[0] and dr <= allowed[0]


# ---------------------------------------------------------------------------------------------------
# 5. convergence and freezing
# ---------------------------------------------------------------------------------------------------
RESID_SENT = -7.0                                # delta_1 = r' M M' r is never negative


def _device_preconditioner(ctx, Ad, m, n, d, delta, key=lm.CONV_KEY):
    from randlapack_amd import device as dev

    pc = dev.rpc_data_svd_saso(ctx, Ad, m, n, d, lm.CONV_NNZ, key=(key, 0))
    rank = dev.make_right_orthogonalizer(ctx, pc["V"], pc["sigma"], float(delta))
    return pc, rank, _np(pc["V"]).T[:, :rank].copy()


def _check_columns(r, A, B, T, tol, model, label, zero_col=None):
    """per column: the iteration count within 2 of the model's, the float64 preconditioned residual ratio within 10 max(tol, the model's),
    y = b - A x within the bound of test_gpu_lsq.py::_check_solution, resid below iters_j untouched"""
    m, n = A.shape
    A64 = A.astype(np.float64)
    X, Y = _np(r["x"]).T, _np(r["y"]).T
    nrmA = np.linalg.norm(A64, 2)
    for j in range(B.shape[1]):
        it = r["iters"][j]
        assert abs(it - model["iters"][j]) <= 2, (label, j, it, model["iters"][j])
        assert np.all(r["resid"][j, it + 1:] == RESID_SENT) and np.all(r["resid"][j, : it + 1] >= 0), (label, j)
        x64, b64 = X[:, j].astype(np.float64), B[:, j].astype(np.float64)
        if j == zero_col:
            assert it == 0 and np.all(X[:, j] == 0) and np.all(Y[:, j] == 0) and r["resid"][j, 0] == 0
            print(f"{label} column {j}: zero right-hand side, iters 0")
            continue
        assert np.all(np.isfinite(X[:, j])) and np.all(np.isfinite(Y[:, j]))
        ratio = lm.precond_residual(A, B[:, j], np.zeros(n), 0.0, X[:, j], r["M"])
        margin = 10.0 * max(tol, model["ratio"][j])
        yerr = np.linalg.norm(Y[:, j].astype(np.float64) - (b64 - A64 @ x64))
        ybound = m * float(np.finfo(T).eps) * (np.linalg.norm(b64) + nrmA * np.linalg.norm(x64))
        print(f"{label} column {j}: device iters={it} ratio={ratio:.3g}; model iters={model['iters'][j]} ratio={model['ratio'][j]:.3g}; margin {margin:.3g}; "
              f"|y - (b - A x)| {yerr:.3g}, allowed {ybound:.3g}")
        assert ratio <= margin and yerr <= ybound


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,d", lm.CONV_SHAPES)
def test_convergence_and_freezing(ctx, m, n, d, prec):
    """five right-hand sides with the preconditioner built on the device (tests/_lsq_block_model.py conv_rhs): the Gaussian column runs
    long, the eigenvector columns stop after about 1, 2 and 4 iterations and stay frozen while the others go on, the zero column never
    starts.  The yardstick is the model run with the same M.  Then one column of B set to NaN: it reports 0 iterations and every other
    column keeps the bits of the clean run."""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    tol = lm.CONV_TOL[T]
    A64, b = lm.conv_case(m, n)
    A = A64.astype(T)
    Ad = _dev(A)
    pc, rank, M = _device_preconditioner(ctx, Ad, m, n, d, 0.0)
    B = bm.conv_rhs(A, M, b).astype(T)
    model = bm.conv_block_model(A, M, B, prec)
    print(f"({m}, {n}, {d}) {prec}: rank {rank}, model iters {model['iters']}")
    assert max(model["iters"][1:4]) <= 6 and model["iters"][0] >= (20 if prec == "f64" else 8) and model["iters"][4] == 0
    s = B.shape[1]

    def run(Bh):
        resid = torch.full((s, lm.CONV_ITER_LIM + 1), RESID_SENT, dtype=Ad.dtype, device="cuda:0")
        r = dev.pcg_saddle_block(ctx, Ad, m, n, s, _dev(Bh), None, 0.0, lm.CONV_ITER_LIM, tol, pc["V"], rank, resid=resid)
        r["M"] = M
        return r

    before = _counts(ctx)
    r = run(B)
    moved = [a - b2 for a, b2 in zip(_counts(ctx), before)]
    by_default = bool(dev.normal_matmat_default(n, s, EB[prec]))         # the default route for this shape: DESIGN 4.31's measured ranges
    assert moved[2] == max(r["iters"]) and moved[0 if by_default else 1] > 0 and moved[1 if by_default else 0] == 0   # as long as the longest column
    _check_columns(r, A, B, T, tol, model, f"({m}, {n}, {d}) {prec}", zero_col=4)
    Bn = B.copy()
    Bn[:, 2] = NAN
    rn = run(Bn)
    assert rn["iters"][2] == 0 and rn["iters"] == [v if j != 2 else 0 for j, v in enumerate(r["iters"])]
    keep = [0, 1, 3, 4]
    assert torch.equal(rn["x"][keep], r["x"][keep]) and torch.equal(rn["y"][keep], r["y"][keep])
    assert np.array_equal(rn["resid"][keep], r["resid"][keep]) and np.all(rn["resid"][2, 1:] == RESID_SENT) and np.isnan(rn["resid"][2, 0])
    assert np.all(_np(rn["x"][2]) == 0)                                  # x_j = x0_j
    # the other route reaches the same solutions under the same checks
    with ctx.normal_matmat_route(0 if by_default else 1):
        r1 = run(B)
    _check_columns(r1, A, B, T, tol, model, f"({m}, {n}, {d}) {prec} {'composed' if by_default else 'one-pass'}", zero_col=4)


# ---------------------------------------------------------------------------------------------------
# 6. sap_lstsq with s right-hand sides
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_sap_lstsq_block_against_single_calls(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    m, n, d = 4099, 33, 132
    tol = lm.CONV_TOL[T]
    A64, b = lm.conv_case(m, n)
    A = A64.astype(T)
    Ad = _dev(A)
    pc, rank, M = _device_preconditioner(ctx, Ad, m, n, d, 0.0)
    B = bm.conv_rhs(A, M, b).astype(T)[:, :4]
    s = B.shape[1]
    model = bm.conv_block_model(A, M, B, prec)
    Bd = _dev(B)
    r = dev.sap_lstsq_block(ctx, Ad, m, n, s, Bd, None, 0.0, 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0))
    z = _dev(np.zeros((n, 1), dtype=T))[0]
    singles = [dev.sap_lstsq(ctx, Ad, m, n, Bd[j], z, 0.0, 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0)) for j in range(s)]
    assert r["rank"] == rank and all(one["rank"] == rank for one in singles)
    assert r["next_ctr"] == pc["next_ctr"] and all(one["next_ctr"] == r["next_ctr"] for one in singles)
    print(f"sap_lstsq_block {prec}: rank {r['rank']}, iters {r['iters']}, single calls {[one['iters'] for one in singles]}, model {model['iters']}")
    for j in range(s):
        assert abs(r["iters"][j] - singles[j]["iters"]) <= 2
        ratio = lm.precond_residual(A, B[:, j], np.zeros(n), 0.0, _np(r["x"])[j], M)
        single_ratio = lm.precond_residual(A, B[:, j], np.zeros(n), 0.0, _np(singles[j]["x"]), M)
        margin = 10.0 * max(tol, model["ratio"][j])
        print(f"  column {j}: ratio {ratio:.3g} (single call {single_ratio:.3g}), margin {margin:.3g}")
        assert ratio <= margin
        assert np.all(np.isnan(r["resid"][j, r["iters"][j] + 1:])) and np.all(r["resid"][j, : r["iters"][j] + 1] >= 0)


# ---------------------------------------------------------------------------------------------------
# 7. argument codes and edges
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_argument_codes(ctx, prec):
    import torch

    T = DT[prec]
    lib, h = ctx.lib, ctx.h
    p = lambda t: t.data_ptr()
    m, n, s = 7, 3, 2
    A = _dev(np.ones((m, n), dtype=T))
    D = _dev(np.array([[1.0, 2.0], [2.0, 0.0], [3.0, 1.0]], dtype=T))
    Q, Tm = _dev(np.full((n, s), 5.0, dtype=T)), _dev(np.full((m, s), 5.0, dtype=T))
    nm = getattr(lib, f"rlhip_normal_matmat_{prec}")
    assert nm(None, m, n, s, p(A), m, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -1
    assert nm(h, -1, n, s, p(A), m, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -2
    assert nm(h, m, -1, s, p(A), m, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -3
    assert nm(h, m, n, -1, p(A), m, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -4
    assert nm(h, m, n, s, None, m, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -5
    assert nm(h, m, n, s, p(A), m - 1, p(D), n, 0.0, p(Q), n, None, m, None, 0) == -6
    assert nm(h, m, n, s, p(A), m, None, n, 0.0, p(Q), n, None, m, None, 0) == -7
    assert nm(h, m, n, s, p(A), m, p(D), n - 1, 0.0, p(Q), n, None, m, None, 0) == -8
    assert nm(h, m, n, s, p(A), m, p(D), n, 0.0, None, n, None, m, None, 0) == -10
    assert nm(h, m, n, s, p(A), m, p(D), n, 0.0, p(Q), n - 1, None, m, None, 0) == -11
    assert nm(h, m, n, s, p(A), m, p(D), n, 0.0, p(Q), n, p(Tm), m - 1, None, 0) == -13
    before = _counts(ctx)
    assert nm(h, m, 0, s, None, m, None, 1, 0.0, None, 1, None, m, None, 0) == 0
    assert nm(h, m, n, 0, p(A), m, None, n, 0.0, None, n, None, m, None, 0) == 0
    assert np.all(_np(Q) == 5.0) and np.all(_np(Tm) == 5.0)
    dq = torch.zeros(s, dtype=Q.dtype, device="cuda:0")
    assert nm(h, 0, n, s, None, 1, p(D), n, 0.5, p(Q), n, None, 1, p(dq), 0) == 0       # m == 0: Q = delta D, d^T q = delta d^T d
    assert np.array_equal(_np(Q).T, 0.5 * _np(D).T) and _np(dq).tolist() == [0.5 * 14.0, 0.5 * 5.0]
    assert _counts(ctx) == before                                        # none of these reached a route

    # the setter: the value found comes back, -1 for no context
    assert lib.rlhip_normal_matmat_set_route(h, 1) == -1
    assert lib.rlhip_normal_matmat_set_route(h, 0) == 1
    assert lib.rlhip_normal_matmat_set_route(h, 7) == 0
    assert lib.rlhip_normal_matmat_set_route(h, -1) == 1
    assert lib.rlhip_normal_matmat_set_route(None, 1) == -1 and lib.rlhip_lsq_block_path_count(None, 76) == -1

    # the steps: codes, then exact values with column 1 switched off
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda:0")
    vec = lambda v: torch.tensor(v, dtype=Q.dtype, device="cuda:0")
    Dd, Qd = vec([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]), vec([[4.0, 5.0, 6.0], [4.0, 5.0, 6.0]])
    X, R = vec([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]), vec([[4.0, 5.0, 6.0], [4.0, 5.0, 6.0]])
    dqv, hist, act = vec([2.0, 2.0]), vec([[2.0, SENT], [2.0, SENT]]), i32([1, 0])
    sxr = getattr(lib, f"rlhip_pcg_saddle_block_step_xr_{prec}")
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("n", n), ("s", s), ("D", p(Dd)), ("ldd", n), ("Q", p(Qd)), ("ldq", n), ("dq", p(dqv)),
                                                  ("d1", p(hist)), ("ldh", 2), ("X", p(X)), ("ldx", n), ("R", p(R)), ("ldr", n), ("act", p(act)))]
    for code, kw in ((-1, dict(h=None)), (-2, dict(n=-1)), (-3, dict(s=-1)), (-3, dict(s=65536)), (-4, dict(D=None)), (-5, dict(ldd=n - 1)),
                     (-7, dict(ldq=n - 1)), (-8, dict(dq=None)), (-9, dict(d1=None)), (-10, dict(ldh=0)), (-11, dict(X=None)), (-12, dict(ldx=n - 1)),
                     (-13, dict(R=None)), (-14, dict(ldr=n - 1)), (-15, dict(act=None))):
        assert sxr(*args(**kw)) == code, (code, kw)
    assert sxr(*args(n=0, D=None, X=None)) == 0 and sxr(*args(s=0, D=None, X=None)) == 0
    assert sxr(*args()) == 0                                             # alpha_0 = 2 / 2: x = 1 + d, r = q - q
    assert _np(X).tolist() == [[2.0, 3.0, 4.0], [1.0, 1.0, 1.0]] and _np(R).tolist() == [[0.0, 0.0, 0.0], [4.0, 5.0, 6.0]]
    srf = getattr(lib, f"rlhip_pcg_saddle_block_step_refresh_{prec}")
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("n", n), ("s", s), ("B1", p(Qd)), ("ldb1", n), ("QX", p(Dd)), ("ldqx", n), ("delta", 0.5),
                                                  ("X", p(X)), ("ldx", n), ("R", p(R)), ("ldr", n), ("act", p(act)))]
    for code, kw in ((-1, dict(h=None)), (-2, dict(n=-1)), (-3, dict(s=-1)), (-4, dict(B1=None)), (-5, dict(ldb1=n - 1)), (-6, dict(QX=None)),
                     (-7, dict(ldqx=n - 1)), (-9, dict(X=None)), (-10, dict(ldx=n - 1)), (-11, dict(R=None)), (-12, dict(ldr=n - 1)), (-13, dict(act=None))):
        assert srf(*args(**kw)) == code, (code, kw)
    assert srf(*args()) == 0                                             # (4,5,6) - (1,2,3) - 0.5 (2,3,4)
    assert _np(R).tolist() == [[2.0, 1.5, 1.0], [4.0, 5.0, 6.0]]
    sd = getattr(lib, f"rlhip_pcg_saddle_block_step_d_{prec}")
    rel, dd = vec([SENT, SENT]), vec([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("n", n), ("s", s), ("R", p(R)), ("ldr", n), ("S", p(Dd)), ("lds", n), ("old", p(hist)),
                                                  ("new", p(hist) + hist.element_size()), ("ldh", 2), ("D", p(dd)), ("ldd", n), ("tol", 0.5),
                                                  ("rel", p(rel)), ("act", p(act)))]
    for code, kw in ((-1, dict(h=None)), (-2, dict(n=-1)), (-3, dict(s=-1)), (-4, dict(R=None)), (-5, dict(ldr=n - 1)), (-6, dict(S=None)),
                     (-7, dict(lds=n - 1)), (-9, dict(new=None)), (-10, dict(ldh=0)), (-11, dict(D=None)), (-12, dict(ldd=n - 1)), (-14, dict(rel=None)),
                     (-15, dict(act=None))):
        assert sd(*args(**kw)) == code, (code, kw)
    before = _counts(ctx)
    # the first call: every column, whatever its flag held: r^T s = (8, 32), rel_sq_tol = (r^T s / 2) / 2, the flags set
    assert sd(*args(old=None, new=p(hist), D=None)) == 0
    assert _np(hist).tolist() == [[8.0, SENT], [32.0, SENT]] and _np(rel).tolist() == [2.0, 8.0] and _np(act).tolist() == [1, 1]
    assert _counts(ctx) == before
    act.copy_(i32([1, 0]))
    assert sd(*args()) == 0                                              # column 0: beta = 8 / 8, d = d + s; column 1 is left alone
    assert _np(hist).tolist() == [[8.0, 8.0], [32.0, SENT]] and _np(dd).tolist() == [[2.0, 3.0, 4.0], [1.0, 1.0, 1.0]] and _np(act).tolist() == [1, 0]
    assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 0, 1]
    # delta1 > rel_sq_tol false clears the flag: equality (tol = 1 on the first call) and NaN
    assert sd(*args(old=None, new=p(hist), D=None, tol=1.0)) == 0 and _np(act).tolist() == [0, 0] and _np(rel).tolist() == [8.0, 32.0]
    R[1, 0] = NAN
    assert sd(*args(old=None, new=p(hist), D=None, tol=0.5)) == 0 and _np(act).tolist() == [1, 0] and np.isnan(_np(hist)[1, 0])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n_kind,stalled", [(1, False), (256, False), (257, False), ("wrap", False), (257, True)])
def test_single_steps_are_block_steps_with_one_column(ctx, n_kind, stalled, prec):
    """rlhip_pcg_saddle_step_{d, xr, refresh}_* against rlhip_pcg_saddle_block_step_*_* with s = 1 on copies of the same random inputs: step_d
    (first call), step_xr with q, step_xr without q, step_refresh, step_d (update).  Every output -- x, r, d, delta1 -- must agree bit for
    bit, the sentinels behind every vector must survive, and the single calls must not move counter 78 (the block update call moves it by
    one).  n = 256 and 257 lie on either side of the stride of the dot product, n = 256 num_cu + 3 makes step_xr's grid-stride loop wrap.
    stalled: s = 0, so the first step_d finds delta1 = 0 and the block call clears its flag (0 > 0 is false).  The single entry points have
    no flag -- the ONE intended difference: the block calls then leave x, r, d and the next delta1 alone while the single calls still write
    them."""
    import torch

    T = DT[prec]
    lib, h = ctx.lib, ctx.h
    n = 256 * torch.cuda.get_device_properties(0).multi_processor_count + 3 if n_kind == "wrap" else n_kind
    PAD, delta, tol = 4, 0.375, 1e-3
    rng = np.random.default_rng(7000 + n)

    def buf(v):
        return torch.from_numpy(np.concatenate([np.asarray(v, dtype=T), np.full(PAD, SENT, dtype=T)])).to("cuda:0")

    names = ("x", "r", "d", "q", "qx", "b1")
    host = {k: rng.standard_normal(n) for k in names}
    host["s"] = np.zeros(n) if stalled else host["r"] * (0.5 + rng.random(n))    # r^T s > 0 unless stalled
    one = {k: buf(v) for k, v in host.items()}                                   # the single calls' vectors
    blk = {k: t.clone() for k, t in one.items()}                                 # the block calls'
    first = {k: t.clone() for k, t in one.items()}                               # as they went in
    scal = lambda v: torch.tensor(v, dtype=one["x"].dtype, device="cuda:0")
    dq = scal([1.5 + rng.random()])
    hist1, histb = scal([SENT, SENT, SENT]), scal([SENT, SENT, SENT])            # delta1 of the first call, of the update, a sentinel
    rel, act = scal([SENT, SENT]), torch.tensor([7, 7], dtype=torch.int32, device="cuda:0")
    p, eb, ld = (lambda t: t.data_ptr()), one["x"].element_size(), n + PAD
    fn = lambda name: getattr(lib, f"rlhip_pcg_saddle_{name}_{prec}")
    before = _counts(ctx)

    # step_d, the first call
    assert fn("step_d")(h, n, p(one["r"]), p(one["s"]), None, p(hist1), None) == 0
    assert fn("block_step_d")(h, n, 1, p(blk["r"]), ld, p(blk["s"]), ld, None, p(histb), 2, None, ld, tol, p(rel), p(act)) == 0
    assert torch.equal(hist1, histb) and _np(hist1)[1:].tolist() == [SENT, SENT]
    d1 = _np(hist1)[0]
    print(f"n = {n} {prec}: delta1 = {d1!r}")
    assert _np(rel).tolist() == [T(T(d1 * T(tol)) * T(tol)), SENT] and _np(act).tolist() == [0 if stalled else 1, 7]
    assert (d1 == 0) if stalled else (d1 > 0)
    # step_xr with q, then without
    assert fn("step_xr")(h, n, p(one["d"]), p(one["q"]), p(dq), p(hist1), p(one["x"]), p(one["r"])) == 0
    assert fn("block_step_xr")(h, n, 1, p(blk["d"]), ld, p(blk["q"]), ld, p(dq), p(histb), 2, p(blk["x"]), ld, p(blk["r"]), ld, p(act)) == 0
    if not stalled:
        assert torch.equal(one["x"], blk["x"]) and torch.equal(one["r"], blk["r"])
        assert not torch.equal(one["x"], first["x"]) and not torch.equal(one["r"], first["r"])
        after_q = one["r"].clone()
    assert fn("step_xr")(h, n, p(one["d"]), None, p(dq), p(hist1), p(one["x"]), None) == 0
    assert fn("block_step_xr")(h, n, 1, p(blk["d"]), ld, None, ld, p(dq), p(histb), 2, p(blk["x"]), ld, None, ld, p(act)) == 0
    if not stalled:
        assert torch.equal(one["x"], blk["x"]) and torch.equal(one["r"], after_q) and torch.equal(blk["r"], after_q)
    # step_refresh
    assert fn("step_refresh")(h, n, p(one["b1"]), p(one["qx"]), delta, p(one["x"]), p(one["r"])) == 0
    assert fn("block_step_refresh")(h, n, 1, p(blk["b1"]), ld, p(blk["qx"]), ld, delta, p(blk["x"]), ld, p(blk["r"]), ld, p(act)) == 0
    if not stalled:
        assert torch.equal(one["r"], blk["r"]) and not torch.equal(one["r"], after_q)
    assert _counts(ctx) == before
    # step_d, the update
    assert fn("step_d")(h, n, p(one["r"]), p(one["s"]), p(hist1), p(hist1) + eb, p(one["d"])) == 0
    assert _counts(ctx) == before                                                # no single call is an iteration of the block solver
    assert fn("block_step_d")(h, n, 1, p(blk["r"]), ld, p(blk["s"]), ld, p(histb), p(histb) + eb, 2, p(blk["d"]), ld, tol, p(rel), p(act)) == 0
    assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 0, 1]            # counted on the host, whatever the flag holds
    if not stalled:
        assert torch.equal(hist1, histb) and torch.equal(one["d"], blk["d"]) and not torch.equal(one["d"], first["d"])
        assert _np(hist1)[1] != SENT and _np(hist1)[2] == SENT
    else:
        # the block column was left alone by every call after the first; the single calls wrote r (refresh) and delta1 (update)
        assert all(torch.equal(blk[k], first[k]) for k in names) and _np(histb).tolist() == [0.0, SENT, SENT] and _np(act).tolist() == [0, 7]
        assert not torch.equal(one["r"], first["r"]) and _np(hist1)[:2].tolist() == [0.0, 0.0] and _np(hist1)[2] == SENT
    # nothing was written behind a vector, no input was written
    for k in names + ("s",):
        assert np.all(_np(one[k])[n:] == SENT) and np.all(_np(blk[k])[n:] == SENT), k
    for k in ("q", "qx", "b1", "s"):
        assert torch.equal(one[k], first[k]) and torch.equal(blk[k], first[k]), k


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_solver_edges(ctx, prec):
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(21)
    m, n, s = 300, 12, 3
    A, B = rng.standard_normal((m, n)).astype(T), rng.standard_normal((m, s)).astype(T)
    X0 = rng.standard_normal((n, s)).astype(T)
    Ad, Md, Bd = _dev(A), _dev(np.eye(n, dtype=T)), _dev(B)
    # iter_lim = 0: X = X0, Y = B - A X0, one residual per column
    r = dev.pcg_saddle_block(ctx, Ad, m, n, s, Bd, None, 0.1, 0, 1e-6, Md, n, X0=_dev(X0))
    assert r["iters"] == [0, 0, 0] and r["resid"].shape == (s, 1) and np.all(r["resid"] > 0)
    assert np.array_equal(_np(r["x"]).T, X0)
    A64, X64 = A.astype(np.float64), X0.astype(np.float64)
    ybound = (n + 2) * eps * (np.abs(B).astype(np.float64) + np.abs(A64) @ np.abs(X64))
    assert np.all(np.abs(_np(r["y"]).T - (B.astype(np.float64) - A64 @ X64)) <= ybound)
    # s == 0: nothing to do, nothing written
    r = dev.pcg_saddle_block(ctx, Ad, m, n, 0, None, None, 0.1, 5, 1e-6, Md, n)
    assert r["iters"] == [] and r["x"].shape[0] == 0
    r = dev.sap_lstsq_block(ctx, Ad, m, n, 0, None, None, 0.0, 4.0, 4, 1e-6, 5, key=(3, 0))
    assert r["iters"] == [] and r["rank"] == n
    assert r["next_ctr"] == dev.rpc_data_svd_saso(ctx, Ad, m, n, 4 * n, 4, key=(3, 0))["next_ctr"]
    # the same call twice: the same bits
    a1 = dev.pcg_saddle_block(ctx, Ad, m, n, s, Bd, None, 0.1, 6, 1e-30, Md, n)
    a2 = dev.pcg_saddle_block(ctx, Ad, m, n, s, Bd, None, 0.1, 6, 1e-30, Md, n)
    assert a1["iters"] == [6, 6, 6] and torch.equal(a1["x"], a2["x"]) and torch.equal(a1["y"], a2["y"]) and np.array_equal(a1["resid"], a2["resid"])
    # what the C++ layer refuses
    with pytest.raises(_lib.RlhipError):
        dev.pcg_saddle_block(ctx, Ad, m, n, s, Bd, None, 0.1, 5, 0.0, Md, n)           # tol must be > 0
    with pytest.raises(_lib.RlhipError):
        dev.pcg_saddle_block(ctx, Ad, m, n, s, Bd, None, -1.0, 5, 1e-3, Md, n)         # delta must be >= 0
    with pytest.raises(_lib.RlhipError):
        dev.pcg_saddle_block(ctx, Ad, m, n, -1, Bd, None, 0.1, 5, 1e-3, Md, n)         # s must be >= 0
    with pytest.raises(_lib.RlhipError):
        dev.sap_lstsq_block(ctx, _dev(np.ones((2, n), dtype=T)), 2, n, s, Bd, None, 0.0, 4.0, 2, 1e-3, 5)   # m >= n


def test_row_sharded_operator_is_refused():
    """least squares over a row-sharded operator is not built: with two ranks (a second context of this process under a host all-reduce
    hook that is never reached) both block entries are refused with their message before any product"""
    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    T = np.float64
    m, n, s = 50, 4, 2
    rng = np.random.default_rng(1)
    c2 = dev.Context(0)
    hook = _lib.HOOK(lambda user, buf, count, is_f64: -1)
    try:
        _lib.check(c2.lib.rlhip_comm_set_hook(c2.h, hook, None, 2, 0), "rlhip_comm_set_hook")
        Ad, Bd, Md = _dev(rng.standard_normal((m, n)).astype(T)), _dev(rng.standard_normal((m, s)).astype(T)), _dev(np.eye(n, dtype=T))
        before = _counts(c2)
        with pytest.raises(_lib.RlhipError, match="row-sharded"):
            dev.pcg_saddle_block(c2, Ad, m, n, s, Bd, None, 0.0, 5, 1e-6, Md, n)
        with pytest.raises(_lib.RlhipError, match="row-sharded"):
            dev.sap_lstsq_block(c2, Ad, m, n, s, Bd, None, 0.0, 4.0, 4, 1e-6, 5)
        assert _counts(c2) == before
    finally:
        c2.lib.rlhip_comm_destroy(c2.h)
        c2.close()
