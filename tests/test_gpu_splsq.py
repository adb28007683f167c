"""Sparse least squares on the device (randlapack_amd/csrc/spmv.hip; the SparseLinOp overloads of pcg_saddle, rpc_data_svd_saso and sap_lstsq
in include/RandLAPACK_amd/) in fp64 and fp32: the sparse matrix-vector kernels exactly on small integers on every route, reproducible and
within their rounding bound on Gaussian values, the argument codes, the solver step by step against the numpy model on the densified
matrix, the dense descriptor against the dense entries bit for bit, the three storage forms, convergence with the model as the yardstick,
and the edges.  Cases and yardsticks: tests/_splsq_cases.py."""
import numpy as np
import pytest

import _lsq_model as lm
import _splsq_cases as sc

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
NAN = float("nan")


def _t(a, dtype=None):
    import torch

    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to("cuda:0")          # (a copy: the cases are read-only arrays)


def _mat(a, T):
    """(rows, cols) numpy -> column-major device tensor (cols, rows)"""
    return _t(np.asarray(a, dtype=T).T)


def _vec(a, T, pad=0, fill=99.0):
    return _t(np.concatenate([np.asarray(a, dtype=T).ravel(), np.full(pad, fill, dtype=T)]))


def _np(t):
    return t.detach().cpu().numpy()


def _counts(ctx):
    return [ctx.spmv_path_count(i) for i in (50, 51, 52, 53, 54)]


def _moved(ctx, before):
    return [a - b for a, b in zip(_counts(ctx), before)]


def _route_slot(lanes, nrows, nnz):
    """index into _counts of the route a product takes, None when it launches no product kernel (nnz == 0)"""
    if nnz == 0:
        return None
    return sc.ROUTE_INDEX[lanes if lanes >= 0 else sc.default_route(nrows, nnz)] - 50


_DEV = {}


def _dev_csr(cs, T):
    """the CSR of the case and of its transpose on the device, uploaded once per precision"""
    key = (id(cs), T)
    if key not in _DEV:
        _DEV[key] = ((_t(cs["rowptr"]), _t(cs["colidx"]), _t(cs["vals"], T)), (_t(cs["rowptr_t"]), _t(cs["colidx_t"]), _t(cs["vals_t"], T)))
    return _DEV[key]


def _unchanged(cs, T):
    fwd, bwd = _dev_csr(cs, T)
    return all(np.array_equal(_np(d), np.asarray(h, dtype=_np(d).dtype)) for d, h in
               zip(fwd + bwd, (cs["rowptr"], cs["colidx"], cs["vals"], cs["rowptr_t"], cs["colidx_t"], cs["vals_t"])))


# ---------------------------------------------------------------------------------------------------
# 1. csr_spmv, exactly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("lanes", sc.LANES)
def test_csr_spmv_exact(ctx, lanes, prec):
    """every exact case, A x on the CSR and A^T x on the transpose's CSR, three (alpha, beta), the route forced by RLHIP_OPT_SPMV_LANES:
    every partial sum is an integer or half-integer below 2^23 (test_splsq_cases.py checks that on the data), so the result must equal
    numpy's bit for bit.  Outputs sit in longer buffers whose tail must survive, y holds NaN when beta == 0, exactly the counter of the
    route taken moves, the inputs are unchanged."""
    from randlapack_amd import device as dev

    T = DT[prec]
    ctx.set_option("spmv_lanes", lanes)
    assert ctx.get_option("spmv_lanes") == lanes
    for cs in sc.exact_cases(prec):
        fwd, bwd = _dev_csr(cs, T)
        nnz = cs["colidx"].size
        for csr, nr, nc, A, x, y0 in ((fwd, cs["nrows"], cs["ncols"], cs["A"], cs["x"], cs["y0"]),
                                      (bwd, cs["ncols"], cs["nrows"], cs["A"].T, cs["xt"], cs["y0t"])):
            xd = _vec(x, T)
            for alpha, beta in sc.ALPHA_BETA:
                before = _counts(ctx)
                y = _vec(np.full(nr, NAN) if beta == 0.0 else y0, T, pad=3)
                dev.csr_spmv(ctx, nr, nc, csr[0], csr[1], csr[2], alpha, xd, beta, y)
                want = alpha * (A @ x) + (beta * y0 if beta != 0.0 else 0.0)
                got = _np(y)
                assert np.array_equal(got[:nr], want.astype(T)) and np.all(got[nr:] == 99.0), (cs["name"], nr, nc, alpha, beta, lanes)
                expect = [0] * 5
                slot = _route_slot(lanes, nr, nnz)
                if slot is not None:
                    expect[slot] = 1
                assert _moved(ctx, before) == expect, (cs["name"], nr, nc, lanes)
            assert np.array_equal(_np(xd), x.astype(T))
        assert _unchanged(cs, T), cs["name"]
    assert ctx.spmv_path_count(49) == -1 and ctx.spmv_path_count(55) == -1 and ctx.spmv_path_count(0) == -1
    assert ctx.lsq_path_count(50) == -1 and ctx.path_count(50) == -1 and ctx.pcg_path_count(50) == -1


# ---------------------------------------------------------------------------------------------------
# 2. csr_normal_matvec, exactly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("lanes", sc.LANES)
def test_csr_normal_matvec_exact(ctx, lanes, prec):
    """q = A^T (A d) + delta d, t = A d and d^T q on every exact case: exact, the same bits for every max_wg and for two runs, with and
    without the optional outputs; counter 54 and the counters of the two products move"""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    ctx.set_option("spmv_lanes", lanes)
    for cs in sc.exact_cases(prec):
        fwd, bwd = _dev_csr(cs, T)
        m, n, nnz, A, d = cs["nrows"], cs["ncols"], cs["colidx"].size, cs["A"], cs["x"]
        dd = _vec(d, T)
        t_want = A @ d
        expect = [0, 0, 0, 0, 1]
        for slot in (_route_slot(lanes, m, nnz), _route_slot(lanes, n, nnz)):
            if slot is not None:
                expect[slot] += 1
        for delta in (0.0, 0.5):
            q_want = A.T @ t_want + delta * d
            dq_want = float(d @ q_want)
            first = None
            for max_wg in (0, 1, 2, 3, 0):
                before = _counts(ctx)
                q, t = _vec(np.full(n, NAN), T, pad=3), _vec(np.full(m, NAN), T, pad=3)
                dq = dev.csr_normal_matvec(ctx, m, n, fwd, bwd, dd, delta, q, t=t, want_dq=True, max_wg=max_wg)
                gq, gt = _np(q), _np(t)
                assert np.array_equal(gq[:n], q_want.astype(T)) and np.all(gq[n:] == 99.0), (cs["name"], delta, lanes, max_wg)
                assert np.array_equal(gt[:m], t_want.astype(T)) and np.all(gt[m:] == 99.0), (cs["name"], delta, lanes, max_wg)
                assert float(dq.item()) == dq_want, (cs["name"], delta, lanes, max_wg)
                assert _moved(ctx, before) == expect, (cs["name"], lanes, max_wg)
                first = q if first is None else first
                assert torch.equal(first, q)
            # neither optional output requested: the same q
            q2 = _vec(np.full(n, NAN), T, pad=3)
            assert dev.csr_normal_matvec(ctx, m, n, fwd, bwd, dd, delta, q2) is None
            assert torch.equal(q2, first)
        assert _unchanged(cs, T) and np.array_equal(_np(dd), d.astype(T)), cs["name"]


# ---------------------------------------------------------------------------------------------------
# 3. Gaussian values: reproducible, and within the rounding bound of the sums
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(lm.CONV_SHAPES)))
def test_spmv_reproducible_and_close(ctx, idx, prec):
    """the convergence matrices: two runs give the same bits on every route, and every route is within (len + 2) eps times the sum of the
    absolute values of the products, per output, of numpy in float64 -- len the row length for A x, the column length for A^T x.  The bound
    is derived: a sum of len products in any order carries at most (len - 1) roundings of partial sums and one per product, the scaling by
    alpha one more."""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    cs = sc.conv_case(idx)
    m, n = cs["m"], cs["n"]
    vals = cs["vals"].astype(T)
    rpt, cit, vt = sc.transpose_csr(m, n, cs["rowptr"], cs["colidx"], vals)
    A64 = sc.densify(m, n, cs["rowptr"], cs["colidx"], vals.astype(np.float64))
    rng = np.random.default_rng(idx)
    worst = 0.0
    for (rp, ci, v), nr, nc, A in (((cs["rowptr"], cs["colidx"], vals), m, n, A64), ((rpt, cit, vt), n, m, A64.T)):
        x = rng.standard_normal(nc).astype(T)
        want = A @ x.astype(np.float64)
        bound = (np.diff(rp) + 2) * eps * (np.abs(A) @ np.abs(x.astype(np.float64)))
        csr = (_t(rp), _t(ci), _t(v))
        xd = _t(x)
        for lanes in sc.LANES:
            ctx.set_option("spmv_lanes", lanes)
            ys = []
            for _ in range(2):
                y = _vec(np.full(nr, NAN), T)
                dev.csr_spmv(ctx, nr, nc, csr[0], csr[1], csr[2], 1.0, xd, 0.0, y)
                ys.append(y)
            assert torch.equal(ys[0], ys[1])
            err = np.abs(_np(ys[0]).astype(np.float64) - want)
            assert np.all(err <= bound), (nr, nc, lanes, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
    print(f"conv case {idx} {prec}: largest error / bound over both products and all routes = {worst:.3g}")


# ---------------------------------------------------------------------------------------------------
# 4. argument codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_argument_codes(ctx, prec):
    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    T = DT[prec]
    lib, h = ctx.lib, ctx.h
    cs = sc.exact_cases(prec)[5]                                        # 2 x 7
    (rp, ci, v), (rpt, cit, vt) = _dev_csr(cs, T)
    m, n, nnz = cs["nrows"], cs["ncols"], cs["colidx"].size
    assert nnz > 0
    p = lambda t: t.data_ptr()
    x, y = _vec(np.ones(n), T), _vec(np.full(m, 5.0), T)
    spmv = getattr(lib, f"rlhip_csr_spmv_{prec}")
    before = _counts(ctx)
    assert spmv(None, m, n, nnz, p(rp), p(ci), p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, -1, n, nnz, p(rp), p(ci), p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, -1, nnz, p(rp), p(ci), p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, n, -1, p(rp), p(ci), p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, n, nnz, None, p(ci), p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, n, nnz, p(rp), None, p(v), 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, n, nnz, p(rp), p(ci), None, 1.0, p(x), 0.0, p(y)) == -2
    assert spmv(h, m, n, nnz, p(rp), p(ci), p(v), 1.0, None, 0.0, p(y)) == -2
    assert spmv(h, m, n, nnz, p(rp), p(ci), p(v), 1.0, p(x), 0.0, None) == -2
    assert spmv(h, 0, n, 0, None, None, None, 1.0, p(x), 0.0, None) == 0      # no rows: nothing to do
    assert _counts(ctx) == before and np.all(_np(y) == 5.0)
    zrp = _t(np.zeros(m + 1, dtype=np.int64))
    assert spmv(h, m, n, 0, p(zrp), None, None, 1.0, None, 2.0, p(y)) == 0     # no entries: y is scaled
    assert np.all(_np(y) == 10.0) and _counts(ctx) == before

    nm = getattr(lib, f"rlhip_csr_normal_matvec_{prec}")
    d, q = _vec(np.arange(1, n + 1), T), _vec(np.full(n, 5.0), T)
    args = lambda **kw: [kw.get(k, dflt) for k, dflt in (("h", h), ("m", m), ("n", n), ("nnz", nnz), ("rp", p(rp)), ("ci", p(ci)), ("v", p(v)), ("rpt", p(rpt)),
                                                       ("cit", p(cit)), ("vt", p(vt)), ("d", p(d)), ("delta", 0.0), ("q", p(q)), ("t", None), ("dq", None),
                                                       ("wg", 0))]
    for bad in (dict(h=None), dict(m=-1), dict(n=-1), dict(nnz=-1), dict(rp=None), dict(ci=None), dict(v=None), dict(rpt=None), dict(cit=None), dict(vt=None),
                dict(d=None), dict(q=None)):
        assert nm(*args(**bad)) == -2, bad
    assert np.all(_np(q) == 5.0) and _counts(ctx) == before
    assert nm(*args(n=0, nnz=0, rpt=None, d=None, q=None, ci=None, v=None, cit=None, vt=None)) == 0 and np.all(_np(q) == 5.0)
    dq = _vec([0.0], T)
    zrpt = _t(np.zeros(n + 1, dtype=np.int64))
    assert nm(*args(m=0, nnz=0, rp=None, ci=None, v=None, rpt=p(zrpt), cit=None, vt=None, delta=0.5, dq=p(dq))) == 0    # m == 0: q = delta d
    assert np.array_equal(_np(q), 0.5 * np.arange(1, n + 1)) and float(dq.item()) == 0.5 * float(np.sum(np.arange(1, n + 1) ** 2))

    # the drivers refuse what the C++ layer refuses, with a message
    op = dev.CsrOperator(m, n, rp, ci, v)
    tall = sc.conv_case(1)
    top = dev.CsrOperator(tall["m"], tall["n"], _t(tall["rowptr"]), _t(tall["colidx"]), _t(tall["vals"], T))
    b, c, x0 = _vec(np.ones(tall["m"]), T), _vec(np.zeros(tall["n"]), T), _vec(np.zeros(tall["n"]), T)
    M = _mat(np.eye(tall["n"]), T)
    with pytest.raises(_lib.RlhipError, match="composite"):
        dev.pcg_saddle_op(ctx, (top, dev.DenseOperator(M, tall["n"], tall["n"])), b, c, 0.0, 5, 1e-3, M, tall["n"], x0)
    with pytest.raises(_lib.RlhipError, match="composite"):
        dev.sap_lstsq_op(ctx, (top, dev.DenseOperator(M, tall["n"], tall["n"])), b, c, 0.0, 4.0, 2, 1e-3, 5)
    with pytest.raises(_lib.RlhipError, match="composite"):
        dev.rpc_data_svd_saso_op(ctx, (top, dev.DenseOperator(M, tall["n"], tall["n"])), 4 * tall["n"], 2)
    with pytest.raises(_lib.RlhipError, match="tol"):
        dev.pcg_saddle_op(ctx, top, b, c, 0.0, 5, 0.0, M, tall["n"], x0)
    with pytest.raises(_lib.RlhipError, match="delta"):
        dev.sap_lstsq_op(ctx, top, b, c, -1.0, 4.0, 2, 1e-3, 5)
    with pytest.raises(_lib.RlhipError):
        dev.rpc_data_svd_saso_op(ctx, top, tall["n"] - 1, 2)                  # d >= n
    with pytest.raises(_lib.RlhipError):
        dev.sap_lstsq_op(ctx, op, _vec(np.ones(m), T), _vec(np.zeros(n), T), 0.0, 4.0, 2, 1e-3, 5)   # m >= n
    bad_kind = dev.CsrOperator(m, n, rp, ci, v)
    bad_kind.desc = lambda: _lib.LinOpDesc(7, m, n, None, 0, nnz, p(rp), p(ci), p(v))
    with pytest.raises(_lib.RlhipError, match="kind"):
        dev.pcg_saddle_op(ctx, bad_kind, b, c, 0.0, 5, 1e-3, M, n, x0)


# ---------------------------------------------------------------------------------------------------
# 5. three iterations against the model
# ---------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), np.finfo(np.float64).tiny))


def _csr_op(cs, T, vals=None):
    from randlapack_amd import device as dev

    return dev.CsrOperator(cs["m"], cs["n"], _t(cs["rowptr"]), _t(cs["colidx"]), _t(cs["vals"] if vals is None else vals, T))


def _three_step_problem(idx, T):
    """(A, b, c, delta, M, x0) on the densified conv_case(idx); idx 2 runs with delta = 0.1, c != 0 and x0 != 0"""
    cs = sc.conv_case(idx)
    m, n, d = cs["m"], cs["n"], cs["d"]
    delta = 0.1 if idx == 2 else 0.0
    A = sc.densify(m, n, cs["rowptr"], cs["colidx"], cs["vals"].astype(T).astype(np.float64)).astype(T)
    S, _ = lm.saso(d, m, lm.CONV_NNZ, lm.CONV_KEY)
    V, sig = lm.rpc_data_svd(A, S, T)
    M, rank = lm.make_right_orthogonalizer(V, sig, delta, T)
    rng = np.random.default_rng(11)
    c, x0 = (rng.standard_normal(n), 1e-2 * rng.standard_normal(n)) if idx == 2 else (np.zeros(n), np.zeros(n))
    return A, cs["b"].astype(T), c.astype(T), delta, M[:, :rank].astype(T), x0.astype(T)


def _three_step_allowance(A, b, c, delta, M, x0, T):
    """test_three_steps_match_the_model's: the model run again on the row-permuted problem differs from itself by rounding alone; 100 times
    that difference, never less than 1000 eps"""
    m = A.shape[0]
    tol = 1e-30
    xm, ym, itm, rm = lm.pcg_saddle(A, b, c, delta, 3, tol, M, x0, T)
    perm = np.random.default_rng(5).permutation(m)
    xp, yp, _, rp = lm.pcg_saddle(A[perm], b[perm], c, delta, 3, tol, M, x0, T)
    yp_back = np.empty_like(yp)
    yp_back[perm] = yp
    self_diff = max(_rel(xm, xp), _rel(ym, yp_back), _rel(rm, rp))
    return (xm, ym, itm, rm), self_diff, max(100.0 * self_diff, 1000.0 * float(np.finfo(T).eps))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(lm.CONV_SHAPES)))
def test_three_steps_match_the_model(ctx, idx, prec):
    """pcg_saddle_op on a CsrOperator, tol so small that nothing stops, three iterations: x, y and the residual history against the model on
    the densified matrix in the same precision, under the allowance of test_gpu_lsq.py::test_three_steps_match_the_model"""
    from randlapack_amd import device as dev

    T = DT[prec]
    A, b, c, delta, M, x0 = _three_step_problem(idx, T)
    (xm, ym, itm, rm), self_diff, allowed = _three_step_allowance(A, b, c, delta, M, x0, T)
    before = _counts(ctx)
    r = dev.pcg_saddle_op(ctx, _csr_op(sc.conv_case(idx), T), _vec(b, T), _vec(c, T), float(delta), 3, 1e-30, _mat(M, T), M.shape[1], _vec(x0, T))
    dx, dy, dr = _rel(xm, _np(r["x"])), _rel(ym, _np(r["y"])), _rel(rm, r["resid"])
    print(f"conv case {idx} {prec}: model self-difference {self_diff:.3g}, allowed {allowed:.3g}; device x {dx:.3g} y {dy:.3g} resid {dr:.3g}")
    assert r["iters"] == itm == 3 and r["resid"].size == 4
    assert dx <= allowed and dy <= allowed and dr <= allowed
    moved = _moved(ctx, before)
    assert moved[4] == 1 + 3 + 1 and sum(moved[:4]) == 2 * moved[4] + 2      # x0, three iterations, the refresh of iteration 1; A^T b and y = b - A x


# ---------------------------------------------------------------------------------------------------
# 6. the dense descriptor runs the dense entries
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_dense_descriptor_gives_the_dense_bits(ctx, prec):
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    idx = 1
    A, b, c, delta, M, x0 = _three_step_problem(idx, T)
    m, n = A.shape
    Ad, bd, cd, Md, x0d = _mat(A, T), _vec(b, T), _vec(c, T), _mat(M, T), _vec(x0, T)
    op = dev.DenseOperator(Ad, m, n)
    before = _counts(ctx)
    r0 = dev.pcg_saddle(ctx, Ad, m, n, bd, cd, float(delta), 6, 1e-30, Md, M.shape[1], x0d)
    r1 = dev.pcg_saddle_op(ctx, op, bd, cd, float(delta), 6, 1e-30, Md, M.shape[1], x0d)
    assert r0["iters"] == r1["iters"] == 6 and torch.equal(r0["x"], r1["x"]) and torch.equal(r0["y"], r1["y"]) and np.array_equal(r0["resid"], r1["resid"])
    tol = lm.CONV_TOL[T]
    s0 = dev.sap_lstsq(ctx, Ad, m, n, bd, cd, 0.0, 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0))
    s1 = dev.sap_lstsq_op(ctx, op, bd, cd, 0.0, 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0))
    assert (s0["rank"], s0["iters"], s0["next_ctr"]) == (s1["rank"], s1["iters"], s1["next_ctr"])
    assert torch.equal(s0["x"], s1["x"]) and torch.equal(s0["y"], s1["y"]) and np.array_equal(s0["resid"], s1["resid"])
    p0 = dev.rpc_data_svd_saso(ctx, Ad, m, n, 4 * n, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    p1 = dev.rpc_data_svd_saso_op(ctx, op, 4 * n, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    assert torch.equal(p0["V"], p1["V"]) and torch.equal(p0["sigma"], p1["sigma"]) and p0["next_ctr"] == p1["next_ctr"]
    assert _counts(ctx) == before                                       # no sparse kernel ran


# ---------------------------------------------------------------------------------------------------
# 7. storage forms
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_storage_forms(ctx, prec):
    """a canonical CSR (sorted columns, no duplicates) and its CSC hold the same two structures after the stable transposition: identical
    bits in sap_lstsq_op.  Shuffled COO triplets change the order inside a row and a column: three steps agree under the allowance of
    test_three_steps_match_the_model (the sketch itself is an order-free integer sum, so M is the same)."""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    idx = 1
    cs = sc.conv_case(idx)
    m, n = cs["m"], cs["n"]
    vals = cs["vals"].astype(T)
    rpt, cit, vt = sc.transpose_csr(m, n, cs["rowptr"], cs["colidx"], vals)
    b, c = _vec(cs["b"], T), _vec(np.zeros(n), T)
    tol = lm.CONV_TOL[T]
    run = lambda op, lim, tl: dev.sap_lstsq_op(ctx, op, b, c, 0.0, 4.0, lm.CONV_NNZ, tl, lim, key=(lm.CONV_KEY, 0))
    csr = dev.CsrOperator(m, n, _t(cs["rowptr"]), _t(cs["colidx"]), _t(vals))
    csc = dev.CscOperator(m, n, _t(rpt), _t(cit), _t(vt))
    r0, r1 = run(csr, lm.CONV_ITER_LIM, tol), run(csc, lm.CONV_ITER_LIM, tol)
    assert (r0["rank"], r0["iters"], r0["next_ctr"]) == (r1["rank"], r1["iters"], r1["next_ctr"])
    assert torch.equal(r0["x"], r1["x"]) and torch.equal(r0["y"], r1["y"]) and np.array_equal(r0["resid"], r1["resid"])
    perm = np.random.default_rng(9).permutation(vals.size)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(cs["rowptr"]))
    coo = dev.CooOperator(m, n, _t(rows[perm]), _t(cs["colidx"][perm]), _t(vals[perm]))
    A, bb, cc, delta, M, x0 = _three_step_problem(idx, T)
    _, self_diff, allowed = _three_step_allowance(A, bb, cc, delta, M, x0, T)
    a0, a1 = run(csr, 3, 1e-30), run(coo, 3, 1e-30)
    dx, dy, dr = _rel(_np(a0["x"]), _np(a1["x"])), _rel(_np(a0["y"]), _np(a1["y"])), _rel(a0["resid"], a1["resid"])
    print(f"{prec}: COO against CSR after three steps: x {dx:.3g} y {dy:.3g} resid {dr:.3g}; allowed {allowed:.3g}")
    assert a0["iters"] == a1["iters"] == 3 and a0["rank"] == a1["rank"] and a0["next_ctr"] == a1["next_ctr"]
    assert dx <= allowed and dy <= allowed and dr <= allowed
    full = run(coo, lm.CONV_ITER_LIM, tol)
    assert abs(full["iters"] - r0["iters"]) <= 2 and full["rank"] == r0["rank"]


# ---------------------------------------------------------------------------------------------------
# 8. convergence with the model as yardstick
# ---------------------------------------------------------------------------------------------------
def _check_solution(r, A, b, c, delta, T, tol, model, label):
    """the criteria of test_gpu_lsq.py::_check_solution"""
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


def _solve_and_check(ctx, idx, prec, delta, zero_col=-1):
    from randlapack_amd import device as dev

    T = DT[prec]
    cs = sc.conv_case(idx)
    m, n, d = cs["m"], cs["n"], cs["d"]
    model = sc.conv_model(idx, prec, delta, zero_col)
    vals = cs["vals"].copy()
    if zero_col >= 0:
        vals[cs["colidx"] == zero_col] = 0.0                            # stored zeros: the structure stays
    op = _csr_op(cs, T, vals)
    tol = lm.CONV_TOL[T]
    r = dev.sap_lstsq_op(ctx, op, _vec(model["b"], T), _vec(model["c"], T), float(delta), 4.0, lm.CONV_NNZ, tol, lm.CONV_ITER_LIM, key=(lm.CONV_KEY, 0))
    pc = dev.rpc_data_svd_saso_op(ctx, op, d, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    assert r["next_ctr"] == pc["next_ctr"] == model["next_ctr"]
    sigma = _np(pc["sigma"]).copy()
    rank = dev.make_right_orthogonalizer(ctx, pc["V"], pc["sigma"], float(delta))
    assert rank == r["rank"]
    r["M"] = _np(pc["V"]).T[:, :rank].copy()
    _check_solution(r, model["A"], model["b"], model["c"], delta, T, tol, model, f"conv case {idx} {prec} delta={delta} zero_col={zero_col}")
    return r, model, sigma


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("delta", [0.0, 0.1])
@pytest.mark.parametrize("idx", range(len(lm.CONV_SHAPES)))
def test_convergence_with_the_model_as_yardstick(ctx, idx, delta, prec):
    """sap_lstsq_op on a CsrOperator: the true preconditioned residual, recomputed in float64 from the returned x and M, within
    10 max(tol, the model's ratio); the iteration count within 2 of the model's; y = b - A x; the model's rank in fp64; sigma equal to
    numpy's SVD of the same sketch to n eps sigma_1 (the bound of test_preconditioner_by_the_reference_checks)"""
    T = DT[prec]
    r, model, sigma = _solve_and_check(ctx, idx, prec, delta)
    n = sc.conv_case(idx)["n"]
    if prec == "f64":
        assert r["rank"] == model["rank"] == n
    serr = float(np.max(np.abs(sigma.astype(np.float64) - model["sigma"].astype(np.float64))))
    print(f"  sigma error against the model {serr:.3g}, allowed {n * np.finfo(T).eps * sigma[0]:.3g}")
    assert serr <= n * float(np.finfo(T).eps) * sigma[0]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("idx", range(len(lm.CONV_SHAPES)))
def test_sketch_of_the_sparse_operator_is_the_dense_one(ctx, idx, prec):
    """rpc_data_svd_saso_op on the CsrOperator against rpc_data_svd_saso on the densified matrix: the sign operator is the same, so the
    state afterwards and sigma are identical.  The sparse sketch (rlhip_saso_apply_csr_ordered_*) adds the stored entries of a column in
    ascending row, cut into the partial groups of the dense sketch; a zero term changes no running sum, so the two sketches agree bit for
    bit (3000 x 64 takes the dense LDS-DMA kernel with a ragged last block as a group of its own, the two other shapes the register-staged one)."""
    from randlapack_amd import device as dev

    T = DT[prec]
    cs = sc.conv_case(idx)
    m, n, d = cs["m"], cs["n"], cs["d"]
    A = sc.densify(m, n, cs["rowptr"], cs["colidx"], cs["vals"].astype(T).astype(np.float64)).astype(T)
    ps = dev.rpc_data_svd_saso_op(ctx, _csr_op(cs, T), d, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    pd = dev.rpc_data_svd_saso(ctx, _mat(A, T), m, n, d, lm.CONV_NNZ, key=(lm.CONV_KEY, 0))
    ss, sd = _np(ps["sigma"]).astype(np.float64), _np(pd["sigma"]).astype(np.float64)
    print(f"conv case {idx} {prec}: max |sigma_sparse - sigma_dense| / sigma_1 = {np.max(np.abs(ss - sd)) / sd[0]:.3g} (eps = {np.finfo(T).eps:.3g})")
    assert ps["next_ctr"] == pd["next_ctr"]
    assert np.array_equal(ss, sd)


# ---------------------------------------------------------------------------------------------------
# 9. edges
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_solver_edges(ctx, prec):
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    cs = sc.conv_case(1)
    m, n = cs["m"], cs["n"]
    A, b, c, delta, M, x0 = _three_step_problem(1, T)
    rng = np.random.default_rng(21)
    x0 = rng.standard_normal(n).astype(T)
    op, Md, z = _csr_op(cs, T), _mat(M, T), _vec(np.zeros(n), T)
    # iter_lim = 0: x = x0, y = b - A x0, one residual recorded
    r = dev.pcg_saddle_op(ctx, op, _vec(b, T), z, 0.1, 0, 1e-6, Md, M.shape[1], _vec(x0, T))
    assert r["iters"] == 0 and r["resid"].size == 1 and r["resid"][0] > 0
    assert np.array_equal(_np(r["x"]), x0)
    A64 = A.astype(np.float64)
    yw = b.astype(np.float64) - A64 @ x0.astype(np.float64)
    ybound = (np.diff(cs["rowptr"]) + 2) * eps * (np.abs(b).astype(np.float64) + np.abs(A64) @ np.abs(x0).astype(np.float64))
    assert np.all(np.abs(_np(r["y"]) - yw) <= ybound)
    # x0 already the solution, exactly: integer data with b = A x0, so r = A^T b - A^T A x0 = 0, delta_1 = 0 and the loop does not start
    ex = next(e for e in sc.exact_cases(prec) if e["name"] == "257x64")
    eop = dev.CsrOperator(257, 64, *_dev_csr(ex, T)[0])
    bx = ex["A"] @ ex["x"]
    r = dev.pcg_saddle_op(ctx, eop, _vec(bx, T), _vec(np.zeros(64), T), 0.0, 10, 1e-6, _mat(np.eye(64), T), 64, _vec(ex["x"], T))
    assert r["iters"] == 0 and r["resid"].tolist() == [0.0]
    assert np.array_equal(_np(r["x"]), ex["x"].astype(T)) and np.array_equal(_np(r["y"]), np.zeros(257))
    # the same call twice: the same bits
    a1 = dev.pcg_saddle_op(ctx, op, _vec(b, T), z, 0.1, 6, 1e-30, Md, M.shape[1], z)
    a2 = dev.pcg_saddle_op(ctx, op, _vec(b, T), z, 0.1, 6, 1e-30, Md, M.shape[1], z)
    assert a1["iters"] == 6 and torch.equal(a1["x"], a2["x"]) and torch.equal(a1["y"], a2["y"]) and np.array_equal(a1["resid"], a2["resid"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("delta", [0.0, 0.1])
def test_zero_column(ctx, delta, prec):
    """an all-zero column (its entries stored as zeros).  delta = 0: the sketch has an exactly zero singular value and the orthogonalizer
    drops it (rank n - 1 in fp64; what the model finds in fp32); delta = 0.1: the regularization keeps every column.  Everything stays
    finite and the solve meets the convergence test's criteria."""
    T = DT[prec]
    n = sc.conv_case(1)["n"]
    r, model, sigma = _solve_and_check(ctx, 1, prec, delta, zero_col=5)
    assert sigma[-1] <= n * float(np.finfo(T).eps) * sigma[0]
    if prec == "f64":
        assert r["rank"] == model["rank"] == (n - 1 if delta == 0.0 else n)


def test_row_sharded_operator_is_refused():
    """least squares over a row-sharded operator is not built: with two ranks (a second context of this process under a host all-reduce
    hook that is never reached) pcg_saddle_op and sap_lstsq_op on a sparse operator are refused with their message before any product"""
    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    T = np.float64
    cs = sc.conv_case(1)
    m, n = cs["m"], cs["n"]
    c2 = dev.Context(0)
    hook = _lib.HOOK(lambda user, buf, count, is_f64: -1)
    try:
        _lib.check(c2.lib.rlhip_comm_set_hook(c2.h, hook, None, 2, 0), "rlhip_comm_set_hook")
        op = _csr_op(cs, T)
        b, z, M = _vec(cs["b"], T), _vec(np.zeros(n), T), _mat(np.eye(n), T)
        before = _counts(c2)
        with pytest.raises(_lib.RlhipError, match="row-sharded"):
            dev.pcg_saddle_op(c2, op, b, z, 0.0, 5, 1e-6, M, n, z)
        with pytest.raises(_lib.RlhipError, match="row-sharded"):
            dev.sap_lstsq_op(c2, op, b, z, 0.0, 4.0, lm.CONV_NNZ, 1e-6, 5)
        assert _counts(c2) == before
    finally:
        c2.lib.rlhip_comm_destroy(c2.h)
        c2.close()
