"""Restricted kernel ridge regression on the device: rlhip_ridge_filter_* against the extended-precision filter model, and
krill_restricted_rpchol / krill_restricted / krr_predict_restricted through their C entries in fp64 and fp32, for the three kernel kinds,
against the float64 dense solve of tests/_krr_restricted_model.py.

Tolerances.  The filter: 2 eps_T per entry (the factor is formed in double with one fused multiply-add and one division and rounded once, the
product adds one rounding in T).  The fit: the device's error against the dense solve (a) may be 8 times the error of the numpy model (b) of
the same algorithm in the same dtype on the same centres, with a floor of 64 eps_T -- both errors relative to the largest entry of (a).  The
factor 8 covers the other summation order of the device's Jacobi SVD and blocked triangular solve.  The largest ratios measured on an MI355X
are in DESIGN 4.24.  Prediction: 64 eps_T |K| |alpha| componentwise, the bound of tests/test_gpu_krr.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import _krr_model as km
import _krr_restricted_model as rm
import _pcg_model as pm
import _pdk_model as pk

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
# (n, rows_x, k, b, s) and, per n, the bandwidth of each kernel kind: tests/test_krr_restricted_model.py says how they were chosen
SHAPES = [(130, 2, 16, 16, 1), (300, 3, 24, 8, 3), (515, 5, 40, 16, 4), (48, 2, 48, 8, 2)]
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5), 48: (0.08, 0.12, 0.1)}
KEY = (7, 0)


def _pts(a, T, ld=None, fill=0.0):
    """matrix (rows x cols, numpy) -> column-major device tensor (cols, ld); rows beyond `rows` hold `fill`"""
    import torch

    rows, cols = a.shape
    ld = ld or rows
    buf = np.full((cols, ld), fill, dtype=T)
    buf[:, :rows] = np.asarray(a, dtype=T).T
    return torch.from_numpy(buf).to("cuda:0")


def _host(t, rows):
    return t.detach().cpu().numpy()[:, :rows].T.astype(np.float64)


def _vec(a, T):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=T)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _problem(n, rows_x, s, prec):
    """points uniform in the unit cube and right-hand sides, rounded to T; computed once, never modified"""
    T = DT[prec]
    rng = np.random.default_rng(1000 * n)
    X = rng.random((rows_x, n)).astype(T).astype(np.float64)
    H = rng.standard_normal((n, s)).astype(T).astype(np.float64)
    X.setflags(write=False)
    H.setflags(write=False)
    return X, H


def _mus(lockstep, s):
    return [10.0 ** (-3 + i) for i in range(s)] if lockstep else [1e-2]


def _relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _assert_within_model(what, dev_alpha, model_alpha, true_alpha, KS, T):
    """device error <= max(8 x error of model (b), 64 eps_T), for the coefficients and for the fitted values K(:, S) alpha"""
    eps = float(np.finfo(T).eps)
    for name, d, m, t in (("alpha", dev_alpha, model_alpha, true_alpha), ("fitted", KS @ dev_alpha, KS @ model_alpha, KS @ true_alpha)):
        e_dev, e_mod = _relmax(d, t), _relmax(m, t)
        allowed = max(8 * e_mod, 64 * eps)
        print(f"{what} {name}: device error {e_dev:.3g}, model (b) error {e_mod:.3g}, ratio {e_dev / max(e_mod, 1e-300):.3g}, "
              f"error / allowed {e_dev / allowed:.3g}")
        assert e_dev <= allowed, f"{what} {name}: device error {e_dev:.3g} > allowed {allowed:.3g} (model (b): {e_mod:.3g})"


# ---------------------------------------------------------------------------------------------------
# 1. the filter kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("per_column", [False, True])
@pytest.mark.parametrize("k,s", [(1, 1), (17, 3), (64, 1), (257, 5), (1000, 64)])
def test_filter_matches_model(ctx, k, s, per_column, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(k + s)
    sigma = np.sort(rng.random(k) * 3 + 1e-3)[::-1].astype(T)
    mus = (10.0 ** rng.uniform(-6, 1, s if per_column else 1)).astype(T)
    Ch = rng.standard_normal((k, s)).astype(T)
    want = rm.ridge_filter(Ch, sigma, mus, 0.5)                              # mu > 0: rcond = 0.5 must cut nothing
    Cd = _pts(Ch, T, k + 3, fill=np.nan)
    dev.ridge_filter(ctx, _vec(sigma, T), _vec(mus, T), Cd, k, s, rcond=0.5, ldc=k + 3)
    got = Cd.cpu().numpy()
    assert np.all(np.isnan(got[:, k:]))                                      # the rows of C past k are not touched
    got = got[:, :k].T.astype(np.longdouble)
    ratio = float(np.max(np.abs(got - want) / np.abs(want)) / eps)
    print(f"filter k={k} s={s} per_column={per_column} {prec}: max error {ratio:.3g} eps")
    assert ratio <= 2.0


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_filter_pseudo_inverse_cut_off(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    k, s = 40, 3
    sigma = (10.0 ** -np.arange(k, dtype=np.float64) * 0.5).astype(T)      # 1 .. 1e-19.5, decreasing
    sigma[0] = 1
    rcond = 1e-6
    below = sigma.astype(np.float64) <= rcond * float(sigma[0])
    assert below.any() and not below.all()
    Ch = np.random.default_rng(1).standard_normal((k, s)).astype(T)
    # mu = 0 for every column
    Cd = _pts(Ch, T)
    dev.ridge_filter(ctx, _vec(sigma, T), _vec([0.0], T), Cd, k, s, rcond=rcond)
    got = _host(Cd, k)
    assert np.all(got[below, :] == 0) and np.all(np.isfinite(got)) and np.all(got[~below, :] != 0)
    want = rm.ridge_filter(Ch, sigma, np.zeros(1, dtype=T), rcond).astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * eps * np.abs(want))
    # per column: mu = 0 cuts, mu > 0 cuts nothing although rcond = 1 says every sigma below sigma_0 is small
    mus = np.array([0.0, 1e-3, 0.0], dtype=T)
    Cd = _pts(Ch, T)
    dev.ridge_filter(ctx, _vec(sigma, T), _vec(mus, T), Cd, k, s, rcond=1.0)
    got = _host(Cd, k)
    assert np.all(got[:, 0] == 0) and np.all(got[:, 2] == 0)                 # sigma_j <= 1 * sigma_0 for every j, sigma_0 itself included
    want = rm.ridge_filter(Ch, sigma, mus, 1.0).astype(np.float64)
    big = sigma.astype(np.float64) ** 2 > 1e-30                              # below that sigma / (sigma^2 + mu) underflows towards denormals in fp32
    assert np.all(got[big, 1] != 0) and np.all(np.abs(got[big, 1] - want[big, 1]) <= 2 * eps * np.abs(want[big, 1]))
    # rcond = 0 and sigma_j = 0: the factor is 0, not 0 / 0
    z = np.array([1.0, 0.0], dtype=T)
    Cd = _pts(np.ones((2, 1)), T)
    dev.ridge_filter(ctx, _vec(z, T), _vec([0.0], T), Cd, 2, 1, rcond=0.0)
    assert _host(Cd, 2)[:, 0].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_filter_empty_shapes_and_argument_codes(ctx, prec):
    import torch

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    k, s = 5, 3
    sigma = torch.ones(k, dtype=dt, device="cuda:0")
    mus = torch.ones(s, dtype=dt, device="cuda:0")
    Cm = torch.full((s, k), 7.0, dtype=dt, device="cuda:0")
    fn = getattr(ctx.lib, f"rlhip_ridge_filter_{prec}")
    good = dict(k=k, s=s, sigma=sigma.data_ptr(), mus=mus.data_ptr(), num_mus=s, rcond=0.0, C=Cm.data_ptr(), ldc=k)

    def call(**kw):
        a = dict(good, **kw)
        return fn(ctx.h, a["k"], a["s"], a["sigma"], a["mus"], a["num_mus"], ct(a["rcond"]), a["C"], a["ldc"])

    bad = [(dict(k=-1), -2), (dict(s=-1), -3), (dict(sigma=None), -4), (dict(mus=None), -5), (dict(num_mus=2), -100), (dict(num_mus=0), -100),
           (dict(rcond=-1.0), -7), (dict(rcond=float("nan")), -7), (dict(C=None), -8), (dict(ldc=k - 1), -9), (dict(k=0, ldc=0), -9)]
    for kw, code in bad:
        assert call(**kw) == code, kw
    assert fn(None, k, s, sigma.data_ptr(), mus.data_ptr(), s, ct(0.0), Cm.data_ptr(), k) == -1
    # k == 0 or s == 0: nothing is touched, NULL arrays are no error
    assert call(k=0, ldc=1) == 0 and call(s=0) == 0 and call(k=0, ldc=1, sigma=None, mus=None, C=None) == 0
    assert call(s=0, sigma=None, mus=None, C=None, num_mus=7) == 0
    torch.cuda.synchronize()
    assert bool((Cm == 7.0).all())
    assert call(num_mus=1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((Cm == 7.0 / 4.0).all())                                     # twice 1 / (1 + 1), exactly


# ---------------------------------------------------------------------------------------------------
# 2. the fit on the pivots of randomly pivoted Cholesky, and with the same centres given
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(n, rows_x, k, b, s, kind, lockstep, prec, S):
    """the dense solve (a) and the model (b) in T on the centres S (a tuple: the device's); computed once, never modified"""
    T = DT[prec]
    X, H = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    mus = np.asarray(_mus(lockstep, s), dtype=T).astype(np.float64)
    Sa = np.array(S, dtype=np.int64)
    true_alpha, KS = rm.truth(kind, X, l, Sa, mus, H)
    blocks = [Sa[p:p + b] for p in range(0, Sa.size, b)]      # a pivoted Cholesky factor depends on the order of the pivots only
    f = rm.factor(kind, X, l, Sa.size, b, T, forced_S=blocks)
    assert f["k"] == Sa.size and np.array_equal(f["S"], Sa)
    model_alpha = rm.algorithm(f["F"], Sa, mus, H, T)["alpha"].astype(np.float64)
    cond = float(np.linalg.cond(KS[Sa, :]))
    for a in (true_alpha, KS, model_alpha):
        a.setflags(write=False)
    return true_alpha, KS, model_alpha, cond


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("lockstep", [True, False], ids=["lockstep", "single_mu"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit(ctx, shape, kind, lockstep, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, H = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    mus = _mus(lockstep, s)
    padded = n == 515                                                        # ldx, ldh and ldalpha larger than the sizes
    Pd = _pts(X, T, rows_x + 2 if padded else None, fill=1e30)
    Hd = _pts(H, T, n + 5 if padded else None, fill=1e30)
    r = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY, ldalpha=k + 3 if padded else None)
    assert r["k"] == k and r["c_status"] == 0 and r["status"] == (1 if k == n else 0)       # k = n: the residual diagonal is exhausted afterwards
    S = r["S"]
    assert len(set(S.tolist())) == k
    # the pivots are those of rp_cholesky on the same operator, state and block size; the model replays them
    rp = dev.drv_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, k, b, key=KEY)
    assert np.array_equal(S, rp["S"]) and r["next_ctr"] == rp["next_ctr"] and (rp["status"], rp["c_status"]) == (r["status"], r["c_status"])
    true_alpha, KS, model_alpha, cond = _reference(n, rows_x, k, b, s, kind, lockstep, prec, tuple(S.tolist()))
    print(f"cond(K_SS) = {cond:.3g}")
    assert cond <= 1e3
    raw = r["alpha"].cpu().numpy()
    if padded:
        assert np.all(np.isnan(raw[:, k:]))                                  # rows of alpha past k are not written
    alpha = raw[:, :k].T.astype(np.float64)
    what = f"fit {shape} kind={kind} {'lockstep' if lockstep else 'single mu'} {prec}"
    _assert_within_model(what, alpha, model_alpha, true_alpha, KS, T)
    if k == n:                                                               # the identity with the full fit, in pivot order
        K = pk.cross_kernel(kind, X, X, l)
        mu_t = np.broadcast_to(np.asarray(mus, dtype=T).astype(np.float64), (s,))
        full = np.stack([np.linalg.solve(K + mu * np.eye(n), H[:, i]) for i, mu in enumerate(mu_t)], axis=1)
        if kind == pk.SQEXP:
            assert np.allclose(full, km.fit(X, l, mu_t, H), rtol=1e-10, atol=0)
        _assert_within_model(what + " against the full fit", alpha, model_alpha, full[S, :], KS, T)
    # the same centres given: the same coefficients within the same bound
    info, a2 = dev.krill_restricted_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, S)
    assert info == 0
    f2, info_m = rm.given_centres_factor(kind, X, l, S, T)
    assert info_m == 0
    model2 = rm.algorithm(f2, S, np.asarray(mus, dtype=T).astype(np.float64), H, T)["alpha"].astype(np.float64)
    _assert_within_model(what + " given centres", a2.cpu().numpy()[:, :k].T.astype(np.float64), model2, true_alpha, KS, T)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_given_centres_with_a_repeated_centre(ctx, prec):
    """S[1] = S[0]: the second pivot of K(S, S) is 1 - 1 * 1 = 0 exactly, so potrf reports position 2 whatever its summation order"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = SHAPES[1]
    X, H = _problem(n, rows_x, s, prec)
    S = np.arange(5, 5 + k, dtype=np.int64)
    S[1] = S[0]
    info, alpha = dev.krill_restricted_pdk(ctx, _pts(X, T), rows_x, n, pk.MATERN32, 0.25, [1e-2], _pts(H, T), s, S)
    assert info == 2
    assert bool(np.all(np.isnan(alpha.cpu().numpy())))                       # alpha, handed in full of NaN, is untouched


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_achieved_rank_below_the_request(ctx, prec):
    """64 points of which 32 are exact duplicates, 48 centres asked for: the factorization stops at 32 or fewer and reports why; the fit is made
    on what it achieved and the rest of alpha and S is cleared.  (Two copies of one point drawn in the same block can both be kept when the
    second pivot rounds to a tiny positive number -- rp_cholesky's own behaviour, which this feature does not change -- so the coefficients
    are only required to be finite here; their accuracy is test_fit's subject.)"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = 64, 2, 48, 8, 2
    rng = np.random.default_rng(64)
    base = rng.random((rows_x, 32)).astype(T).astype(np.float64)
    X = np.concatenate([base, base], axis=1)[:, rng.permutation(n)]
    H = rng.standard_normal((n, s)).astype(T).astype(np.float64)
    kind, l, mus = pk.MATERN52, 0.1, [1e-2, 1e-1]
    r = dev.krill_restricted_rpchol_pdk(ctx, _pts(X, T), rows_x, n, kind, l, mus, _pts(H, T), s, k=k, b=b, key=KEY)
    ko = r["k"]
    print(f"achieved rank {ko} of {k}: w_status {r['status']}, c_status {r['c_status']}")
    assert 1 <= ko <= 32 and (r["status"] != 0 or r["c_status"] != 0)
    assert np.all(r["S_all"][ko:] == -1) and len(set(r["S"].tolist())) == ko and np.all((r["S"] >= 0) & (r["S"] < n))
    raw = r["alpha"].cpu().numpy()
    assert np.all(raw[:, ko:] == 0) and np.all(np.isfinite(raw[:, :ko]))
    # the factorization is rp_cholesky's: the same pivots, rank and codes as the driver of the factorization alone
    rp = dev.drv_rpchol_pdk(ctx, _pts(X, T), rows_x, n, kind, l, k, b, key=KEY)
    assert np.array_equal(r["S"], rp["S"]) and (rp["k"], rp["status"], rp["c_status"]) == (ko, r["status"], r["c_status"])


# ---------------------------------------------------------------------------------------------------
# 3. prediction
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("mz", [1, 70])
@pytest.mark.parametrize("k", [16, 40])
def test_predict_restricted_matches_krr_predict(ctx, k, mz, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    n, rows_x, s = 515, 5, 4
    X, _ = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    rng = np.random.default_rng(k + mz)
    S = rng.permutation(n)[:k].astype(np.int64)
    alpha = rng.standard_normal((k, s)).astype(T).astype(np.float64)
    Z = rng.random((rows_x, mz)).astype(T).astype(np.float64)
    full = np.zeros((n, s))
    full[S, :] = alpha                                                       # the n x s coefficient block that is zero off S
    Pd, Zd = _pts(X, T, rows_x + 2), _pts(Z, T)
    want_dev = _host(dev.krr_predict_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, _pts(full, T), s), mz)
    before = [ctx.rbf_path_count(w) for w in (55, 56, 57)]
    got = _host(dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, _pts(alpha, T, k + 1), s), mz)
    assert [ctx.rbf_path_count(w) - c for w, c in zip((55, 56, 57), before)] == [1, 0, 0]     # one fused cross apply, nothing else
    want, mag = rm.predict(kind, Z, X, l, S, alpha)
    bound = 64 * eps * mag
    for name, ref in (("krr_predict on the zero-padded block", want_dev), ("the model", want)):
        err = np.abs(got - ref)
        print(f"predict k={k} mz={mz} kind={kind} {prec} against {name}: max error / bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------
# 4. the existing entries keep their bits on a context that has run restricted fits
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_full_fit_and_predict_are_bit_identical_around_a_restricted_fit(ctx, prec):
    """the fit-then-predict problem of tests/test_gpu_krr.py (lockstep), before and after restricted work on the same context"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, h, k, blk, s, mz = 1000, 5, 3.0, 128, 16, 3, 130
    pts = np.random.default_rng(2).standard_normal((rows_x, n)).astype(T).astype(np.float64)
    mus = (1e-2, 1e-1, 1.0)
    G = pm.reg_op(pm.rbf_kernel(pts, h, np.float64), mus, np.float64)
    H = G(np.random.default_rng(101).standard_normal((n, s)).astype(T))
    Zh = np.random.default_rng(303).standard_normal((rows_x, mz)).astype(T).astype(np.float64)
    tol = 100 * float(np.finfo(T).eps)
    Pd, Hd, Zd = _pts(pts, T), _pts(H, T), _pts(Zh, T)

    def full():
        r = dev.krill_full_rpchol_rbf(ctx, Pd, rows_x, n, h, list(mus), Hd, _pts(np.zeros_like(H), T), s, tol, 40, k=k, b=blk, key=(7, 0))
        Y = dev.krr_predict(ctx, Zd, mz, Pd, rows_x, n, h, r["X"], s)
        return r["X"].cpu().numpy(), Y.cpu().numpy(), r["iters"], r["next_ctr"]

    first = full()
    r = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, dev.PDK_MATERN32, h, list(mus), Hd, s, k=40, b=blk, key=(9, 0))
    assert r["k"] == 40
    dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, dev.PDK_MATERN32, h, r["S"], r["alpha"], s)
    info, _ = dev.krill_restricted_pdk(ctx, Pd, rows_x, n, dev.PDK_MATERN32, h, [1e-2], Hd, s, r["S"])
    assert info == 0
    second = full()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2:] == second[2:]


# ---------------------------------------------------------------------------------------------------
# 5. what the drivers refuse
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_drivers_refuse_an_unknown_kernel_and_bad_arguments(ctx, prec):
    from randlapack_amd import device as dev
    from randlapack_amd._lib import RlhipError
    import torch

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    n, rows_x, k, b, s = SHAPES[0]
    X, H = _problem(n, rows_x, s, prec)
    Pd, Hd = _pts(X, T), _pts(H, T)
    alpha = torch.full((s, k), 5.0, dtype=Pd.dtype, device="cuda:0")
    S = np.arange(k, dtype=np.int64)
    Sp = S.ctypes.data_as(C.POINTER(C.c_int64))
    rg = (ct * 1)(1e-2)
    kk, info = C.c_int64(k), C.c_int64(0)
    st, status = (C.c_uint32 * 6)(), (C.c_int * 2)()
    for kernel in (-1, 3):
        assert getattr(ctx.lib, f"rlhip_drv_krill_restricted_rpchol_pdk_{prec}")(ctx.h, Pd.data_ptr(), rows_x, rows_x, n, kernel, ct(0.2), rg, 1, Hd.data_ptr(), n,
                                                                                s, C.byref(kk), b, Sp, alpha.data_ptr(), k, st, status) == -6
        assert getattr(ctx.lib, f"rlhip_drv_krill_restricted_pdk_{prec}")(ctx.h, Pd.data_ptr(), rows_x, rows_x, n, kernel, ct(0.2), rg, 1, Hd.data_ptr(), n, s, k,
                                                                         Sp, alpha.data_ptr(), k, C.byref(info)) == -6
        assert getattr(ctx.lib, f"rlhip_drv_krr_predict_restricted_pdk_{prec}")(ctx.h, rows_x, n, Pd.data_ptr(), rows_x, n, Pd.data_ptr(), rows_x, kernel, ct(0.2),
                                                                               k, Sp, s, alpha.data_ptr(), k, Hd.data_ptr(), n) == -9
    assert bool((alpha == 5.0).all()) and kk.value == k
    with pytest.raises(RlhipError):                                          # two regularizations for one right-hand side
        dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, 0, 0.2, [1e-2, 1e-1], Hd, s, k=k, b=b)
    with pytest.raises(RlhipError):                                          # more centres than points
        dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, 0, 0.2, [1e-2], Hd, s, k=n + 1, b=b)
    with pytest.raises(RlhipError):                                          # a negative regularization
        dev.krill_restricted_pdk(ctx, Pd, rows_x, n, 0, 0.2, [-1e-2], Hd, s, S)
    with pytest.raises(RlhipError):                                          # a centre that is no point
        dev.krill_restricted_pdk(ctx, Pd, rows_x, n, 0, 0.2, [1e-2], Hd, s, np.array([0, n]))
    with pytest.raises(RlhipError):
        dev.krr_predict_restricted_pdk(ctx, Pd, n, Pd, rows_x, n, 0, 0.2, np.array([0, -1]), alpha, s)
    # the operator is usable afterwards: a good call on the same context
    r = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, 0, 0.12, [1e-2], Hd, s, k=k, b=b, key=KEY)
    assert r["k"] == k
