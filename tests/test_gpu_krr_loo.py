"""The regularization path of restricted kernel ridge regression on the device: rlhip_ridge_loo_* against the extended-precision
model of tests/_krr_loo_model.py, and krill_restricted_rpchol_cv / krill_restricted_cv through their C entries in fp64 and fp32, for the
three kernel kinds and both criteria.

Tolerances.  The kernel: every entry of loo and rss within the model's first-order running-error bound for sums of k terms in double in any
order (tests/_krr_loo_model.py derives it); inputs of type float are exact in double, so both precisions share it.  The drivers: the
device's table against the float64 model on the device's own centres may be off by 8 times the error of the numpy model of the same
algorithm in T, with a floor of 64 eps_T, both relative to the column's largest entry -- the rule of tests/test_gpu_krr_restricted.py, for
the same reason: another SVD and another summation order.  The selection is checked on the columns whose gap to the runner-up is at least
100 times that allowance; tests/test_krr_loo_model.py shows that every column of these inputs is one.  alpha and S are bit-identical to
the existing fits called with the selected values.  The largest measured fractions are in DESIGN 4.26."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import _krr_loo_model as lm
import _krr_restricted_model as rm
import _pdk_model as pk

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
SHAPES = [(130, 2, 16, 16, 1), (300, 3, 24, 8, 3), (515, 5, 40, 16, 4)]      # tests/test_gpu_krr_restricted.py without its k = n row
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5), 48: (0.08, 0.12, 0.1)}
KEY = (7, 0)
GOLDEN = Path(__file__).resolve().parent / "golden" / "krr_restricted_bits.json"
# the kernel's chunk boundaries (pcg.hip): rows per workgroup, columns of U per LDS slab, grid values per chunk, right-hand sides per chunk
LOO_ROWS, LOO_JS, LOO_GC, LOO_LC = 256, 64, 8, 4
KERNEL_SHAPES = [(1, 1, 1, 1), (63, 5, 1, 3), (257, 17, 3, 8), (1000, 64, 1, 33), (515, 130, 4, 65),
                 (LOO_ROWS + 1, LOO_JS + 1, LOO_LC + 1, LOO_GC + 1)]


def _pts(a, T, ld=None, fill=0.0):
    """matrix (rows x cols, numpy) -> column-major device tensor (cols, ld); rows beyond `rows` hold `fill`"""
    import torch

    rows, cols = a.shape
    ld = ld or rows
    buf = np.full((cols, ld), fill, dtype=T)
    buf[:, :rows] = np.asarray(a, dtype=T).T
    return torch.from_numpy(buf).to("cuda:0")


def _vec(a, T):
    import torch

    return torch.from_numpy(np.array(a, dtype=T)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _kernel_inputs(n, k, ell, g, prec):
    """U from a QR of a random matrix, sigma decreasing, C and H, mus log-uniform in 1e-6 .. 10, all rounded to T; never modified"""
    T = DT[prec]
    rng = np.random.default_rng(1000 * n + 10 * k + ell + g)
    U = np.linalg.qr(rng.standard_normal((n, k)))[0].astype(T)
    sigma = np.sort(rng.random(k) * 3 + 1e-3)[::-1].astype(T)
    Cm = rng.standard_normal((k, ell)).astype(T)
    H = rng.standard_normal((n, ell)).astype(T)
    mus = (10.0 ** rng.uniform(-6, 1, g)).astype(T)
    for a in (U, sigma, Cm, H, mus):
        a.setflags(write=False)
    return U, sigma, Cm, H, mus


def _run_kernel(ctx, prec, U, sigma, Cm, H, mus, rcond=0.0, pad=False):
    """(loo, rss) as float64 g x ell arrays, through the C entry; pad: leading dimensions larger than the sizes with NaN behind them, which
    must still be there afterwards, as must the NaN behind the two outputs"""
    import torch

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    (n, k), ell, g = U.shape, H.shape[1], mus.size
    ldu, ldc, ldh = (n + 3, k + 2, n + 1) if pad else (n, k, n)
    Ud, Cd, Hd = _pts(U, T, ldu, np.nan), _pts(Cm, T, ldc, np.nan), _pts(H, T, ldh, np.nan)
    sd, md = _vec(sigma, T), _vec(mus, T)
    out = torch.full((2, g * ell + 4), float("nan"), dtype=torch.float64, device="cuda:0")
    rc = getattr(ctx.lib, f"rlhip_ridge_loo_{prec}")(ctx.h, n, k, ell, g, Ud.data_ptr(), ldu, sd.data_ptr(), Cd.data_ptr(), ldc, Hd.data_ptr(), ldh,
                                                    md.data_ptr(), ct(rcond), out[0].data_ptr(), out[1].data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(np.isnan(o[:, g * ell:]))
    if pad:
        assert np.all(np.isnan(Ud.cpu().numpy()[:, n:])) and np.all(np.isnan(Cd.cpu().numpy()[:, k:])) and np.all(np.isnan(Hd.cpu().numpy()[:, n:]))
    return o[0, :g * ell].reshape(ell, g).T, o[1, :g * ell].reshape(ell, g).T


def _assert_within_bound(what, got, model):
    worst = 0.0
    for name, have in zip(("loo", "rss"), got):
        want, bound = model[name], model["bound_" + name]
        frac = float(np.max(np.abs(have.astype(lm.L) - want) / bound))
        worst = max(worst, frac)
        print(f"{what} {name}: largest error / bound = {frac:.3g}")
        assert np.all(np.abs(have.astype(lm.L) - want) <= bound), f"{what} {name}: error / bound = {frac:.3g}"
    return worst


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_model(ctx, shape, prec):
    U, sigma, Cm, H, mus = _kernel_inputs(*shape, prec)
    model = lm.table(U, sigma, Cm, H, mus)
    got = _run_kernel(ctx, prec, U, sigma, Cm, H, mus, pad=shape[0] in (257, 515))
    _assert_within_bound(f"kernel {shape} {prec}", got, model)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_wrapper_and_mu_zero_with_sigma_around_the_cut(ctx, prec):
    """mu == 0: d_j is 1 above rcond sigma_0 and 0 at or below it; the other grid values cut nothing.  Through the Python wrapper."""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, k, ell = 70, 12, 2
    U, _, Cm, H, _ = _kernel_inputs(n, k, ell, 3, prec)
    sigma = (10.0 ** -np.arange(k, dtype=np.float64)).astype(T)
    rcond = float(T(1e-6))
    d = lm.d_factor(sigma, [0.0], rcond)[:, 0]
    assert d.min() == 0 and d.max() == 1 and d.sum() == 6                    # sigma_6 = rcond sigma_0 itself is cut
    mus = np.array([0.0, 1e-3, 0.0], dtype=T)
    loo, rss = dev.ridge_loo(ctx, _pts(U, T), _vec(sigma, T), _pts(Cm, T), _pts(H, T), _vec(mus, T), n, k, ell, rcond=rcond)
    got = (loo.cpu().numpy().T, rss.cpu().numpy().T)
    _assert_within_bound(f"mu = 0 {prec}", got, lm.table(U, sigma, Cm, H, mus, rcond))
    uncut = lm.table(U, sigma, Cm, H, mus, 0.0)
    assert np.all(np.abs(got[1][0].astype(lm.L) - uncut["rss"][0]) > 100 * uncut["bound_rss"][0])     # the cut is not a rounding matter
    assert np.array_equal(got[0][0], got[0][2]) and np.array_equal(got[1][0], got[1][2])               # the same mu, the same bits


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_reports_a_leverage_of_one_as_it_is(ctx, prec):
    """n = k = 1, U = 1, mu = 0: s = 1 exactly, the residual h - c is not 0: loo is inf, rss finite; with h = c both are 0 / 0 and 0"""
    one = np.ones((1, 1))
    loo, rss = _run_kernel(ctx, prec, one, np.ones(1), 3 * one, 2 * one, np.array([0.0, 1.0]))
    assert np.isinf(loo[0, 0]) and rss[0, 0] == 1.0 and loo[1, 0] == 1.0 and rss[1, 0] == 0.25
    loo, rss = _run_kernel(ctx, prec, one, np.ones(1), 2 * one, 2 * one, np.array([0.0]))
    assert np.isnan(loo[0, 0]) and rss[0, 0] == 0.0


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_bits_are_reproducible(prec):
    """two calls, and a call after a larger one has grown the scratch arena of a fresh context"""
    from randlapack_amd.device import Context

    c = Context(0)
    try:
        args = _kernel_inputs(515, 130, 4, 65, prec)
        a = _run_kernel(c, prec, *args)
        b = _run_kernel(c, prec, *args)
        big = _kernel_inputs(4100, 3, 16, 256, prec)                         # 2 * 17 * 256 * 16 partial sums: 1.1 MB of scratch
        _run_kernel(c, prec, *big)
        d = _run_kernel(c, prec, *args)
    finally:
        c.close()
    for x, y, z in zip(a, b, d):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kernel_empty_shapes_and_argument_codes(ctx, prec):
    import torch

    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    n, k, ell, g = 9, 4, 2, 3
    U = torch.full((k, n), 0.5, dtype=dt, device="cuda:0")
    sg = torch.ones(k, dtype=dt, device="cuda:0")
    Cm = torch.ones((ell, k), dtype=dt, device="cuda:0")
    H = torch.full((ell, n), 2.0, dtype=dt, device="cuda:0")
    mus = torch.ones(g, dtype=dt, device="cuda:0")
    out = torch.full((2, g * ell), 7.0, dtype=torch.float64, device="cuda:0")
    fn = getattr(ctx.lib, f"rlhip_ridge_loo_{prec}")
    good = dict(n=n, k=k, ell=ell, g=g, U=U.data_ptr(), ldu=n, sigma=sg.data_ptr(), C=Cm.data_ptr(), ldc=k, H=H.data_ptr(), ldh=n, mus=mus.data_ptr(),
                rcond=0.0, loo=out[0].data_ptr(), rss=out[1].data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return fn(ctx.h, a["n"], a["k"], a["ell"], a["g"], a["U"], a["ldu"], a["sigma"], a["C"], a["ldc"], a["H"], a["ldh"], a["mus"], ct(a["rcond"]),
                  a["loo"], a["rss"])

    bad = [(dict(n=-1), -2), (dict(k=-1), -3), (dict(ell=-1), -4), (dict(g=-1), -5), (dict(U=None), -6), (dict(ldu=n - 1), -7), (dict(sigma=None), -8),
           (dict(C=None), -9), (dict(ldc=k - 1), -10), (dict(H=None), -11), (dict(ldh=n - 1), -12), (dict(mus=None), -13), (dict(rcond=-1.0), -14),
           (dict(rcond=float("nan")), -14), (dict(loo=None), -15), (dict(rss=None), -16), (dict(n=0, ldu=0), -7), (dict(k=0, ldc=0), -10)]
    for kw, code in bad:
        assert call(**kw) == code, kw
    assert fn(None, n, k, ell, g, U.data_ptr(), n, sg.data_ptr(), Cm.data_ptr(), k, H.data_ptr(), n, mus.data_ptr(), ct(0.0), out[0].data_ptr(),
              out[1].data_ptr()) == -1
    # an empty shape: nothing is touched, NULL arrays are no error
    nulls = dict(U=None, sigma=None, C=None, H=None, mus=None, loo=None, rss=None)
    for kw in (dict(n=0), dict(k=0), dict(ell=0), dict(g=0)):
        assert call(**kw) == 0 and call(**dict(nulls, **kw)) == 0, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    # every d is 1 / 2: s = 4 * 0.25 / 2 = 0.5, yhat = 4 * 0.5 / 2 = 1, residual 1 and leave-one-out residual 2 on each of the 9 rows, exactly
    assert bool((out[1] == 9.0).all()) and bool((out[0] == 36.0).all())


# ---------------------------------------------------------------------------------------------------
# 2. the fits that choose from the grid
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(n, rows_x, k, b, s, kind, prec, S):
    """the float64 model and the model in T on the centres S (a tuple: the device's); computed once, never modified"""
    T = DT[prec]
    X, H = lm.problem(n, rows_x, s, T)
    l = BANDWIDTH[n][kind]
    Sa = np.array(S, dtype=np.int64)
    blocks = [Sa[p:p + b] for p in range(0, Sa.size, b)]
    f64 = rm.factor(kind, X, l, Sa.size, b, np.float64, forced_S=blocks)
    fT = rm.factor(kind, X, l, Sa.size, b, T, forced_S=blocks)
    assert np.array_equal(fT["S"], Sa)
    return lm.path(f64["F"], H, lm.GRID, np.float64, n_for_rcond=n), lm.path(fT["F"], H, lm.GRID, T)


def _check_path(what, r, n, crit, p64, pT, T):
    """tables within the allowance, best equal to the model's on every column with a clear runner-up; returns the number of such columns"""
    eps = float(np.finfo(T).eps)
    allowed = {}
    for name in ("loo", "rss"):
        t64, tT, td = p64[name].astype(np.float64), pT[name].astype(np.float64), r[name].T
        colmax = np.max(np.abs(t64), axis=0)
        e_dev, e_mod = np.max(np.abs(td - t64), axis=0) / colmax, np.max(np.abs(tT - t64), axis=0) / colmax
        allowed[name] = np.maximum(8 * e_mod, 64 * eps)
        print(f"{what} {name}: device error {e_dev}, model-T error {e_mod}, error / allowed {e_dev / allowed[name]}")
        assert np.all(e_dev <= allowed[name]), f"{what} {name}: device error {e_dev} > allowed {allowed[name]}"
    assert np.allclose(r["dof"], p64["dof"], rtol=max(64 * eps, 8 * float(np.max(np.abs(pT["dof"] - p64["dof"]) / p64["dof"]))), atol=0)
    c64 = lm.criterion(crit, n, p64["loo"], p64["rss"], p64["dof"])
    best, gaps = lm.select(c64), lm.runner_up_gap(c64)
    used = gaps >= 100 * allowed["loo" if crit == lm.LOO else "rss"]
    assert np.array_equal(r["best"][used], best[used]), f"{what}: best {r['best']} against the model's {best} on the columns {used}"
    # the selection is the rule applied to the device's own table, on every column
    own = lm.select(lm.criterion(crit, n, r["loo"].T, r["rss"].T, r["dof"]))
    assert np.array_equal(r["best"], own) and np.array_equal(r["best_mu"], np.asarray(lm.GRID, dtype=T).astype(np.float64)[own])
    return int(used.sum())


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("crit", [lm.LOO, lm.GCV], ids=["loo", "gcv"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit_with_selection(ctx, shape, kind, crit, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, H = lm.problem(n, rows_x, s, T)
    l = BANDWIDTH[n][kind]
    padded = n == 515
    Pd = _pts(X, T, rows_x + 2 if padded else None, fill=1e30)
    Hd = _pts(H, T, n + 5 if padded else None, fill=1e30)
    r = dev.krill_restricted_rpchol_cv_pdk(ctx, Pd, rows_x, n, kind, l, lm.GRID, crit, Hd, s, k=k, b=b, key=KEY, ldalpha=k + 3 if padded else None)
    assert r["k"] == k and r["c_status"] == 0 and r["status"] == 0
    S = r["S"]
    p64, pT = _reference(n, rows_x, k, b, s, kind, prec, tuple(S.tolist()))
    what = f"cv fit {shape} kind={kind} crit={crit} {prec}"
    assert _check_path(what, r, n, crit, p64, pT, T) >= 1
    # the existing fit with the selected values: the same centres, state and coefficients, bit for bit
    e = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, [float(m) for m in r["best_mu"]], Hd, s, k=k, b=b, key=KEY,
                                        ldalpha=k + 3 if padded else None)
    assert np.array_equal(S, e["S"]) and r["next_ctr"] == e["next_ctr"]
    assert np.array_equal(r["alpha"].cpu().numpy(), e["alpha"].cpu().numpy(), equal_nan=True)
    # the centres given
    info, a2, path2 = dev.krill_restricted_cv_pdk(ctx, Pd, rows_x, n, kind, l, lm.GRID, crit, Hd, s, S)
    assert info == 0
    f2 = rm.given_centres_factor(kind, X, l, S, T)[0]
    f2_64 = rm.given_centres_factor(kind, X, l, S, np.float64)[0]
    assert _check_path(what + " given centres", path2, n, crit, lm.path(f2_64, H, lm.GRID, np.float64, n_for_rcond=n), lm.path(f2, H, lm.GRID, T), T) >= 1
    info, a3 = dev.krill_restricted_pdk(ctx, Pd, rows_x, n, kind, l, [float(m) for m in path2["best_mu"]], Hd, s, S)
    assert info == 0 and np.array_equal(a2.cpu().numpy(), a3.cpu().numpy())


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_existing_fits_keep_the_bits_they_had(ctx, prec):
    """krill_restricted_rpchol and krill_restricted on one case recorded on an MI355X before restricted_tail was split (tests/golden/)"""
    from randlapack_amd import device as dev

    T = DT[prec]
    gold = json.loads(GOLDEN.read_text())[prec]
    n, rows_x, k, b, s = SHAPES[1]
    X, H = lm.problem(n, rows_x, s, T)
    Pd, Hd = _pts(X, T), _pts(H, T)
    view = np.uint64 if prec == "f64" else np.uint32
    r = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, pk.MATERN52, 0.25, [1e-3, 1e-2, 1e-1], Hd, s, k=k, b=b, key=KEY)
    assert r["S"].tolist() == gold["S"]
    assert r["alpha"].cpu().numpy().view(view).ravel().tolist() == gold["alpha_rpchol"]
    info, a = dev.krill_restricted_pdk(ctx, Pd, rows_x, n, pk.MATERN52, 0.25, [1e-2], Hd, s, r["S"])
    assert info == 0 and a.cpu().numpy().view(view).ravel().tolist() == gold["alpha_given"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_selection_after_an_early_stop(ctx, prec):
    """the 48 points of tests/test_gpu_krr_restricted.py with 24 of them duplicated, 48 centres asked for: the factorization stops early, the
    path is that of the achieved rank and the fit is the existing one with the selected values"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = 48, 2, 48, 8, 2
    rng = np.random.default_rng(1000 * n)
    base = rng.random((rows_x, 24)).astype(T).astype(np.float64)
    X = np.concatenate([base, base], axis=1)[:, rng.permutation(n)]
    H = lm.targets(X, s, T, rng)
    kind, l = pk.MATERN52, BANDWIDTH[n][2]
    Pd, Hd = _pts(X, T), _pts(H, T)
    r = dev.krill_restricted_rpchol_cv_pdk(ctx, Pd, rows_x, n, kind, l, lm.GRID, lm.LOO, Hd, s, k=k, b=b, key=KEY)
    ko = r["k"]
    print(f"achieved rank {ko} of {k}: w_status {r['status']}, c_status {r['c_status']}, best {r['best']}, loo {r['loo']}")
    assert 1 <= ko < k and (r["status"] != 0 or r["c_status"] != 0)
    assert np.all(r["S_all"][ko:] == -1) and np.all(np.isfinite(r["loo"])) and np.all(r["loo"] > 0) and np.all(r["dof"] <= ko)
    assert np.array_equal(r["best"], lm.select(r["loo"].T))
    e = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, [float(m) for m in r["best_mu"]], Hd, s, k=k, b=b, key=KEY)
    assert e["k"] == ko and np.array_equal(r["alpha"].cpu().numpy(), e["alpha"].cpu().numpy())
    assert np.all(r["alpha"].cpu().numpy()[:, ko:] == 0)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_drivers_refuse_invalid_calls(ctx, prec):
    from randlapack_amd import device as dev
    from randlapack_amd._lib import RlhipError
    import torch

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    n, rows_x, k, b, s = SHAPES[0]
    X, H = lm.problem(n, rows_x, s, T)
    Pd, Hd = _pts(X, T), _pts(H, T)
    S = np.arange(k, dtype=np.int64)
    for grid in ([], [1e-2, -1e-3]):                                         # an empty grid, a negative grid value
        with pytest.raises(RlhipError):
            dev.krill_restricted_rpchol_cv_pdk(ctx, Pd, rows_x, n, 0, 0.2, grid, lm.LOO, Hd, s, k=k, b=b)
        with pytest.raises(RlhipError):
            dev.krill_restricted_cv_pdk(ctx, Pd, rows_x, n, 0, 0.2, grid, lm.GCV, Hd, s, S)
    with pytest.raises(RlhipError):                                          # an unknown criterion
        dev.krill_restricted_cv_pdk(ctx, Pd, rows_x, n, 0, 0.2, [1e-2], 2, Hd, s, S)
    # null buffers and an unknown kernel kind, through the C entries
    alpha = torch.full((s, k), 5.0, dtype=Pd.dtype, device="cuda:0")
    Sp = S.ctypes.data_as(C.POINTER(C.c_int64))
    mg = (ct * 2)(1e-2, 1e-1)
    kk, info = C.c_int64(k), C.c_int64(0)
    st, status = (C.c_uint32 * 6)(), (C.c_int * 2)()
    f1 = getattr(ctx.lib, f"rlhip_drv_krill_restricted_rpchol_cv_pdk_{prec}")
    f2 = getattr(ctx.lib, f"rlhip_drv_krill_restricted_cv_pdk_{prec}")

    def rp(kernel=0, grid=mg, Hp=Hd.data_ptr(), Sq=Sp, ap=alpha.data_ptr()):
        return f1(ctx.h, Pd.data_ptr(), rows_x, rows_x, n, kernel, ct(0.2), grid, 2, 0, Hp, n, s, C.byref(kk), b, Sq, ap, k, st, status, None, None, None,
                  None, None)

    def gv(kernel=0, grid=mg, Hp=Hd.data_ptr(), Sq=Sp, ap=alpha.data_ptr()):
        return f2(ctx.h, Pd.data_ptr(), rows_x, rows_x, n, kernel, ct(0.2), grid, 2, 1, Hp, n, s, k, Sq, ap, k, C.byref(info), None, None, None, None, None)

    for f in (rp, gv):
        assert f(kernel=-1) == -6 and f(kernel=3) == -6
        assert f(grid=None) == -100 and f(Hp=None) == -100 and f(Sq=None) == -100 and f(ap=None) == -100
    assert bool((alpha == 5.0).all()) and kk.value == k
    assert rp() == 0 and gv() == 0                                           # the path outputs may be NULL; the context is usable afterwards
    assert info.value == 0 and not bool((alpha == 5.0).any())
