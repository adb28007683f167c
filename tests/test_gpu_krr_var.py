"""The predictive variance of restricted kernel ridge regression on the device: rlhip_pdk_cross_var_* alone on a synthetic
basis, on its fused (opt-in) and composed (default) routes, and the fits that keep their basis followed by krr_predict_restricted_var through the C entries,
in fp64 and fp32 for the three kernel kinds, against the float64 models of tests/_krr_var_model.py.

Tolerances.  The project's rule of DESIGN 4.24: the device's error against the float64 value (a) may be 8 times the error of the numpy
model (b) of the same algorithm in the same dtype, with a floor of 64 eps_T.  For the kernel alone both errors are relative to
max_i sum_j a_ij^2 with a = |K| |G| (what an error of t moves the quadratic form by); for the fit they are absolute, the variance scale
being 1.  The factor 8 covers the device's other summation orders (MFMA products, the Jacobi SVD and the blocked triangular solve of the
fit).  The largest ratios measured on an MI355X are in DESIGN 4.27."""
import ctypes as C
import functools

import numpy as np
import pytest

import _krr_restricted_model as rm
import _krr_var_model as vm
import _pdk_model as pk

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
KEY = (7, 0)
FUSED_MAX_S = 8                                                              # RLHIP_PDK_VAR_FUSED_MAX_S
# the kernel alone, (mz, k, rows_x, s): one point and one centre; nothing a multiple of anything; exactly one panel of 64 columns; a second
# panel of one column; three panels, five coordinates past a multiple of four; rows_x beyond the fused limit (the composed route); s beyond
# the sums the fused kernel carries (the composed route, two passes over a row of t).  The fused kernel is opt-in (Context.var_fused); every
# shape also runs on the composed route, by default and with the cross apply behind it forced onto its own composed route (rbf_fused = 0).
# The last two: 40 and 100 coordinates on the fused route (its instantiations for 33 .. 64 and 65 .. 128 coordinates); with 100 the fp64
# kernel stages tiles of 16 centres: five tiles, the last of 6 centres, and two panels.
KERNEL_SHAPES = [(1, 1, 1, 1), (63, 17, 2, 3), (65, 64, 5, 1), (130, 65, 3, 3), (200, 130, 17, 4), (70, 40, 130, 2), (66, 70, 4, FUSED_MAX_S + 3),
                 (65, 70, 40, 2), (65, 70, 100, 2)]
# fit then variance, (n, rows_x, k, b, s) and per n the bandwidths of the three kinds: the four of tests/test_gpu_krr_restricted.py and
# three with k one past a panel, two panels and a bit, a panel and a half
FIT_SHAPES = [(130, 2, 16, 16, 1), (300, 3, 24, 8, 3), (515, 5, 40, 16, 4), (48, 2, 48, 8, 2), (400, 3, 65, 16, 3), (640, 5, 130, 32, 3),
              (520, 17, 96, 32, 3)]
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5), 48: (0.08, 0.12, 0.1), 400: (0.12, 0.2, 0.15),
             640: (0.2, 0.35, 0.3), 520: (0.6, 1.0, 0.8)}


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

    return torch.from_numpy(np.array(a, dtype=T)).to("cuda:0")              # a copy: the cached inputs are read-only


def _ids(shape):
    return "x".join(map(str, shape))


def _within_model(what, dev, model, truth, scale, T):
    """device error <= max(8 x error of model (b), 64 eps_T), both relative to scale; returns the ratio device error / allowed"""
    eps = float(np.finfo(T).eps)
    e_dev, e_mod = float(np.max(np.abs(dev - truth))) / scale, float(np.max(np.abs(model - truth))) / scale
    allowed = max(8 * e_mod, 64 * eps)
    print(f"{what}: device error {e_dev:.3g}, model (b) error {e_mod:.3g}, ratio {e_dev / max(e_mod, 1e-300):.3g}, error / allowed {e_dev / allowed:.3g}")
    assert e_dev <= allowed, f"{what}: device error {e_dev:.3g} > allowed {allowed:.3g} (model (b): {e_mod:.3g})"


# ---------------------------------------------------------------------------------------------------
# 1. the kernel alone, on a synthetic basis
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(shape, kind, per_column, prec):
    """inputs rounded to T and the two models; computed once, never modified.  G has entries N(0, 1) / sqrt(k): 1 - sum t^2 takes both signs"""
    T = DT[prec]
    mz, k, rows_x, s = shape
    rng = np.random.default_rng(1000 * mz + 10 * k + s)
    Z = rng.random((rows_x, mz)).astype(T).astype(np.float64)
    Xs = rng.random((rows_x, k)).astype(T).astype(np.float64)
    G = (rng.standard_normal((k, k)) / np.sqrt(k)).astype(T).astype(np.float64)
    sigma = np.sort(rng.random(k) * 3 + 1e-3)[::-1].astype(T).astype(np.float64)
    mus = (10.0 ** rng.uniform(-4, 0, s if per_column else 1)).astype(T).astype(np.float64)
    # the bandwidth at which the median over the points of sum_j t_j^2 is 1 (bisection on log l: the sum is 0 for l -> 0 and about k for
    # l -> infinity), so that about half of the points are clamped
    q = lambda l: float(np.median(((pk.cross_kernel(kind, Z, Xs, l) @ G) ** 2).sum(axis=1)))
    lo, hi = np.log(1e-3), np.log(1e2)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if q(np.exp(mid)) < 1.0 else (lo, mid)
    l = float(np.exp(hi))
    prior = 1 - ((pk.cross_kernel(kind, Z, Xs, l) @ G) ** 2).sum(axis=1)
    assert mz < 63 or (np.any(prior < 0) and np.any(prior > 0)), "the clamp must be exercised, and not on every point"
    truth, scale = vm.quad_form(kind, Z, Xs, l, G, sigma, mus, s)
    model = vm.quad_form_model(kind, Z, Xs, l, G, sigma, mus, s, T)
    for a in (Z, Xs, G, sigma, mus, truth, model):
        a.setflags(write=False)
    return Z, Xs, G, sigma, mus, l, truth, model, scale


def _run_kernel(ctx, shape, kind, prec, Z, Xs, G, sigma, mus, l, rcond=0.0, mz=None, z0=0):
    """the device's V (mz x s, float64) for the points z0 .. z0 + mz of Z, every leading dimension padded with NaN"""
    from randlapack_amd import device as dev

    T = DT[prec]
    _, k, rows_x, s = shape
    mz = Z.shape[1] if mz is None else mz
    Zd = _pts(Z[:, z0:z0 + mz], T, rows_x + 1, fill=np.nan)
    Xd = _pts(Xs, T, rows_x + 2, fill=np.nan)
    Gd = _pts(G, T, k + 3, fill=np.nan)
    V = dev.pdk_cross_var(ctx, Zd, mz, Xd, rows_x, k, kind, l, Gd, _vec(sigma, T), _vec(mus, T), s, rcond=rcond, ldv=mz + 2)
    raw = V.cpu().numpy()
    assert np.all(np.isnan(raw[:, mz:]))                                     # the rows of V past mz are not touched
    return raw[:, :mz].T.astype(np.float64)


ROUTES = ["fused", "default", "rbf_fused=0"]


def _route(ctx, route):
    """the context manager under which a call takes the route: the fused kernel on request; the defaults; the composed route over the
    composed cross apply"""
    import contextlib

    return ctx.var_fused() if route == "fused" else (ctx.options(rbf_fused=0) if route == "rbf_fused=0" else contextlib.nullcontext())


def _expect_route(ctx, shape, route):
    from randlapack_amd import _lib

    _, k, rows_x, s = shape
    return 58 if route == "fused" and _lib.load().rlhip_pdk_var_fused(rows_x, k, s) else 59


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("per_column", [True, False], ids=["s_mus", "one_mu"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids)
def test_kernel_matches_model(ctx, shape, kind, per_column, route, prec):
    T = DT[prec]
    Z, Xs, G, sigma, mus, l, truth, model, scale = _kernel_case(shape, kind, per_column, prec)
    before = [ctx.var_path_count(w) for w in (58, 59)]
    with _route(ctx, route):
        got = _run_kernel(ctx, shape, kind, prec, Z, Xs, G, sigma, mus, l)
    took = _expect_route(ctx, shape, route)
    assert [ctx.var_path_count(w) - c for w, c in zip((58, 59), before)] == [int(took == 58), int(took == 59)]
    assert np.all(got >= 0)
    _within_model(f"kernel {shape} kind={kind} {'s mus' if per_column else 'one mu'} route {took} ({route}) {prec}", got, model, truth, scale, T)


def test_the_shapes_cover_both_routes(ctx):
    assert [_expect_route(ctx, s, "fused") for s in KERNEL_SHAPES] == [58, 58, 58, 58, 58, 59, 59, 58, 58]
    assert [_expect_route(ctx, s, "default") for s in KERNEL_SHAPES] == [59] * len(KERNEL_SHAPES)      # the fused kernel is opt-in
    assert ctx.lib.rlhip_pdk_var_set_fused(ctx.h, 1) == 0 and ctx.lib.rlhip_pdk_var_set_fused(ctx.h, 0) == 1      # returns the value found
    assert ctx.lib.rlhip_pdk_var_set_fused(None, 1) == -1


# (mz, k, rows_x, s) of the bit tests: three panels; k a multiple of 256, where the GEMM of the composed route is the stream-K one
BIT_SHAPES = [KERNEL_SHAPES[4], (130, 256, 16, 2)]


def _rows_alone(ctx, shape, kind, prec, route):
    """(rows that differ in bits between a call with mz = 1 and the batch, the largest difference, whether two batched calls agree)"""
    Z, Xs, G, sigma, mus, l, *_ = _kernel_case(shape, kind, True, prec)
    with _route(ctx, route):
        batch = _run_kernel(ctx, shape, kind, prec, Z, Xs, G, sigma, mus, l)
        again = _run_kernel(ctx, shape, kind, prec, Z, Xs, G, sigma, mus, l)
        bad, worst = [], 0.0
        for i in (0, 63, 64, shape[0] - 1):
            alone = _run_kernel(ctx, shape, kind, prec, Z, Xs, G, sigma, mus, l, mz=1, z0=i)
            if not np.array_equal(alone[0], batch[i]):
                bad.append(i)
                worst = max(worst, float(np.max(np.abs(alone[0] - batch[i]))))
    return bad, worst, np.array_equal(batch, again)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", [pk.SQEXP, pk.MATERN52])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=_ids)
def test_a_row_alone_has_the_bits_of_its_row_in_the_batch_fused(ctx, shape, kind, prec):
    """rows 0, 63, 64 and the last, each as a call with mz = 1, and the whole call twice: the fused kernel's contract, for every k"""
    bad, worst, repeatable = _rows_alone(ctx, shape, kind, prec, "fused")
    assert repeatable and not bad, f"rows {bad} differ by up to {worst:.3g}"


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", [pk.SQEXP, pk.MATERN52])
@pytest.mark.parametrize("shape,route", [(KERNEL_SHAPES[4], "default"), (KERNEL_SHAPES[5], "fused")], ids=["composed_by_default", "composed_by_shape"])
def test_a_row_alone_has_the_bits_of_its_row_in_the_batch_composed(ctx, shape, route, kind, prec):
    """The same on the composed route, as the issue behind DESIGN 4.27 asks for it on both routes.  The composed route sizes its blocks as
    the cross apply does (capped by mz) and takes t from the GEMMs behind it, which choose their kernel by the shape: it has no per-row
    contract (include/rlhip.h), and this case records what it does.  On an MI355X the eight cases below agree bit for bit (for these shapes the
    products keep the order of a row's sums whatever the number of rows); the interface does not promise it."""
    bad, worst, repeatable = _rows_alone(ctx, shape, kind, prec, route)
    print(f"composed route {shape} kind={kind} {prec}: rows {bad} differ between mz = 1 and the batch by up to {worst:.3g}")
    assert repeatable
    assert not bad, f"rows {bad} differ by up to {worst:.3g}"


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES)
def test_mu_zero_cuts_small_singular_values(ctx, route, prec):
    """mu = 0 in columns 0 and 2: e = 1 where sigma_j <= rcond sigma_0 and 0 elsewhere; mu > 0 in column 1 cuts nothing whatever rcond says"""
    T = DT[prec]
    shape = (70, 40, 3, 3)
    Z, Xs, G, _, _, l, *_ = _kernel_case(shape, pk.MATERN32, True, prec)
    sigma = (10.0 ** -np.arange(40, dtype=np.float64) * 0.5).astype(T).astype(np.float64)
    sigma[0] = 1
    mus = np.array([0.0, 1e-3, 0.0], dtype=T).astype(np.float64)
    rcond = 1e-6
    below = sigma <= rcond * sigma[0]
    assert below.any() and not below.all()
    e = vm.weights(sigma, mus, 3, rcond).astype(np.float64)
    assert np.array_equal(e[:, 0], below.astype(np.float64)) and np.array_equal(e[:, 2], e[:, 0]) and np.all(e[:, 1] > 0)
    with _route(ctx, route):
        got = _run_kernel(ctx, shape, pk.MATERN32, prec, Z, Xs, G, sigma, mus, l, rcond=rcond)
    truth, scale = vm.quad_form(pk.MATERN32, Z, Xs, l, G, sigma, mus, 3, rcond)
    model = vm.quad_form_model(pk.MATERN32, Z, Xs, l, G, sigma, mus, 3, T, rcond)
    _within_model(f"mu = 0 {prec}", got, model, truth, scale, T)
    assert np.array_equal(got[:, 0], got[:, 2])
    # without the cut the two columns are the clamped Nystrom residual alone
    with _route(ctx, route):
        plain = _run_kernel(ctx, shape, pk.MATERN32, prec, Z, Xs, G, sigma, mus, l, rcond=0.0)
    assert np.all(plain[:, 0] <= got[:, 0]) and np.any(plain[:, 0] < got[:, 0])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_empty_shapes_and_argument_codes(ctx, prec):
    import torch

    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    rows_x, mz, k, s = 3, 5, 4, 2
    dev0 = "cuda:0"
    Z = torch.rand((mz, rows_x), dtype=dt, device=dev0)
    X = torch.rand((k, rows_x), dtype=dt, device=dev0)
    G = torch.rand((k, k), dtype=dt, device=dev0)
    sg = torch.ones(k, dtype=dt, device=dev0)
    mus = torch.ones(s, dtype=dt, device=dev0)
    V = torch.full((s, mz), 7.0, dtype=dt, device=dev0)
    fn = getattr(ctx.lib, f"rlhip_pdk_cross_var_{prec}")
    good = dict(rows_x=rows_x, mz=mz, Z=Z.data_ptr(), ldz=rows_x, k=k, Xs=X.data_ptr(), ldx=rows_x, kernel=0, h=0.5, G=G.data_ptr(), ldg=k,
                sigma=sg.data_ptr(), s=s, mus=mus.data_ptr(), num_mus=s, rcond=0.0, V=V.data_ptr(), ldv=mz)

    def call(**kw):
        a = dict(good, **kw)
        return fn(ctx.h, a["rows_x"], a["mz"], a["Z"], a["ldz"], a["k"], a["Xs"], a["ldx"], a["kernel"], ct(a["h"]), a["G"], a["ldg"], a["sigma"],
                  a["s"], a["mus"], a["num_mus"], ct(a["rcond"]), a["V"], a["ldv"])

    bad = [(dict(rows_x=0), -2), (dict(mz=-1), -3), (dict(Z=None), -4), (dict(ldz=rows_x - 1), -5), (dict(k=-1), -6), (dict(Xs=None), -7),
           (dict(ldx=rows_x - 1), -8), (dict(kernel=3), -9), (dict(kernel=-1), -9), (dict(h=0.0), -10), (dict(h=float("nan")), -10),
           (dict(G=None), -11), (dict(ldg=k - 1), -12), (dict(sigma=None), -13), (dict(s=-1), -14), (dict(mus=None), -15),
           (dict(rcond=-1.0), -17), (dict(rcond=float("nan")), -17), (dict(V=None), -18), (dict(ldv=mz - 1), -19),
           (dict(num_mus=3), -100), (dict(num_mus=0), -100), (dict(s=3, num_mus=2), -100)]
    before = [ctx.var_path_count(w) for w in (58, 59)]
    for kw, code in bad:
        assert call(**kw) == code, kw
    assert fn(None, rows_x, mz, Z.data_ptr(), rows_x, k, X.data_ptr(), rows_x, 0, ct(0.5), G.data_ptr(), k, sg.data_ptr(), s, mus.data_ptr(), s, ct(0.0),
              V.data_ptr(), mz) == -1
    # mz == 0 or s == 0: returns 0, launches nothing, NULL arrays are no error
    assert call(mz=0, ldv=1) == 0 and call(mz=0, ldv=1, Z=None, Xs=None, G=None, sigma=None, mus=None, V=None, num_mus=7) == 0
    assert call(s=0) == 0 and call(s=0, V=None, mus=None, num_mus=5) == 0
    torch.cuda.synchronize()
    assert bool((V == 7.0).all()) and [ctx.var_path_count(w) for w in (58, 59)] == before
    # k == 0: the prior variance 1 in every entry, nothing else is read
    Vp = torch.full((s, mz + 2), float("nan"), dtype=dt, device=dev0)
    assert call(k=0, ldg=1, Z=None, Xs=None, G=None, sigma=None, mus=None, V=Vp.data_ptr(), ldv=mz + 2) == 0
    torch.cuda.synchronize()
    out = Vp.cpu().numpy()
    assert np.all(out[:, :mz] == 1.0) and np.all(np.isnan(out[:, mz:]))
    assert call() == 0 and call(num_mus=1) == 0


# ---------------------------------------------------------------------------------------------------
# 2. fit, then variance, through the driver entries
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(n, rows_x, s, prec):
    T = DT[prec]
    X = vm.points(n, rows_x, T)
    H = np.random.default_rng(1000 * n + 1).standard_normal((n, s)).astype(T).astype(np.float64)
    H.setflags(write=False)
    return X, H


def _mus(s):
    return [10.0 ** (-3 + i) for i in range(s)]


@functools.lru_cache(maxsize=None)
def _fit_reference(shape, kind, prec, S):
    """the dense definition (a) and the model (b) in T on the centres S (a tuple: the device's), for the pivoted factor and for the factor
    of the given-centres fit; computed once, never modified"""
    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, _ = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    mus = np.asarray(_mus(s), dtype=T).astype(np.float64)
    Sa = np.array(S, dtype=np.int64)
    Z, _ = vm.eval_points(X, Sa, T)
    truth = vm.dense(kind, X, l, Sa, mus, Z)
    f = rm.factor(kind, X, l, Sa.size, b, T, forced_S=[Sa[p:p + b] for p in range(0, Sa.size, b)])
    assert f["k"] == Sa.size and np.array_equal(f["S"], Sa)
    model = vm.algorithm(kind, X, l, f["F"], Sa, mus, Z, s, T)
    f2, info = rm.given_centres_factor(kind, X, l, Sa, T)
    assert info == 0
    model2 = vm.algorithm(kind, X, l, f2, Sa, mus, Z, s, T)
    KSS = pk.cross_kernel(kind, X[:, Sa], X[:, Sa], l)
    cond = float(np.linalg.cond(KSS))
    Gm, sgm = vm.basis(f["F"], Sa, T)
    Gm = Gm.astype(np.float64)
    basis_res = float(np.max(np.abs(Gm.T @ KSS @ Gm - np.eye(Sa.size))))
    for a in (truth, model, model2, KSS):
        a.setflags(write=False)
    return Z, truth, model, model2, cond, KSS, sgm.astype(np.float64), basis_res


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=_ids)
def test_fit_then_variance(ctx, shape, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, H = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    mus = _mus(s)
    Pd, Hd = _pts(X, T, rows_x + 2, fill=1e30), _pts(H, T)
    plain = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY)
    r = dev.krill_restricted_rpchol_gp_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY, ldg=k + 3)
    assert r["k"] == k == plain["k"]
    # with a basis, S, alpha, the state and the codes are those of the fit without one, bit for bit
    assert np.array_equal(r["S"], plain["S"]) and np.array_equal(r["alpha"].cpu().numpy(), plain["alpha"].cpu().numpy())
    assert (r["next_ctr"], r["status"], r["c_status"]) == (plain["next_ctr"], plain["status"], plain["c_status"])
    Graw = r["G"].cpu().numpy()
    assert np.all(np.isnan(Graw[:, k:])) and np.all(np.isfinite(Graw[:, :k])) and np.all(np.isfinite(r["sigma"].cpu().numpy()))
    S = r["S"]
    Z, truth, model, model2, cond, KSS, sg_model, res_model = _fit_reference(shape, kind, prec, tuple(S.tolist()))
    print(f"cond(K_SS) = {cond:.3g}")
    assert cond <= 1e3
    # the basis itself, in quantities that do not depend on the signs of the singular vectors: G^T K_SS G = W^T M^-1 K_SS M^-T W = I, with
    # the rule above and a floor of 64 eps cond(K_SS) (M^-1 acts on either side: cond(M)^2 = cond(K_SS)); sigma within 64 eps cond
    # sigma_0 of LAPACK's (the factor's panel solves carry sqrt(cond) eps per column, and Weyl)
    eps = float(np.finfo(T).eps)
    Gh = Graw[:, :k].T.astype(np.float64)
    res_dev = float(np.max(np.abs(Gh.T @ KSS @ Gh - np.eye(k))))
    sg_dev = r["sigma"].cpu().numpy().astype(np.float64)
    sg_err = float(np.max(np.abs(sg_dev - sg_model)) / sg_model[0])
    print(f"basis: |G^T K_SS G - I| device {res_dev:.3g}, model (b) {res_model:.3g}; sigma error {sg_err:.3g} sigma_0")
    assert res_dev <= max(8 * res_model, 64 * eps * cond) and sg_err <= 64 * eps * cond
    mz = Z.shape[1]
    Zd = _pts(Z, T)
    Y0 = dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s).cpu().numpy()
    before = [ctx.var_path_count(w) for w in (58, 59)]
    V = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["G"], r["sigma"], mus, s), mz)
    Vf = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["G"], r["sigma"], mus, s, fused_kernel=True), mz)
    assert ctx.lib.rlhip_pdk_var_set_fused(ctx.h, 0) == 0                    # the request lasted for the call
    assert [ctx.var_path_count(w) - c for w, c in zip((58, 59), before)] == [1, 1]
    Y1 = dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s).cpu().numpy()
    assert np.array_equal(Y0, Y1)                                            # prediction on the same context keeps its bits
    what = f"fit {shape} kind={kind} {prec}"
    for name, v in (("composed", V), ("fused", Vf)):
        _within_model(f"{what} {name}", v, model, truth, 1.0, T)
        assert np.all(v >= 0)
        assert np.all(v[-5:, :] == 1.0)                                      # the points 50 away: the prior, exactly
    # the same centres given
    info0, a0 = dev.krill_restricted_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, S)
    info, a2, G2, sg2 = dev.krill_restricted_gp_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, S)
    assert info == 0 == info0 and np.array_equal(a0.cpu().numpy(), a2.cpu().numpy())
    V2 = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, G2, sg2, mus, s), mz)
    _within_model(what + " given centres", V2, model2, truth, 1.0, T)
    assert np.all(V2 >= 0) and np.all(V2[-5:, :] == 1.0)
    if s > 1:                                                                # one regularization for every column: column 1 of the above
        V1 = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["G"], r["sigma"], mus[1:2], s), mz)
        assert np.array_equal(V1, np.repeat(V[:, 1:2], s, axis=1))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_given_centres_with_a_repeated_centre_leave_the_basis_untouched(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = FIT_SHAPES[1]
    X, H = _problem(n, rows_x, s, prec)
    S = np.arange(5, 5 + k, dtype=np.int64)
    S[1] = S[0]
    info, alpha, G, sg = dev.krill_restricted_gp_pdk(ctx, _pts(X, T), rows_x, n, pk.MATERN32, 0.25, [1e-2], _pts(H, T), s, S)
    assert info == 2
    assert all(bool(np.all(np.isnan(t.cpu().numpy()))) for t in (alpha, G, sg))      # handed in full of NaN, untouched


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rank_deficient_fit(ctx, prec):
    """64 points of which 32 are exact duplicates, 48 centres asked for (the problem of tests/test_gpu_krr_restricted.py): the basis is zero
    behind the achieved rank, and the variance from the whole k_in x k_in basis is finite and is the model's on the achieved centres"""
    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    n, rows_x, k, b, s = 64, 2, 48, 8, 2
    rng = np.random.default_rng(64)
    base = rng.random((rows_x, 32)).astype(T).astype(np.float64)
    X = np.concatenate([base, base], axis=1)[:, rng.permutation(n)]
    H = rng.standard_normal((n, s)).astype(T).astype(np.float64)
    kind, l, mus = pk.MATERN52, 0.1, [1e-2, 1e-1]
    Pd, Hd = _pts(X, T), _pts(H, T)
    plain = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY)
    r = dev.krill_restricted_rpchol_gp_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY)
    ko = r["k"]
    assert 1 <= ko <= 32 and ko == plain["k"] and np.array_equal(r["alpha"].cpu().numpy(), plain["alpha"].cpu().numpy())
    Gh, sg = r["G"].cpu().numpy().T, r["sigma"].cpu().numpy()               # Gh: k_in x k_in
    assert np.all(Gh[ko:, :] == 0) and np.all(Gh[:, ko:] == 0) and np.all(sg[ko:] == 0)
    assert np.all(np.isfinite(Gh)) and np.all(sg[:ko] > 0)
    S = r["S"]
    # sigma_j^2 are the eigenvalues of F F^T, in exact arithmetic the Nystrom approximation K(:, S') K(S', S')^-1 K(S', :) on the distinct
    # points S' among the centres.  A duplicate that was kept has a pivot and a residual column of the order of eps, so its column of F is
    # of the order of sqrt(eps): by Weyl sigma moves by at most sqrt(k) times that; the bound is 64 sqrt(k eps) sigma_0.
    _, first = np.unique(X[:, S].T, axis=0, return_index=True)
    Sd = S[np.sort(first)]
    KSd = pk.cross_kernel(kind, X, X[:, Sd], l)
    want = np.sqrt(np.maximum(np.sort(np.linalg.eigvalsh(KSd @ np.linalg.solve(KSd[Sd, :], KSd.T)))[::-1][:ko], 0.0))
    sg_err = float(np.max(np.abs(np.sort(sg[:ko].astype(np.float64))[::-1] - want)) / want[0])
    print(f"achieved rank {ko}, {Sd.size} distinct centres: sigma error {sg_err:.3g} sigma_0 (bound {64 * np.sqrt(k * eps):.3g})")
    assert np.all(np.diff(sg[:ko].astype(np.float64)) <= 0) and sg_err <= 64 * np.sqrt(k * eps)
    Z, _ = vm.eval_points(X, S, T)
    mz = Z.shape[1]
    Zd = _pts(Z, T)
    # k = the achieved rank with the k_in-strided basis, and k = k_in with the centres behind the rank set to any point: the same values
    V = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["G"], r["sigma"], mus, s), mz)
    S_all = np.where(r["S_all"] < 0, 0, r["S_all"])
    V_all = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S_all, r["G"], r["sigma"], mus, s), mz)
    assert np.all(np.isfinite(V)) and np.all(V >= 0) and np.all(V[-5:, :] == 1.0)
    assert np.max(np.abs(V - V_all)) <= 64 * eps
    # the model on the device's own basis (the quadratic form alone: the duplicates make the fit's own conditioning the factorization's affair)
    truth, scale = vm.quad_form(kind, Z, X[:, S], l, Gh[:ko, :ko].astype(np.float64), sg[:ko].astype(np.float64),
                                np.asarray(mus, dtype=T).astype(np.float64), s)
    model = vm.quad_form_model(kind, Z, X[:, S], l, Gh[:ko, :ko], sg[:ko], mus, s, T)
    _within_model(f"rank-deficient fit {prec}", V, model, truth, scale, T)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_drivers_refuse_bad_arguments(ctx, prec):
    from randlapack_amd import device as dev
    from randlapack_amd._lib import RlhipError

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    n, rows_x, k, b, s = FIT_SHAPES[0]
    X, H = _problem(n, rows_x, s, prec)
    Pd, Hd = _pts(X, T), _pts(H, T)
    r = dev.krill_restricted_rpchol_gp_pdk(ctx, Pd, rows_x, n, 0, 0.12, [1e-2], Hd, s, k=k, b=b, key=KEY)
    S, Sp = r["S"], r["S"].ctypes.data_as(C.POINTER(C.c_int64))
    Zd = _pts(X[:, :7], T)
    mu1 = (ct * 1)(1e-2)
    for kernel in (-1, 3):
        assert getattr(ctx.lib, f"rlhip_drv_krr_predict_restricted_var_pdk_{prec}")(ctx.h, rows_x, 7, Zd.data_ptr(), rows_x, n, Pd.data_ptr(), rows_x, kernel,
                                                                                   ct(0.12), k, Sp, r["G"].data_ptr(), k, r["sigma"].data_ptr(), 1, mu1, 1,
                                                                                   Hd.data_ptr(), 7, 0) == -9
    with pytest.raises(RlhipError):                                          # a negative regularization
        dev.krr_predict_restricted_var_pdk(ctx, Zd, 7, Pd, rows_x, n, 0, 0.12, S, r["G"], r["sigma"], [-1e-2], 1)
    with pytest.raises(RlhipError):                                          # two regularizations for three columns
        dev.krr_predict_restricted_var_pdk(ctx, Zd, 7, Pd, rows_x, n, 0, 0.12, S, r["G"], r["sigma"], [1e-2, 1e-1], 3)
    with pytest.raises(RlhipError):                                          # a centre that is no point
        dev.krr_predict_restricted_var_pdk(ctx, Zd, 7, Pd, rows_x, n, 0, 0.12, np.array([0, n]), r["G"], r["sigma"], [1e-2], 1)
    with pytest.raises(RlhipError):                                          # ldg below the number of centres asked for
        dev.krill_restricted_rpchol_gp_pdk(ctx, Pd, rows_x, n, 0, 0.12, [1e-2], Hd, s, k=k, b=b, key=KEY, ldg=k - 1)
    # the context is usable afterwards
    V = _host(dev.krr_predict_restricted_var_pdk(ctx, Zd, 7, Pd, rows_x, n, 0, 0.12, S, r["G"], r["sigma"], [1e-2], 1), 7)
    assert np.all(np.isfinite(V)) and np.all(V >= 0)
