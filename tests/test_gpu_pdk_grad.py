"""The gradient of a kernel expansion with respect to the evaluation point on the device: rlhip_pdk_cross_grad_* alone, in fp64
and fp32 for the three kernel kinds, on its fused route (opt-in), by default (the composed route) and with the cross apply behind the
composed route forced onto its own row-block route (rbf_fused = 0), against the float64 model by differences of tests/_pdk_grad_model.py.

Tolerance.  The project's rule of DESIGN 4.24, as tests/test_gpu_krr_var.py applies it: the device's error against the float64 gradient (a)
may be 8 times the error of the numpy emulation (b) of the same formula in the same dtype, with a floor of 64 eps_T; both errors are taken
entry by entry relative to the magnitude sum_j |w_ij| (|z_ic| + |x_jc|) |b_j| and the largest counts.  tests/test_pdk_grad_model.py bounds
(b)'s own error.  The largest ratios measured on an MI355X are in DESIGN 4.30."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import _pdk_grad_model as gm
import _pdk_model as pk

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
FUSED_MAX_COLS = 64                                                          # RLHIP_PDK_GRAD_FUSED_MAX_COLS
# (mz, nx, rows_x, n): the smallest case; nothing a multiple of anything; a second Z tile of one point and exactly one X tile; an X tile of
# one point; coordinates one past a multiple of four; n (rows_x + 1) = 64 exactly; 68 columns, past one cross apply's width; 65 columns,
# one past the fused kernel's limit; rows_x past the fused limit; 40 coordinates on the fused route (its instantiation for 33 .. 63)
SHAPES = [(1, 1, 1, 1), (63, 17, 2, 3), (65, 64, 5, 1), (130, 65, 3, 3), (200, 130, 17, 1), (66, 70, 15, 4), (70, 40, 16, 4), (66, 70, 12, 5),
          (40, 150, 130, 1), (65, 70, 40, 1)]
FUSED_SHAPES = [True, True, True, True, True, True, False, False, False, True]
ROUTES = ["fused", "default", "rbf_fused=0"]
ALPHA = 0.75


def _ids(shape):
    return "x".join(map(str, shape))


def _bandwidth(rows_x):
    return 0.4 * float(np.sqrt(rows_x))                                      # s / (2 l^2) about 1/2 at the mean distance of uniform points


@functools.lru_cache(maxsize=None)
def _case(shape, kind, prec, coincident=False):
    """inputs rounded to T, the model (a) with its magnitude and the emulation (b); computed once, never modified"""
    T = DT[prec]
    mz, nx, rows_x, n = shape
    rng = np.random.default_rng(1000 * mz + 10 * nx + n)
    Z = rng.random((rows_x, mz)).astype(T).astype(np.float64)
    X = rng.random((rows_x, nx)).astype(T).astype(np.float64)
    B = rng.standard_normal((nx, n)).astype(T).astype(np.float64)
    if coincident:                                                           # every fourth point of Z is a point of X
        Z[:, ::4] = X[:, :Z[:, ::4].shape[1]]
    l = _bandwidth(rows_x)
    truth, mag = gm.cross_grad(kind, Z, X, l, B, ALPHA)
    model = gm.emulate_grad(kind, Z, X, l, B, T, ALPHA).astype(np.float64)
    for a in (Z, X, B, truth, mag, model):
        a.setflags(write=False)
    return Z, X, B, l, truth, mag, model


def _pts(a, T, ld, fill=np.nan):
    """matrix (rows x cols, numpy) -> column-major device tensor (cols, ld); rows beyond `rows` hold `fill`"""
    import torch

    rows, cols = a.shape
    buf = np.full((cols, ld), fill, dtype=T)
    buf[:, :rows] = np.asarray(a, dtype=T).T
    return torch.from_numpy(buf).to("cuda:0")


def _run(ctx, kind, prec, Z, X, B, l, alpha=ALPHA, nx=None):
    """the device's G as [c, r, i] in float64; every leading dimension padded with NaN, two columns of NaN behind G, all asserted untouched.
    nx: the number of points of X the call is told of, where that is not all of them"""
    import torch
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, mz = Z.shape
    n = B.shape[1]
    nx = B.shape[0] if nx is None else nx
    Zd, Xd, Bd = _pts(Z, T, rows_x + 1), _pts(X, T, rows_x + 2), _pts(B, T, B.shape[0] + 3)
    G = torch.full((n * mz + 2, rows_x + 3), float("nan"), dtype=Zd.dtype, device="cuda:0")
    dev.pdk_cross_grad(ctx, Zd, Xd, rows_x, mz, nx, kind, l, Bd, n, alpha=alpha, G=G)
    raw = G.cpu().numpy()
    assert np.all(np.isnan(raw[:, rows_x:])) and np.all(np.isnan(raw[n * mz:, :]))
    return raw[:n * mz, :rows_x].astype(np.float64).reshape(n, mz, rows_x).transpose(2, 0, 1)


def _route(ctx, route):
    return ctx.grad_fused() if route == "fused" else (ctx.options(rbf_fused=0) if route == "rbf_fused=0" else contextlib.nullcontext())


def _expect_route(ctx, shape, route):
    _, _, rows_x, n = shape
    return 74 if route == "fused" and ctx.lib.rlhip_pdk_grad_fused(rows_x, n) else 75


def _within_model(what, dev, model, truth, mag, T):
    """device error <= max(8 x error of emulation (b), 64 eps_T), both relative to the magnitude"""
    eps = float(np.finfo(T).eps)
    e_dev, e_mod = float(np.max(np.abs(dev - truth) / mag)), float(np.max(np.abs(model - truth) / mag))
    allowed = max(8 * e_mod, 64 * eps)
    print(f"{what}: device error {e_dev / eps:.3g} eps, emulation (b) {e_mod / eps:.3g} eps, ratio {e_dev / max(e_mod, 1e-300):.3g}, "
          f"error / allowed {e_dev / allowed:.3g}")
    assert np.all(np.isfinite(dev))
    assert e_dev <= allowed, f"{what}: device error {e_dev:.3g} > allowed {allowed:.3g} (emulation (b): {e_mod:.3g})"


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradient_matches_model(ctx, shape, kind, route, prec):
    Z, X, B, l, truth, mag, model = _case(shape, kind, prec)
    before = [ctx.grad_path_count(w) for w in (74, 75)]
    with _route(ctx, route):
        got = _run(ctx, kind, prec, Z, X, B, l)
    took = _expect_route(ctx, shape, route)
    assert [ctx.grad_path_count(w) - c for w, c in zip((74, 75), before)] == [int(took == 74), int(took == 75)]
    _within_model(f"grad {shape} kind={kind} route {took} ({route}) {prec}", got, model, truth, mag, DT[prec])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", pk.KINDS)
def test_coincident_points(ctx, kind, route, prec):
    """every fourth point of Z is a point of X: s = 0 up to cancellation, the Matern clamp, and a finite weight w(0)"""
    shape = SHAPES[3]
    Z, X, B, l, truth, mag, model = _case(shape, kind, prec, True)
    assert np.array_equal(Z[:, 4], X[:, 1])
    with _route(ctx, route):
        got = _run(ctx, kind, prec, Z, X, B, l)
    _within_model(f"coincident {shape} kind={kind} ({route}) {prec}", got, model, truth, mag, DT[prec])


def test_the_shapes_cover_both_routes(ctx):
    assert [_expect_route(ctx, s, "fused") == 74 for s in SHAPES] == FUSED_SHAPES
    assert [_expect_route(ctx, s, "default") for s in SHAPES] == [75] * len(SHAPES)      # the fused kernel is opt-in
    assert ctx.lib.rlhip_pdk_grad_fused(15, 4) == 1 and ctx.lib.rlhip_pdk_grad_fused(12, 5) == 0 and ctx.lib.rlhip_pdk_grad_fused(63, 1) == 1
    assert ctx.lib.rlhip_pdk_grad_fused(64, 1) == 0 and ctx.lib.rlhip_pdk_grad_fused(0, 1) == 0 and ctx.lib.rlhip_pdk_grad_fused(3, 0) == 0
    assert SHAPES[7][3] * (SHAPES[7][2] + 1) == FUSED_MAX_COLS + 1 and SHAPES[5][3] * (SHAPES[5][2] + 1) == FUSED_MAX_COLS
    assert ctx.lib.rlhip_pdk_grad_set_fused(ctx.h, 1) == 0 and ctx.lib.rlhip_pdk_grad_set_fused(ctx.h, 0) == 1      # returns the value found
    assert ctx.lib.rlhip_pdk_grad_set_fused(None, 1) == -1
    assert [ctx.grad_path_count(w) for w in (59, 73, 76)] == [-1, -1, -1] and ctx.lib.rlhip_pdk_grad_path_count(None, 74) == -1


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4], SHAPES[5]], ids=_ids)
def test_points_alone_have_the_bits_of_their_columns_in_the_batch_fused(ctx, shape, kind, prec):
    """the fused kernel's contract: the gradient at the points z0 .. z0 + m computed alone is, bit for bit, that of the full call"""
    Z, X, B, l, *_ = _case(shape, kind, prec)
    mz, m = shape[0], 3
    with _route(ctx, "fused"):
        before = ctx.grad_path_count(74)
        batch = _run(ctx, kind, prec, Z, X, B, l)
        for z0 in (0, 62, 64, mz - m):
            alone = _run(ctx, kind, prec, Z[:, z0:z0 + m], X, B, l)
            assert np.array_equal(alone, batch[:, :, z0:z0 + m]), f"points {z0} .. {z0 + m}: {np.max(np.abs(alone - batch[:, :, z0:z0 + m])):.3g}"
        assert ctx.grad_path_count(74) - before == 5


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[6]], ids=_ids)
def test_two_calls_give_the_same_bits(ctx, shape, route, prec):
    Z, X, B, l, *_ = _case(shape, pk.MATERN52, prec)
    with _route(ctx, route):
        assert np.array_equal(_run(ctx, pk.MATERN52, prec, Z, X, B, l), _run(ctx, pk.MATERN52, prec, Z, X, B, l))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("route", ["fused", "default"])
def test_alpha_zero_and_no_points_give_exact_zeros(ctx, route, prec):
    """alpha == 0 and nx == 0: exact zeros in G, X and B (full of NaN) are not read, the padding of G stays"""
    Z, X, B, l, *_ = _case(SHAPES[1], pk.MATERN32, prec)
    nan = lambda a: np.full_like(a, np.nan)
    with _route(ctx, route):
        before = [ctx.grad_path_count(w) for w in (74, 75)]
        got = _run(ctx, pk.MATERN32, prec, Z, nan(X), nan(B), l, alpha=0.0)
        assert got.shape == (2, 3, 63) and np.all(got == 0) and not np.any(np.signbit(got))
        got = _run(ctx, pk.MATERN32, prec, Z, nan(X), nan(B), l, nx=0)
        assert got.shape == (2, 3, 63) and np.all(got == 0)
        assert [ctx.grad_path_count(w) for w in (74, 75)] == before          # no route is reached


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_empty_shapes_and_argument_codes(ctx, prec):
    import torch

    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    rows_x, mz, nx, n = 3, 5, 4, 2
    Z = torch.rand((mz, rows_x), dtype=dt, device="cuda:0")
    X = torch.rand((nx, rows_x), dtype=dt, device="cuda:0")
    B = torch.rand((n, nx), dtype=dt, device="cuda:0")
    G = torch.full((n * mz, rows_x), 7.0, dtype=dt, device="cuda:0")
    fn = getattr(ctx.lib, f"rlhip_pdk_cross_grad_{prec}")
    good = dict(rows_x=rows_x, mz=mz, Z=Z.data_ptr(), ldz=rows_x, nx=nx, X=X.data_ptr(), ldx=rows_x, kernel=1, h=0.5, n=n, alpha=1.0, B=B.data_ptr(),
                ldb=nx, G=G.data_ptr(), ldg=rows_x)

    def call(**kw):
        a = dict(good, **kw)
        return fn(ctx.h, a["rows_x"], a["mz"], a["Z"], a["ldz"], a["nx"], a["X"], a["ldx"], a["kernel"], ct(a["h"]), a["n"], ct(a["alpha"]), a["B"],
                  a["ldb"], a["G"], a["ldg"])

    bad = [(dict(rows_x=0), -2), (dict(mz=-1), -3), (dict(Z=None), -4), (dict(ldz=rows_x - 1), -5), (dict(nx=-1), -6), (dict(X=None), -7),
           (dict(ldx=rows_x - 1), -8), (dict(kernel=3), -9), (dict(kernel=-1), -9), (dict(h=0.0), -10), (dict(h=float("nan")), -10),
           (dict(n=-1), -11), (dict(B=None), -13), (dict(ldb=nx - 1), -14), (dict(G=None), -15), (dict(ldg=rows_x - 1), -16)]
    before = [ctx.grad_path_count(w) for w in (74, 75)]
    for kw, code in bad:
        assert call(**kw) == code, kw
    assert fn(None, rows_x, mz, Z.data_ptr(), rows_x, nx, X.data_ptr(), rows_x, 1, ct(0.5), n, ct(1.0), B.data_ptr(), nx, G.data_ptr(), rows_x) == -1
    # mz == 0 or n == 0: returns 0, launches nothing, NULL arrays are no error
    assert call(mz=0) == 0 and call(mz=0, Z=None, X=None, B=None, G=None) == 0
    assert call(n=0) == 0 and call(n=0, B=None, G=None) == 0
    torch.cuda.synchronize()
    assert bool((G == 7.0).all()) and [ctx.grad_path_count(w) for w in (74, 75)] == before
    # alpha == 0 and nx == 0 with NULL X and B: zeros
    assert call(alpha=0.0, X=None, B=None) == 0
    torch.cuda.synchronize()
    assert bool((G == 0.0).all())
    G.fill_(7.0)
    assert call(nx=0, ldb=1, X=None, B=None) == 0
    torch.cuda.synchronize()
    assert bool((G == 0.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(G).all()) and bool((G != 0.0).any())
