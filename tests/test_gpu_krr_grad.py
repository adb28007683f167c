"""Gradients of fitted kernel ridge regression predictors on the device: a fit, then krr_predict_restricted_grad or
krr_predict_grad through the driver entries, in fp64 and fp32 for the three kernel kinds.

The device gradient is compared with the float64 model by differences of tests/_pdk_grad_model.py applied to the device's OWN coefficients
read back, under the rule of tests/test_gpu_pdk_grad.py: at most 8 times the error of the emulation in the same dtype, floor 64 eps_T, both
relative to sum_j |w_ij| (|z_ic| + |x_jc|) |coef_j|.  For fp64 the gradient is also compared with central differences of krr_predict_pdk on
the device itself."""
import functools

import numpy as np
import pytest

import _krr_var_model as vm
import _pdk_grad_model as gm
import _pdk_model as pk
from test_gpu_krr_var import BANDWIDTH, FIT_SHAPES
from test_gpu_pdk_grad import _within_model

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
KEY = (7, 0)


def _pts(a, T, ld=None, fill=0.0):
    import torch

    rows, cols = a.shape
    ld = ld or rows
    buf = np.full((cols, ld), fill, dtype=T)
    buf[:, :rows] = np.asarray(a, dtype=T).T
    return torch.from_numpy(buf).to("cuda:0")


def _host(t, rows):
    return t.detach().cpu().numpy()[:, :rows].T.astype(np.float64)


def _grad_host(G, s, mz, rows_x):
    """the drivers' (s mz, rows_x) tensor as [c, r, i] in float64"""
    return G.cpu().numpy().astype(np.float64).reshape(s, mz, rows_x).transpose(2, 0, 1)


@functools.lru_cache(maxsize=None)
def _problem(n, rows_x, s, prec):
    T = DT[prec]
    X = vm.points(n, rows_x, T)
    H = np.random.default_rng(1000 * n + 1).standard_normal((n, s)).astype(T).astype(np.float64)
    H.setflags(write=False)
    return X, H


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", FIT_SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_restricted_fit_then_gradient(ctx, shape, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, H = _problem(n, rows_x, s, prec)
    l = BANDWIDTH[n][kind]
    mus = [10.0 ** (-3 + i) for i in range(s)]
    Pd, Hd = _pts(X, T, rows_x + 2, fill=1e30), _pts(H, T)
    r = dev.krill_restricted_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, mus, Hd, s, k=k, b=b, key=KEY, ldalpha=k + 3)
    assert r["k"] == k
    S = r["S"]
    coef = _host(r["alpha"], k)                                              # k x s, the device's own
    Z = vm.eval_points(X, S, T)[0][:, :-5]                                   # fresh points, centres and other training points; not the far ones
    mz = Z.shape[1]
    Zd = _pts(Z, T, rows_x + 1, fill=np.nan)
    Y0 = dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s).cpu().numpy()
    before = [ctx.grad_path_count(w) for w in (74, 75)]
    got = _grad_host(dev.krr_predict_restricted_grad_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s), s, mz, rows_x)
    with ctx.grad_fused():
        fused = _grad_host(dev.krr_predict_restricted_grad_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s), s, mz, rows_x)
    assert [ctx.grad_path_count(w) - c for w, c in zip((74, 75), before)] == [1, 1]
    Y1 = dev.krr_predict_restricted_pdk(ctx, Zd, mz, Pd, rows_x, n, kind, l, S, r["alpha"], s).cpu().numpy()
    assert np.array_equal(Y0, Y1)                                            # prediction on the same context keeps its bits
    truth, mag = gm.cross_grad(kind, Z, X[:, S], l, coef)
    model = gm.emulate_grad(kind, Z, X[:, S], l, coef, T).astype(np.float64)
    _within_model(f"restricted fit {shape} kind={kind} {prec} composed", got, model, truth, mag, T)
    _within_model(f"restricted fit {shape} kind={kind} {prec} fused", fused, model, truth, mag, T)


@functools.lru_cache(maxsize=None)
def _full_fit(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, s, k, b = 130, 3, 2, 32, 8
    l = (0.3, 0.5, 0.4)[kind]
    X, H = _problem(n, rows_x, s, prec)
    Pd = _pts(X, T)
    r = dev.krill_full_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, [1e-1], _pts(H, T), _pts(np.zeros_like(H), T), s, 100 * float(np.finfo(T).eps), 200,
                                  k=k, b=b, key=KEY)
    assert r["k"] == k and r["iters"] >= 1
    coef = _host(r["X"], n)
    coef.setflags(write=False)
    return X, l, Pd, r["X"], coef


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_full_fit_then_gradient(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, s = 130, 3, 2
    X, l, Pd, coef_dev, coef = _full_fit(ctx, kind, prec)
    Z = np.concatenate([np.random.default_rng(5).random((rows_x, 60)), X[:, :10]], axis=1).astype(T).astype(np.float64)
    mz = Z.shape[1]
    before = [ctx.grad_path_count(w) for w in (74, 75)]
    got = _grad_host(dev.krr_predict_grad_pdk(ctx, _pts(Z, T), mz, Pd, rows_x, n, kind, l, coef_dev, s), s, mz, rows_x)
    assert [ctx.grad_path_count(w) - c for w, c in zip((74, 75), before)] == [0, 1]
    truth, mag = gm.cross_grad(kind, Z, X, l, coef)
    model = gm.emulate_grad(kind, Z, X, l, coef, T).astype(np.float64)
    _within_model(f"full fit kind={kind} {prec}", got, model, truth, mag, T)


@pytest.mark.parametrize("kind", pk.KINDS)
def test_gradient_matches_central_differences_of_the_device_prediction(ctx, kind):
    """fp64: (f(z + h e_c) - f(z - h e_c)) / (2 h) by krr_predict_pdk on the device, h = 1e-4 l, at three points.  Tolerance: the truncation
    bound h^2 max |f'''|, estimated from the model (a) as the second difference |g(z + h e_c) - 2 g(z) + g(z - h e_c)| of the gradient's
    coordinate c (the largest over the three points and the coordinates), plus 64 eps |f| / h for the rounding of the two predictions.
    The three points are those of twelve candidates where |f| is largest relative to sum_j |k_j| |coef_j|: where f cancels, the
    prediction's rounding is not a multiple of |f|."""
    from randlapack_amd import device as dev

    T = np.float64
    eps = float(np.finfo(T).eps)
    n, rows_x, s = 130, 3, 2
    X, l, Pd, coef_dev, coef = _full_fit(ctx, kind, "f64")
    cand = np.random.default_rng(9).random((rows_x, 12))
    f, fmag = pk.cross_apply(kind, cand, X, l, coef)
    Z = cand[:, np.argsort(-np.min(np.abs(f) / fmag, axis=1))[:3]]
    h = 1e-4 * l
    E = h * np.eye(rows_x)
    Zp = np.concatenate([Z + E[:, c:c + 1] for c in range(rows_x)], axis=1)  # column 3 c + i: point i moved along coordinate c
    Zm = np.concatenate([Z - E[:, c:c + 1] for c in range(rows_x)], axis=1)
    h_eff = (Zp - Zm)[np.arange(rows_x).repeat(3), np.arange(3 * rows_x)] / 2  # the step as the rounded points have it
    fp = _host(dev.krr_predict_pdk(ctx, _pts(Zp, T), 3 * rows_x, Pd, rows_x, n, kind, l, coef_dev, s), 3 * rows_x)
    fm = _host(dev.krr_predict_pdk(ctx, _pts(Zm, T), 3 * rows_x, Pd, rows_x, n, kind, l, coef_dev, s), 3 * rows_x)
    fd = ((fp - fm) / (2 * h_eff[:, None])).T.reshape(s, rows_x, 3).transpose(1, 0, 2)      # [c, r, i]
    got = _grad_host(dev.krr_predict_grad_pdk(ctx, _pts(Z, T), 3, Pd, rows_x, n, kind, l, coef_dev, s), s, 3, rows_x)
    g0 = gm.cross_grad(kind, Z, X, l, coef)[0]
    gp, gmn = gm.cross_grad(kind, Zp, X, l, coef)[0], gm.cross_grad(kind, Zm, X, l, coef)[0]
    trunc = max(float(np.max(np.abs(gp[c, :, 3 * c:3 * c + 3] - 2 * g0[c] + gmn[c, :, 3 * c:3 * c + 3]))) for c in range(rows_x))
    f0 = pk.cross_apply(kind, Z, X, l, coef)[0].T                            # s x 3
    tol = trunc + 64 * eps * np.abs(f0)[None, :, :] / h
    err = np.abs(got - fd)
    print(f"kind {kind}: largest |gradient - difference quotient| {err.max():.3g}, truncation bound {trunc:.3g}, rounding bound "
          f"{float(np.max(tol)) - trunc:.3g}, largest error / tolerance {float(np.max(err / tol)):.3g}")
    assert np.all(err <= tol)
