"""The two numpy forms of the kernel gradient (tests/_pdk_grad_model.py) against each other and against central differences
of the kernels of tests/_pdk_model.py.  No GPU.  The device tests (tests/test_gpu_pdk_grad.py, tests/test_gpu_krr_grad.py) allow the device 8
times the error of the emulation (b) with a floor of 64 eps_T; this file shows that (b)'s own error is a small multiple of eps_T relative
to sum_j |w_ij| (|z_ic| + |x_jc|) |b_j|, so that bound is a statement about rounding, not about the device."""
import numpy as np
import pytest

import _pdk_grad_model as gm
import _pdk_model as pk


def _case(mz, nx, rows_x, n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((rows_x, mz)), rng.random((rows_x, nx)), rng.standard_normal((nx, n))


@pytest.mark.parametrize("kind", pk.KINDS)
def test_weights_are_twice_the_derivative_of_the_kernel_in_s(kind):
    l = 0.7
    s = np.linspace(0.05, 4.0, 60)
    h = 1e-6
    fd = (pk.kernel_of_s(kind, s + h, l) - pk.kernel_of_s(kind, s - h, l)) / (2 * h)
    assert np.max(np.abs(2 * fd - gm.weight_of_s(kind, s, l)) / np.abs(gm.weight_of_s(kind, s, l))) <= 1e-6
    # the value at s = 0 of the table in include/rlhip.h; finite, so the gradient at a coincident point is 0 from that point
    assert gm.weight_of_s(kind, 0.0, l) == gm.weight0(kind, l)
    assert gm.weight0(kind, l) == {pk.SQEXP: -1.0, pk.MATERN32: -3.0, pk.MATERN52: -5.0 / 3.0}[kind] / (l * l)


@pytest.mark.parametrize("l", [0.3, 1.5])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_model_matches_central_differences_of_the_cross_apply(kind, l):
    Z, X, B = _case(9, 40, 5, 2, 11)
    Z[:, 0] = X[:, 3]                                                        # a coincident point
    G, mag = gm.cross_grad(kind, Z, X, l, B, alpha=0.75)
    h = 1e-6
    for c in range(Z.shape[0]):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[c] += h
        Zm[c] -= h
        fp, _ = pk.cross_apply(kind, Zp, X, l, B, alpha=0.75)
        fm, _ = pk.cross_apply(kind, Zm, X, l, B, alpha=0.75)
        fd = ((fp - fm) / (2 * h)).T                                         # n x mz
        # Matern 3/2 is twice, not three times, differentiable at a coincident point: there the difference quotient is exact to h only
        tol = np.where(np.arange(Z.shape[1]) == 0, 4 * h / l ** 3, 1e-6)[None, :] if kind == pk.MATERN32 else 1e-6
        assert np.all(np.abs(fd - G[c]) <= tol * mag[c]), (kind, l, c, float(np.max(np.abs(fd - G[c]) / mag[c])))


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("l", [0.3, 1.5])
@pytest.mark.parametrize("rows_x", [5, 17, 33])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_error_constant_of_the_expanded_formula(kind, rows_x, l, T):
    """the emulation in T against the float64 gradient by differences, coincident points included.  Two sources: the cancellation in
    z_c T_0 - T_c, a few eps_T of the magnitude; and the error eps_T (|z|^2 + |x|^2) of the expanded s, which moves w by its derivative --
    relative to the magnitude that is L_kind (|z|^2 + |x|^2) eps_T, the entry scale of tests/_pdk_model.py.  At a coincident point w is not
    Lipschitz for Matern 3/2, but the error of u is multiplied by z_c - x_c there: c sqrt(ds) sqrt(ds), the same order.  The bound is 8
    eps_T times the largest entry scale; the error measured is 1 to 10 eps_T where that scale is near 1 and at most a fifth of the bound."""
    Z, X, B = _case(24, 70, rows_x, 2, 100 * rows_x + kind)
    Z, X, B = (a.astype(T).astype(np.float64) for a in (Z, X, B))
    Z[:, :4] = X[:, 10:14]
    G, mag = gm.cross_grad(kind, Z, X, l, B)
    E = gm.emulate_grad(kind, Z, X, l, B, T).astype(np.float64)
    ratio = float(np.max(np.abs(E - G) / mag)) / float(np.finfo(T).eps)
    scale = float(np.max(pk.entry_scale(kind, Z, X, l)))
    print(f"kind {kind} rows_x {rows_x} l {l} {np.dtype(T).name}: error {ratio:.3g} eps, entry scale {scale:.3g}, error / bound {ratio / (8 * scale):.3g}")
    assert np.all(np.isfinite(E)) and ratio <= 8.0 * scale


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_emulated_u_is_one_at_zero_and_clamped(kind, T):
    assert gm.emulate_u(kind, np.array([0.0]), 0.4, T)[0] == T(1)
    if kind != pk.SQEXP:
        assert gm.emulate_u(kind, np.array([-1e-7]), 0.4, T)[0] == T(1)      # a negative s from cancellation is a coincident point
    assert np.isnan(gm.emulate_u(kind, np.array([np.nan]), 0.4, T)[0])
