"""No GPU.  (1) The numpy model of the kernel family (tests/_pdk_model.py) against closed forms.  (2) The measurements that the tolerances of
tests/test_gpu_pdk.py rest on, made on the emulation in T of the norm-expansion route, so that nothing is tuned to the device:
  entry bound   |K_T - K_model| <= C_e eps_T (1 + L_kind (|z_i|^2 + |x_j|^2)), L = 1/(2 l^2), 3/(2 l^2), 5/(6 l^2): the emulation stays at or
                below 2.1 in these units (asserted: 4); the device tests use C_e = 16, a fourfold margin for the device's exp, sqrt and
                summation order;
  apply bound   |C_T - C_model| <= 64 eps_T (|alpha| |K| |B| + |beta| |C0|), the form and value of tests/test_gpu_krr.py: the emulation
                stays at or below 9.5 at the bandwidths of the device tests (asserted: 16);
  Matern 1/2    exp(-sqrt(s) / l) does NOT satisfy the entry bound on the norm-expansion route: its derivative in s is unbounded at s = 0.
(3) The C++ layer of the feature instantiates with the host compiler alone and the library exports the new entries: these fail before the
feature."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _krr_model as km
import _pdk_model as pk

ROOT = Path(__file__).resolve().parent.parent
DT = {"f64": np.float64, "f32": np.float32}
C_E = 16.0                # the entry constant of the device tests
FACTOR = 64.0             # the apply constant of the device tests


# ---- (1) closed forms
@pytest.mark.parametrize("kind", pk.KINDS)
def test_kernel_is_one_at_distance_zero(kind):
    X = np.random.default_rng(kind).standard_normal((4, 9))
    K = pk.cross_kernel(kind, X, X, 0.8)
    assert np.array_equal(np.diag(K), np.ones(9)) and np.array_equal(K, K.T)
    assert np.all(K > 0) and np.all(K[~np.eye(9, dtype=bool)] < 1)


def test_two_points_at_distance_l():
    l = 1.7
    Z, X = np.zeros((3, 1)), np.array([[l], [0.0], [0.0]])
    assert np.isclose(pk.cross_kernel(pk.SQEXP, Z, X, l)[0, 0], np.exp(-0.5), rtol=1e-15, atol=0)
    assert np.isclose(pk.cross_kernel(pk.MATERN32, Z, X, l)[0, 0], (1 + np.sqrt(3)) * np.exp(-np.sqrt(3)), rtol=1e-15, atol=0)
    assert np.isclose(pk.cross_kernel(pk.MATERN52, Z, X, l)[0, 0], (1 + np.sqrt(5) + 5.0 / 3.0) * np.exp(-np.sqrt(5)), rtol=1e-15, atol=0)


def test_kind_zero_is_the_existing_model():
    rng = np.random.default_rng(1)
    Z, X, B = rng.standard_normal((5, 17)), rng.standard_normal((5, 23)), rng.standard_normal((23, 3))
    assert np.array_equal(pk.cross_kernel(pk.SQEXP, Z, X, 1.3), km.cross_kernel(Z, X, 1.3))
    for a, b in zip(pk.cross_apply(pk.SQEXP, Z, X, 1.3, B, -0.5), km.cross_apply(Z, X, 1.3, B, -0.5)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", pk.KINDS)
def test_lipschitz_constant_bounds_the_derivative_in_s(kind):
    l = 0.9
    s = np.concatenate([np.linspace(0.0, 1e-6, 11)[:-1], np.linspace(1e-6, 40.0, 400001)])
    slope = np.abs(np.diff(pk.kernel_of_s(kind, s, l)) / np.diff(s))
    L = pk.lipschitz(kind, l)
    assert np.max(slope) <= L and np.max(slope) >= 0.99 * L          # attained at s -> 0


def test_constants_are_rounded_once_from_double():
    f = np.float32
    c, third = pk.constants(pk.MATERN52, 0.3, f)
    assert c == f(np.sqrt(5.0) / 0.3) and third == f(1.0 / 3.0)
    assert pk.constants(pk.MATERN32, 0.3, f) == (f(np.sqrt(3.0) / 0.3), f(0))
    assert pk.constants(pk.SQEXP, 0.3, f)[0] == f(-1.0 / (2.0 * 0.3 * 0.3))


# ---- (2) the measurements
@functools.lru_cache(maxsize=None)
def _points(prec, rows_x, same):
    T = DT[prec]
    rng = np.random.default_rng(100 * rows_x + same)
    X = rng.standard_normal((rows_x, 67)).astype(T).astype(np.float64)
    Z = X if same else rng.standard_normal((rows_x, 65)).astype(T).astype(np.float64)
    B = rng.standard_normal((67, 5)).astype(T).astype(np.float64)
    for a in (Z, X, B):
        a.setflags(write=False)
    return Z, X, B


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("same", [0, 1], ids=["ZneX", "ZeqX"])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_entry_bound_of_the_emulation(kind, same, prec):
    T = DT[prec]
    eps = float(np.finfo(T).eps)
    worst = 0.0
    for rows_x in (1, 3, 5, 33, 128, 300):
        Z, X, _ = _points(prec, rows_x, same)
        for f in (0.2, 0.7, 3.0):
            l = f * float(np.sqrt(rows_x))
            err = np.abs(pk.emulate_kernel(kind, Z, X, l, T).astype(np.float64) - pk.cross_kernel(kind, Z, X, l))
            worst = max(worst, float(np.max(err / (eps * pk.entry_scale(kind, Z, X, l)))))
    print(f"kind {kind} {prec} same={same}: worst entry error = {worst:.3g} eps (1 + L (|z|^2 + |x|^2))")
    assert worst <= 4.0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("same", [0, 1], ids=["ZneX", "ZeqX"])
@pytest.mark.parametrize("kind", [pk.MATERN32, pk.MATERN52])
def test_apply_bound_of_the_emulation(kind, same, prec):
    """at the (rows_x, l) of the device tests that use this bound: l = 0.7 sqrt(rows_x), l = 1 on 3 and 4 coordinates, l = 3 on 5.  The bound
    is relative to |K|, and the RELATIVE error of an entry grows like L (|z|^2 + |x|^2) / (1 + a): it is a bound for bandwidths of the order
    of the points' norms, which is what a kernel method uses, not for l -> 0 (the emulation reaches 20 at l = 1 on 7 coordinates with
    Z = X, where L (|z|^2 + |x|^2) is about 21 and the diagonal carries the sums, and 33 at l = 0.2 sqrt(rows_x))."""
    T = DT[prec]
    eps = float(np.finfo(T).eps)
    worst = 0.0
    for rows_x, l in [(r, 0.7 * float(np.sqrt(r))) for r in (1, 4, 5, 7, 33, 128)] + [(3, 1.0), (4, 1.0), (5, 3.0)]:
        Z, X, B = _points(prec, rows_x, same)
        C0 = np.random.default_rng(rows_x).standard_normal((Z.shape[1], B.shape[1])).astype(T).astype(np.float64)
        for alpha, beta in ((1.0, 0.0), (-0.5, 2.0)):
            want, mag = pk.cross_apply(kind, Z, X, l, B, alpha, beta, C0)
            got = pk.emulate_apply(kind, Z, X, l, B, T, alpha, beta, C0).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got - want) / (eps * mag))))
    print(f"kind {kind} {prec} same={same}: worst apply error = {worst:.3g} eps (|alpha| |K| |B| + |beta| |C0|)")
    assert worst <= FACTOR / 4


def test_matern_one_half_would_break_the_entry_bound():
    """Why exp(-sqrt(s) / l) is not a kind of the library: near coincident points (the diagonal of K(X, X) included) the expanded s is off by
    about eps (|z|^2 + |x|^2), and sqrt turns that into sqrt(eps): the entry error is far outside the bound that kinds 0-2 satisfy, whichever
    of their constants L scales it."""
    T = np.float64
    Z, X, _ = _points("f64", 5, 1)
    l = 0.7 * float(np.sqrt(5))
    err = np.abs(pk.emulate_kernel(pk.MATERN12, Z, X, l, T) - pk.cross_kernel(pk.MATERN12, Z, X, l))
    units = err / (float(np.finfo(T).eps) * pk.entry_scale(pk.MATERN32, Z, X, l))      # the largest L: the most generous scale
    print(f"Matern 1/2, fp64, Z = X: worst entry error = {float(np.max(units)):.3g} of the entry bound's unit")
    assert float(np.max(units)) > 100 * C_E


def test_the_clamp_is_exercised_at_five_rows_and_not_at_one():
    """what tests/test_gpu_pdk.py::test_clamp relies on: coincident points give negative expanded s with rows_x = 5, never with rows_x = 1
    (one product, one sum: (x^2 + x^2) - 2 x x is exactly 0)"""
    for T in (np.float64, np.float32):
        X5 = (8.0 * np.random.default_rng(5).standard_normal((5, 100))).astype(T).astype(np.float64)
        assert np.any(np.diag(pk.expanded_s(X5, X5, T)) < 0)
        X1 = (8.0 * np.random.default_rng(1).standard_normal((1, 100))).astype(T).astype(np.float64)
        assert np.all(np.diag(pk.expanded_s(X1, X1, T)) == 0)


def test_nan_coordinate_stays_nan_through_the_clamp():
    s = np.array([np.nan, -1e-9, 0.0, 2.0])
    for kind in (pk.MATERN32, pk.MATERN52):
        k = pk.emulate_of_s(kind, s, 1.0, np.float64)
        assert np.isnan(k[0]) and k[1] == 1.0 and k[2] == 1.0 and 0 < k[3] < 1


# ---- (3) the feature's C++ layer and exports
def test_cxx_layer_takes_a_kernel_kind_with_the_host_compiler_alone():
    src = """#include "RandLAPACK_amd.hh"
template <typename T> void use(RandLAPACK::linops::RBFKernelMatrix<T>& G, RandLAPACK::linops::RBFCrossKernel<T>& Kzx, T* p) {
    G.set_kernel(RandLAPACK::PDKernel::Matern32);
    Kzx.set_kernel(RandLAPACK::PDKernel::Matern52);
    static_assert((int)RandLAPACK::PDKernel::SquaredExp == RLHIP_PDK_SQEXP && (int)RandLAPACK::PDKernel::Matern32 == RLHIP_PDK_MATERN32 &&
                  (int)RandLAPACK::PDKernel::Matern52 == RLHIP_PDK_MATERN52, "the enum follows the C constants");
    RandLAPACK::PDKernel k = G.kernel; (void)k;
    RandLAPACK::pd_kernel_submatrix<T>(RandLAPACK::PDKernel::Matern52, 1, 1, p, p, 1, 1, p, 0, 0, T(1));
}
template void use<double>(RandLAPACK::linops::RBFKernelMatrix<double>&, RandLAPACK::linops::RBFCrossKernel<double>&, double*);
template void use<float>(RandLAPACK::linops::RBFKernelMatrix<float>&, RandLAPACK::linops::RBFCrossKernel<float>&, float*);
template struct RandLAPACK::linops::RBFKernelMatrix<double>; template struct RandLAPACK::linops::RBFKernelMatrix<float>;
template struct RandLAPACK::linops::RBFCrossKernel<double>; template struct RandLAPACK::linops::RBFCrossKernel<float>;
int main() { return 0; }
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_library_exports_the_kernel_family_and_refuses_without_a_context():
    from randlapack_amd import _lib

    lib = _lib.load()
    names = ["pdk_columns", "pdk_submatrix", "pdk_apply", "pdk_cross_submatrix", "pdk_cross_apply", "drv_rpchol_pdk", "drv_krill_full_rpchol_pdk",
             "drv_krr_predict_pdk", "drv_pdk_kernel_apply"]
    for name in names:
        for suf in ("f64", "f32"):
            assert f"rlhip_{name}_{suf}" in _lib.SIGNATURES and hasattr(lib, f"rlhip_{name}_{suf}")
    # no context: -1 before anything else is looked at, so this needs no device
    z = ctypes.c_double(1.0)
    assert lib.rlhip_pdk_cross_apply_f64(None, 1, 1, None, 1, 1, None, 1, 7, z, 1, z, None, 1, z, None, 1) == -1
    assert lib.rlhip_pdk_cross_submatrix_f64(None, 1, 1, None, 1, None, 1, None, 1, None, 1, 1, None, 1, 0, 0, 7, z) == -1
