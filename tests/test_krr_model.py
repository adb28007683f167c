"""No GPU.  (1) The numpy model of the cross kernel and of fit-then-predict (tests/_krr_model.py) against closed forms; (2) the C++ layer of
the feature (linops::RBFCrossKernel, krr_predict, RBFKernelMatrix::set_matrix_free) instantiates in both precisions with the host compiler
alone; (3) the library exports the new entry points.  (2) and (3) fail before the feature."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _krr_model as km
import _rpchol_model as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("rows_x", [1, 3, 16])
def test_same_point_set_reproduces_the_square_kernel(rows_x):
    rng = np.random.default_rng(rows_x)
    X = rng.standard_normal((rows_x, 57))
    for h in (0.5, 2.0):
        assert np.allclose(km.cross_kernel(X, X, h), M.sqexp_matrix(X, h), rtol=1e-14, atol=0)
        assert np.allclose(km.cross_kernel(X[:, 5:20], X, h), M.sqexp_matrix(X, h)[5:20], rtol=1e-14, atol=0)


def test_cross_kernel_is_rectangular_and_its_transpose_swaps_the_sets():
    rng = np.random.default_rng(1)
    Z, X = rng.standard_normal((4, 9)), rng.standard_normal((4, 23))
    K = km.cross_kernel(Z, X, 1.3)
    assert K.shape == (9, 23)
    assert np.array_equal(K.T, km.cross_kernel(X, Z, 1.3))
    assert K[2, 5] == np.exp(-np.sum((Z[:, 2] - X[:, 5]) ** 2) / (2 * 1.3 ** 2))


def test_far_point_predicts_zero():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((3, 40))
    a = km.fit(X, 1.0, [1e-2], rng.standard_normal((40, 2)))
    Z = np.full((3, 1), 1e3)
    assert np.array_equal(km.predict(Z, X, 1.0, a), np.zeros((1, 2)))     # exp(-~1.5e6) underflows to 0


def test_one_training_point_closed_form():
    x = np.array([[0.3], [-1.2]])
    Z = np.array([[0.0, 1.0, 0.3], [0.0, 2.0, -1.2]])
    h, mu, y = 0.8, 0.25, 1.7
    a = km.fit(x, h, [mu], np.array([[y]]))
    assert np.allclose(a, y / (1 + mu), rtol=1e-15)
    k = np.exp(-np.sum((Z - x) ** 2, axis=0) / (2 * h * h))
    got = km.predict(Z, x, h, a)[:, 0]
    assert np.allclose(got, y * k / (1 + mu), rtol=1e-15, atol=0)
    assert got[2] == a[0, 0]                                                 # at the training point itself k = 1


def test_fit_then_predict_interpolates_as_mu_vanishes():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((2, 12))
    H = rng.standard_normal((12, 3))
    a = km.fit(X, 0.7, [1e-10, 1e-10, 1e-10], H)
    assert np.allclose(km.predict(X, X, 0.7, a), H, atol=1e-6)
    out, mag = km.cross_apply(X[:, :5], X, 0.7, a, alpha=-0.5, beta=2.0, C0=H[:5])
    assert np.allclose(out, -0.5 * km.predict(X[:, :5], X, 0.7, a) + 2.0 * H[:5]) and np.all(mag >= np.abs(out) * (1 - 1e-14))


def test_cxx_layer_instantiates_in_both_precisions():
    """RBFCrossKernel (operator(), matvec, submatrix), krr_predict and set_matrix_free, double and float, host compiler only"""
    src = """#include "RandLAPACK_amd.hh"
namespace RL = RandLAPACK;
template <typename T>
void use(blas::Queue& q, const T* Z, const T* X, const T* B, T* C, T* K) {
    RL::linops::RBFCrossKernel<T> Kzx(5, 30, Z, 100, X, (T)1.5, q, 8, 5);
    static_assert(std::is_same<typename RL::linops::RBFCrossKernel<T>::scalar_t, T>::value, "scalar_t");
    int64_t m = Kzx.n_rows, n = Kzx.n_cols;
    Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, 3, (T)1, B, n, (T)0, C, m);
    Kzx(blas::Layout::ColMajor, blas::Op::Trans, 3, (T)1, C, m, (T)0, K, n);
    Kzx.matvec(blas::Op::NoTrans, (T)1, B, (T)0, C);
    Kzx.submatrix(10, 20, K, 1, 2);
    RL::krr_predict(Kzx, 3, B, n, C, m);
    std::vector<T> regs{(T)0.1};
    RL::linops::RBFKernelMatrix<T> G(100, X, 5, (T)1.5, regs, q);
    G.set_matrix_free(true);
    G(blas::Layout::ColMajor, 3, (T)1, const_cast<T*>(B), 100, (T)0, K, 100);
}
template void use<double>(blas::Queue&, const double*, const double*, const double*, double*, double*);
template void use<float>(blas::Queue&, const float*, const float*, const float*, float*, float*);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_library_exports_the_cross_kernel_entry_points():
    from randlapack_amd import _lib

    lib = _lib.load()
    for name in ("rlhip_rbf_cross_apply", "rlhip_sqexp_cross_submatrix", "rlhip_drv_krr_predict", "rlhip_drv_rbf_kernel_apply"):
        for suf in ("f64", "f32"):
            assert hasattr(lib, f"{name}_{suf}")
    assert lib.rlhip_rbf_path_count(None, 55) == -1
    assert lib.rlhip_rbf_cross_apply_f64(None, 1, 0, None, 1, 0, None, 1, ctypes.c_double(1.0), 0, ctypes.c_double(1.0), None, 1,
                                         ctypes.c_double(0.0), None, 1) == -1
    from randlapack_amd import device as dev

    assert dev.Context.OPT["rbf_fused"] == 14
    for fn in ("rbf_cross_apply", "sqexp_cross_submatrix", "krr_predict"):
        assert callable(getattr(dev, fn))
    hdr = (ROOT / "include" / "rlhip.h").read_text()
    assert "RLHIP_OPT_RBF_FUSED = 14" in hdr and "RLHIP_OPT_COUNT = 15" in hdr
    assert "#define RLHIP_RBF_FUSED_MAX_N 64" in hdr and "#define RLHIP_RBF_FUSED_MAX_ROWS_X 128" in hdr
