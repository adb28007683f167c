"""No GPU.  (1) The numpy model of the predictive variance of restricted kernel ridge regression (tests/_krr_var_model.py): the quadratic form
on the fit's basis (b) against the dense definition (a); at a training point var = d_i + mu s_i with d the residual diagonal of the
factorization and s the leverage of tests/_krr_loo_model.py; at k = n the variance of the full Gaussian process; a far point gives the prior
exactly; the variance does not decrease when mu grows.  (2) The C++ layer (KrillRestrictedBasis, the basis argument of the four fits,
krr_predict_restricted_var) instantiates in both precisions with the host compiler alone.  (3) The library exports the new entry points.
(2) and (3) fail before the feature.

Where the tolerance comes from.  (a) solves with K_SS and with the normal equations, (b) inverts M with cond(M) = sqrt(cond(K_SS)) and
squares: both carry cond(K_SS) eps of their dtype; the bound is the 8 cond eps of tests/test_krr_restricted_model.py, with cond the larger
of cond(K_SS) and, for the float64 comparison, cond(K_S^T K_S + mu K_SS).  The variance scale is 1, so the errors are absolute."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _krr_loo_model as lm
import _krr_restricted_model as rm
import _krr_var_model as vm
import _pdk_model as pk

ROOT = Path(__file__).resolve().parent.parent
DT = {"f64": np.float64, "f32": np.float32}
# (n, rows_x, k, b): the four fit shapes of tests/test_gpu_krr_restricted.py with their bandwidths, and three larger ones whose k is one
# past a panel of 64 columns, two panels and a bit, and a panel and a half with 17 coordinates; the bandwidths keep cond_2(K(S, S)) <= 1e3
SHAPES = [(130, 2, 16, 16), (300, 3, 24, 8), (515, 5, 40, 16), (48, 2, 48, 8), (400, 3, 65, 16), (640, 5, 130, 32), (520, 17, 96, 32)]
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5), 48: (0.08, 0.12, 0.1), 400: (0.12, 0.2, 0.15),
             640: (0.2, 0.35, 0.3), 520: (0.6, 1.0, 0.8)}
MUS = (1e-3, 1e-2, 1e-1)
KEY = (7, 0)


points, eval_points = vm.points, vm.eval_points


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quadratic_form_equals_the_dense_definition(shape, kind, prec):
    T = DT[prec]
    eps = float(np.finfo(T).eps)
    n, rows_x, k, b = shape
    X = points(n, rows_x, T)
    l = BANDWIDTH[n][kind]
    f = rm.factor(kind, X, l, k, b, T, key=KEY)
    assert f["k"] == k
    S = f["S"]
    Z, _ = eval_points(X, S, T)
    mus = np.asarray(MUS, dtype=T).astype(np.float64)
    want = vm.dense(kind, X, l, S, mus, Z)
    got = vm.algorithm(kind, X, l, f["F"], S, mus, Z, len(MUS), T)
    KS = pk.cross_kernel(kind, X, X[:, S], l)
    KSS = KS[S, :]
    cond = float(np.linalg.cond(KSS))
    cond_a = max(float(np.linalg.cond(KS.T @ KS + mu * KSS)) for mu in mus)
    err = float(np.max(np.abs(got - want)))
    print(f"kind={kind} {shape} {prec}: cond(K_SS)={cond:.3g} cond(normal eq)={cond_a:.3g} error={err:.3g}")
    assert cond <= 1e3
    assert err <= 8 * max(cond, cond_a * float(np.finfo(np.float64).eps) / eps) * eps
    assert np.all(got >= 0)
    assert np.all(got[-5:, :] == 1.0)                                        # 50 away from the unit cube: every kernel entry underflows
    assert np.all(np.diff(got, axis=1) >= -8 * cond * eps)                   # MUS ascends: the variance does not decrease with mu


@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES[:3] + SHAPES[4:5], ids=lambda s: "x".join(map(str, s)))
def test_training_point_variance_is_residual_diagonal_plus_mu_times_leverage(shape, kind):
    """k_S(x_i) = M F(i, :)^T, so t = W^T F(i, :)^T = diag(sigma) U(i, :)^T: sum_j t_j^2 = (F F^T)_ii = 1 - d_i and
    sum_j mu / (sigma_j^2 + mu) t_j^2 = mu sum_j U_ij^2 sigma_j^2 / (sigma_j^2 + mu) = mu s_i"""
    T = np.float64
    n, rows_x, k, b = shape
    X = points(n, rows_x, T)
    l = BANDWIDTH[n][kind]
    f = rm.factor(kind, X, l, k, b, T, key=KEY)
    S = f["S"]
    U, sg, _ = np.linalg.svd(f["F"], full_matrices=False)
    mus = np.asarray(MUS)
    lev = ((U * U) @ lm.d_factor(sg, mus)).astype(np.float64)                # n x s
    want = np.asarray(f["d"], dtype=np.float64)[:, None] + mus[None, :] * lev
    got = vm.algorithm(kind, X, l, f["F"], S, mus, X, len(MUS), T)
    cond = float(np.linalg.cond(pk.cross_kernel(kind, X[:, S], X[:, S], l)))
    err = float(np.max(np.abs(got - want)))
    # (b) takes its kernel entries from the norm expansion, whose error is eps times 1 + L (|z|^2 + |x|^2) (tests/_pdk_model.entry_scale);
    # the factor and d took theirs from differences
    scale = float(np.max(pk.entry_scale(kind, X, X[:, S], l)))
    print(f"kind={kind} {shape}: cond(K_SS)={cond:.3g} entry scale={scale:.3g} error={err:.3g}")
    assert err <= 8 * cond * scale * float(np.finfo(T).eps)
    assert np.all(np.abs(np.asarray(f["d"])[S]) <= 8 * cond * float(np.finfo(T).eps))      # a centre has no Nystrom residual


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind,l", [(pk.MATERN32, 0.2), (pk.SQEXP, 0.12)])
def test_k_equal_n_is_the_full_gaussian_process(kind, l, prec):
    """all points are centres: the variance at training point i is mu (K (K + mu I)^-1)_ii"""
    T = DT[prec]
    n, rows_x, k, b = SHAPES[3]
    X = points(n, rows_x, T)
    f = rm.factor(kind, X, l, k, b, T, key=(3, 0))
    assert f["k"] == n
    K = pk.cross_kernel(kind, X, X, l)
    mus = np.asarray([1e-2, 1e-1], dtype=T).astype(np.float64)
    want = np.stack([mu * np.diag(K @ np.linalg.inv(K + mu * np.eye(n))) for mu in mus], axis=1)
    got = vm.algorithm(kind, X, l, f["F"], f["S"], mus, X, 2, T)
    cond = float(np.linalg.cond(K))
    err = float(np.max(np.abs(got - want)))
    print(f"k = n kind={kind} {prec}: cond(K)={cond:.3g} error={err:.3g}")
    assert err <= 8 * cond * float(np.finfo(T).eps)
    assert np.allclose(want, vm.dense(kind, X, l, f["S"], mus, X), rtol=0, atol=8 * cond * float(np.finfo(np.float64).eps))


def test_weights_model_values():
    e = vm.weights(np.array([2.0, 0.5]), np.array([0.0, 1.0]), 2, 0.3).astype(np.float64)
    assert np.allclose(e, [[0.0, 1.0 / 5.0], [1.0, 1.0 / 1.25]], rtol=1e-15) and e[0, 0] == 0 and e[1, 0] == 1
    one = vm.weights(np.array([2.0, 0.5]), np.array([1.0]), 3, 0.9).astype(np.float64)      # mu > 0: nothing is cut, one mu serves 3 columns
    assert one.shape == (2, 3) and np.allclose(one[:, 0], [0.2, 0.8]) and np.array_equal(one[:, 0], one[:, 2])
    t = np.array([[1.0, 1.0], [0.5, 0.0]])
    assert np.allclose(vm.from_t(t, e), [[0.0 + 1.0, 0.0 + 1.0], [0.75, 0.75 + 0.05]])      # the first row: 1 - 2 is clamped at 0


def test_cxx_layer_instantiates_in_both_precisions():
    """KrillRestrictedBasis, the basis argument of the four fits and krr_predict_restricted_var, double and float, host compiler only"""
    src = """#include "RandLAPACK_amd.hh"
namespace RL = RandLAPACK;
using RNG = r123::Philox4x32;
template <typename T>
void use(blas::Queue& q, const T* X, const T* H, const T* Z, T* alpha, T* Gb, T* sg, T* V, int64_t* S) {
    std::vector<T> regs{(T)0.1, (T)0.2, (T)0.3};
    RL::linops::RBFKernelMatrix<T> G(100, X, 5, (T)1.5, regs, q, 8);
    G.set_kernel(RL::PDKernel::Matern52);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t k = 10;
    RL::KrillRestrictedInfo info;
    RL::KrillRestrictedBasis<T> basis{Gb, 12, sg};
    static_assert(std::is_same<decltype(basis.G), T*>::value && std::is_same<decltype(basis.ldg), int64_t>::value &&
                  std::is_same<decltype(basis.sigma), T*>::value, "the basis");
    state = RL::krill_restricted_rpchol(100, G, 3, H, 104, k, S, alpha, 12, state, 4, &info, &basis);
    int64_t rc = RL::krill_restricted(100, G, 3, H, 104, k, (const int64_t*)S, alpha, 12, &basis);
    T grid[2] = {(T)0.01, (T)0.1};
    RL::KrillRidgePath path;
    state = RL::krill_restricted_rpchol_cv(100, G, 3, H, 104, 2, grid, RL::KrillCriterion::LeaveOneOut, k, S, alpha, 12, path, state, 4, &info, &basis);
    rc += RL::krill_restricted_cv(100, G, 3, H, 104, 2, grid, RL::KrillCriterion::GCV, k, (const int64_t*)S, alpha, 12, path, &basis);
    (void)rc;
    std::vector<T> mus(path.best_mu.begin(), path.best_mu.end());
    RL::krr_predict_restricted_var(G, k, (const int64_t*)S, basis, 30, Z, 5, 3, mus.data(), 3, V, 30);
}
template void use<double>(blas::Queue&, const double*, const double*, const double*, double*, double*, double*, double*, int64_t*);
template void use<float>(blas::Queue&, const float*, const float*, const float*, float*, float*, float*, float*, int64_t*);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_library_exports_the_variance_entry_points():
    from randlapack_amd import _lib

    lib = _lib.load()
    for name in ("rlhip_pdk_cross_var", "rlhip_drv_krill_restricted_rpchol_gp_pdk", "rlhip_drv_krill_restricted_gp_pdk",
                 "rlhip_drv_krr_predict_restricted_var_pdk"):
        for suf in ("f64", "f32"):
            assert hasattr(lib, f"{name}_{suf}")
    assert lib.rlhip_pdk_cross_var_f64(None, 1, 1, None, 1, 1, None, 1, 0, ctypes.c_double(1.0), None, 1, None, 1, None, 1, ctypes.c_double(0.0), None,
                                       1) == -1
    assert lib.rlhip_pdk_cross_var_f32(None, 1, 1, None, 1, 1, None, 1, 0, ctypes.c_float(1.0), None, 1, None, 1, None, 1, ctypes.c_float(0.0), None,
                                       1) == -1
    # the shape rule needs no device: rows_x within the fused kernel's limit, 1 <= s <= 8, at least one centre
    assert [lib.rlhip_pdk_var_fused(*a) for a in ((5, 100, 1), (128, 1, 8), (129, 100, 1), (5, 100, 9), (5, 0, 1), (5, 100, 0))] == [1, 1, 0, 0, 0, 0]
    from randlapack_amd import device as dev

    for fn in ("pdk_cross_var", "krill_restricted_rpchol_gp_pdk", "krill_restricted_gp_pdk", "krr_predict_restricted_var_pdk"):
        assert callable(getattr(dev, fn))
    hdr = (ROOT / "include" / "RandLAPACK_amd" / "rl_krill.hh").read_text()
    for name in ("struct KrillRestrictedBasis", "krr_predict_restricted_var"):
        assert name in hdr
