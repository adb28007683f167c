"""No GPU.  (1) The numpy model of restricted kernel ridge regression (tests/_krr_restricted_model.py): the SVD-filter-trsm tail (b) against
the dense solve (a), the k = n identity with the full fit, the properties of M = F(S, :) the tail relies on, the pseudo-inverse cut-off;
(2) the C++ layer (krill_restricted_rpchol, krill_restricted, krr_predict_restricted) instantiates in both precisions with the host compiler
alone; (3) the library exports the new entry points.  (2) and (3) fail before the feature.

Where the tolerances come from.  (a) solves normal equations, so it carries a relative error of about cond(K_S^T K_S + mu K_SS) eps_64; (b)
works on F and carries cond(F) eps_T = sqrt(cond(K_SS)) eps_T times the triangular solve's cond(M) = sqrt(cond(K_SS)).  The tests compute
these condition numbers and allow 8 times the larger estimate."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _krr_model as km
import _krr_restricted_model as rm
import _pdk_model as pk

ROOT = Path(__file__).resolve().parent.parent
DT = {"f64": np.float64, "f32": np.float32}
# (n, rows_x, k, b, s): the shapes of tests/test_gpu_krr_restricted.py, and per n the bandwidth of each kernel kind (squared exponential,
# Matern 3/2, Matern 5/2).  On these points cond_2(K(S, S)) is 40 to 500 for three sampling keys, in both precisions: the squared exponential
# needs the shortest bandwidth for that, and the small sets (130 points in the plane, all 48 points as centres) shorter ones than the large.
SHAPES = [(130, 2, 16, 16, 1), (300, 3, 24, 8, 3), (515, 5, 40, 16, 4), (48, 2, 48, 8, 2)]
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5), 48: (0.08, 0.12, 0.1)}


def _problem(n, rows_x, s, T, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    X = rng.random((rows_x, n)).astype(T).astype(np.float64)              # uniform in the unit cube
    H = rng.standard_normal((n, s)).astype(T).astype(np.float64)
    return X, H


def _relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("lockstep", [True, False])
def test_tail_in_float64_equals_the_dense_solve(shape, kind, lockstep):
    n, rows_x, k, b, s = shape
    X, H = _problem(n, rows_x, s, np.float64)
    l = BANDWIDTH[n][kind]
    mus = [10.0 ** (-3 + i) for i in range(s)] if lockstep else [1e-2]
    f = rm.factor(kind, X, l, k, b, np.float64, key=(7, 0))
    assert f["k"] == k
    want, KS = rm.truth(kind, X, l, f["S"], mus, H)
    got = rm.algorithm(f["F"], f["S"], mus, H, np.float64)["alpha"]
    KSS = KS[f["S"], :]
    cond_a = max(np.linalg.cond(KS.T @ KS + mu * KSS) for mu in mus)
    err = _relmax(got, want)
    eps = float(np.finfo(np.float64).eps)
    print(f"kind={kind} {shape} lockstep={lockstep}: cond(K_SS)={np.linalg.cond(KSS):.3g} cond(normal eq)={cond_a:.3g} error={err:.3g}")
    assert np.linalg.cond(KSS) <= 1e3
    assert err <= 8 * max(cond_a, np.linalg.cond(KSS)) * eps


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind,l", [(pk.MATERN32, 0.2), (pk.SQEXP, 0.12)])
def test_k_equal_n_is_the_full_fit_in_pivot_order(kind, l, prec):
    """min_x |K x - h|^2 + mu x^T K x has the normal equations K (K + mu I) x = K h: x = (K + mu I)^-1 h, the full fit, in the order of S"""
    T = DT[prec]
    n, rows_x, k, b, s = SHAPES[3]
    X, H = _problem(n, rows_x, s, T)
    mus = [1e-2, 1e-1]
    f = rm.factor(kind, X, l, k, b, T, key=(3, 0))
    assert f["k"] == n and sorted(f["S"].tolist()) == list(range(n))
    K = pk.cross_kernel(kind, X, X, l)
    full = np.stack([np.linalg.solve(K + mu * np.eye(n), H[:, i]) for i, mu in enumerate(mus)], axis=1)
    if kind == pk.SQEXP:
        assert np.allclose(full, km.fit(X, l, mus, H), rtol=1e-12, atol=0)      # the full fit's own model
    got = rm.algorithm(f["F"], f["S"], mus, H, T)["alpha"].astype(np.float64)
    err = _relmax(got, full[f["S"], :])
    cond = float(np.linalg.cond(K))
    print(f"k = n kind={kind} {prec}: cond(K)={cond:.3g} error={err:.3g}")
    assert err <= 8 * cond * float(np.finfo(T).eps)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", pk.KINDS)
def test_pivot_rows_of_the_factor_are_a_lower_triangular_root(kind, prec):
    """M = F(S, :): F M^T = K(:, S) (so M M^T = K(S, S)) and the part of M above the diagonal is rounding"""
    T = DT[prec]
    n, rows_x, k, b, s = SHAPES[1]
    X, _ = _problem(n, rows_x, s, T)
    l = BANDWIDTH[n][kind]
    f = rm.factor(kind, X, l, k, b, T, key=(7, 0))
    F, S = f["F"].astype(np.float64), f["S"]
    Mt = F[S, :]
    KS = pk.cross_kernel(kind, X, X[:, S], l)
    eps = float(np.finfo(T).eps)
    cond = float(np.linalg.cond(KS[S, :]))
    e1, e2 = float(np.max(np.abs(F @ Mt.T - KS))), float(np.max(np.abs(np.triu(Mt, 1))))
    print(f"kind={kind} {prec}: |F M^T - K_S| = {e1:.3g}, |triu(M, 1)| = {e2:.3g}, cond(K_SS) = {cond:.3g}")
    # a Cholesky factor's residual is k eps |K|; the panel solves F = A U^-1 add cond(U) eps = sqrt(cond) eps per entry of F
    assert e1 <= 8 * k * eps * np.sqrt(cond) and e2 <= 8 * k * eps * np.sqrt(cond)
    assert np.all(np.diag(Mt) > 0)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_mu_zero_with_a_rank_deficient_factor_hits_the_cut_off(prec):
    """A factor with M = F(S, :) regular has full column rank, so rank deficiency can only be numerical and only the part in front of the
    triangular solve sees it: with mu = 0 that part must return the minimum-norm least-squares solution, not 1 / sigma_min times rounding."""
    T = DT[prec]
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(5)
    n, k = 60, 6
    F = rng.standard_normal((n, k)).astype(T)
    F[:, 5] = F[:, 2]                                                        # rank 5: the last singular value is rounding
    H = rng.standard_normal((n, 2)).astype(T)
    Y, sg = rm.filtered_solution(F, [0.0], H, T)
    sg = sg.astype(np.float64)
    assert sg[-1] <= n * eps * sg[0] < sg[-2]                                # one value below the cut, the others above
    want = np.linalg.lstsq(F.astype(np.float64), H.astype(np.float64), rcond=n * eps)[0]
    err = _relmax(Y.astype(np.float64), want)
    print(f"{prec}: sigma = {sg}, error against the minimum-norm solution {err:.3g}")
    assert np.all(np.isfinite(Y)) and err <= 64 * (sg[0] / sg[-2]) * eps
    # the filter itself: exactly 0 below the cut, finite above; without the cut the factor is 1 / sigma
    C = np.ones((k, 1), dtype=T)
    cut = rm.ridge_filter(C, sg.astype(T), [0.0], n * eps)
    assert cut[-1, 0] == 0 and np.all(np.isfinite(cut)) and np.all(cut[:-1, 0] > 0)
    if sg[-1] > 0:
        raw = rm.ridge_filter(C, sg.astype(T), [0.0], 0.0)
        assert raw[-1, 0] > 1e3 * raw[0, 0]
    kept = rm.ridge_filter(C, sg.astype(T), [1e-3], 1.0)                    # mu > 0: nothing is cut, whatever rcond says
    assert np.all(kept[:, 0] > 0) or sg[-1] == 0


def test_filter_model_values():
    got = rm.ridge_filter(np.array([[2.0, 2.0], [3.0, 3.0]]), np.array([2.0, 0.5]), np.array([0.0, 1.0]), 0.3)
    assert np.allclose(got.astype(np.float64), [[2.0 / 2.0, 2.0 * 2.0 / 5.0], [0.0, 3.0 * 0.5 / 1.25]], rtol=1e-15)
    assert got[1, 0] == 0


def test_cxx_layer_instantiates_in_both_precisions():
    """krill_restricted_rpchol, krill_restricted and krr_predict_restricted, double and float, host compiler only"""
    src = """#include "RandLAPACK_amd.hh"
namespace RL = RandLAPACK;
using RNG = r123::Philox4x32;
template <typename T>
void use(blas::Queue& q, const T* X, const T* H, const T* Z, T* alpha, T* Y, int64_t* S) {
    std::vector<T> regs{(T)0.1, (T)0.2, (T)0.3};
    RL::linops::RBFKernelMatrix<T> G(100, X, 5, (T)1.5, regs, q, 8);
    G.set_kernel(RL::PDKernel::Matern52);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t k = 10;
    RL::KrillRestrictedInfo info;
    state = RL::krill_restricted_rpchol(100, G, 3, H, 104, k, S, alpha, 12, state);
    state = RL::krill_restricted_rpchol(100, G, 3, H, 104, k, S, alpha, 12, state, 4, &info);
    static_assert(std::is_same<decltype(info.w_status), int>::value && std::is_same<decltype(info.c_status), int>::value, "status codes");
    int64_t rc = RL::krill_restricted(100, G, 3, H, 104, k, (const int64_t*)S, alpha, 12);
    (void)rc;
    RL::krr_predict_restricted(G, k, (const int64_t*)S, 30, Z, 5, 3, (const T*)alpha, 12, Y, 30);
}
template void use<double>(blas::Queue&, const double*, const double*, const double*, double*, double*, int64_t*);
template void use<float>(blas::Queue&, const float*, const float*, const float*, float*, float*, int64_t*);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_library_exports_the_restricted_entry_points():
    from randlapack_amd import _lib

    lib = _lib.load()
    for name in ("rlhip_ridge_filter", "rlhip_drv_krill_restricted_rpchol_pdk", "rlhip_drv_krill_restricted_pdk", "rlhip_drv_krr_predict_restricted_pdk"):
        for suf in ("f64", "f32"):
            assert hasattr(lib, f"{name}_{suf}")
    assert lib.rlhip_ridge_filter_f64(None, 1, 1, None, None, 1, ctypes.c_double(0.0), None, 1) == -1
    assert lib.rlhip_ridge_filter_f32(None, 1, 1, None, None, 1, ctypes.c_float(0.0), None, 1) == -1
    from randlapack_amd import device as dev

    for fn in ("ridge_filter", "krill_restricted_rpchol_pdk", "krill_restricted_pdk", "krr_predict_restricted_pdk"):
        assert callable(getattr(dev, fn))
    hdr = (ROOT / "include" / "RandLAPACK_amd" / "rl_krill.hh").read_text()
    for name in ("krill_restricted_rpchol", "krill_restricted(", "krr_predict_restricted", "struct KrillRestrictedInfo"):
        assert name in hdr
