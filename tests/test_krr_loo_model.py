"""No GPU.  (1) The numpy model of the regularization path of restricted kernel ridge regression (tests/_krr_loo_model.py): the
leave-one-out shortcut against brute-force refits of the rows of F and against the dense restricted fit refitted without a point, the
selection rules; (2) the inputs of the driver tests in tests/test_gpu_krr_loo.py have what those tests rely on: a minimum strictly inside
the grid and a gap to the runner-up far above the allowed error; (3) the C++ layer (krill_restricted_rpchol_cv, krill_restricted_cv)
instantiates in both precisions with the host compiler alone; (4) the library exports the new entry points.  (3) and (4) fail before the
feature.

Where the tolerances come from.  A refit solves normal equations, relative error about cond(F^T F + mu I) eps_64 in the coefficients; the
shortcut divides by 1 - s_i, which amplifies the rounding of s_i by 1 / (1 - s_i).  The tests compute both and allow 64 times their sum."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _krr_loo_model as lm
import _krr_restricted_model as rm
import _pdk_model as pk

ROOT = Path(__file__).resolve().parent.parent
DT = {"f64": np.float64, "f32": np.float32}
EPS64 = float(np.finfo(np.float64).eps)
# the driver shapes: SHAPES and BANDWIDTH of tests/test_gpu_krr_restricted.py without the row whose 48 points are all centres
SHAPES = [(130, 2, 16, 16, 1), (300, 3, 24, 8, 3), (515, 5, 40, 16, 4)]
BANDWIDTH = {130: (0.12, 0.25, 0.15), 300: (0.25, 0.25, 0.25), 515: (0.35, 0.5, 0.5)}
KEY = (7, 0)


@pytest.mark.parametrize("n,k", [(130, 16), (300, 24), (515, 40), (65, 33), (48, 48)])
def test_shortcut_equals_brute_force_refits(n, k):
    rng = np.random.default_rng(n + k)
    F = rng.standard_normal((n, k)) * (0.7 ** np.arange(k))[None, :]
    H = rng.standard_normal((n, 2))
    U, sg, _ = np.linalg.svd(F, full_matrices=False)
    C = U.T @ H
    worst = 0.0
    for mu in lm.GRID:
        e, _, t, _ = lm.rows(U, sg, C, H, [mu])
        want = lm.brute_force(F, H, mu)
        cond = (sg[0] ** 2 + mu) / (sg[-1] ** 2 + mu)
        allowed = 64 * EPS64 * (cond + 1 / float(t.min()))
        err = float(np.max(np.abs(e[:, 0, :].astype(np.float64) - want)) / np.max(np.abs(want)))
        worst = max(worst, err / allowed)
        print(f"n={n} k={k} mu={mu:g}: relative difference {err:.3g}, allowed {allowed:.3g}, min (1 - s_i) {float(t.min()):.3g}")
        assert err <= allowed
    print(f"largest difference / allowed: {worst:.3g}")


@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shortcut_equals_the_dense_fit_without_a_non_centre_point(shape, kind):
    """Row i of F depends on point i and the centres only, so for a point that is no centre the shortcut is the leave-one-out residual of
    restricted kernel ridge regression with the centres held fixed: model (a) of tests/_krr_restricted_model.py on the other n - 1 points,
    evaluated at the point left out.  Held to the accuracy tests/test_krr_restricted_model.py holds model (b) to (a)."""
    n, rows_x, k, b, s = shape
    X, H = lm.problem(n, rows_x, s, np.float64)
    l = BANDWIDTH[n][kind]
    f = rm.factor(kind, X, l, k, b, np.float64, key=KEY)
    S = f["S"]
    U, sg, _ = np.linalg.svd(f["F"], full_matrices=False)
    mus = [1e-4, 1e-2, 1.0]
    e, _, _, _ = lm.rows(U, sg, U.T @ H, H, mus)
    others = [i for i in range(n) if i not in set(S.tolist())]
    for i in (others[0], others[len(others) // 2], others[-1]):
        keep = np.arange(n) != i
        S_in = np.searchsorted(np.flatnonzero(keep), S)                      # the centres' indices among the n - 1 points kept
        for m, mu in enumerate(mus):
            alpha, KS = rm.truth(kind, X[:, keep], l, S_in, [mu], H[keep])
            ki = pk.cross_kernel(kind, X[:, [i]], X[:, S], l)
            want = H[i] - (ki @ alpha)[0]
            mag = (np.abs(ki) @ np.abs(alpha))[0] + np.abs(H[i])
            cond = max(np.linalg.cond(KS.T @ KS + mu * KS[S_in, :]), np.linalg.cond(KS[S_in, :]))
            err = float(np.max(np.abs(e[i, m, :].astype(np.float64) - want) / mag))
            print(f"{shape} kind={kind} point {i} mu={mu:g}: error {err:.3g}, allowed {8 * cond * EPS64:.3g}")
            assert err <= 8 * cond * EPS64


def test_table_sums_and_bound_on_a_hand_case():
    """k = 1, U = (0.6, 0.8)^T: s_i = u_i^2 d, yhat_i = u_i d c"""
    U = np.array([[0.6], [0.8]])
    sg, C, H, mus = np.array([2.0]), np.array([[1.5]]), np.array([[1.0], [2.0]]), np.array([0.0, 4.0])
    out = lm.table(U, sg, C, H, mus)
    for m, d in enumerate((1.0, 0.5)):
        r = np.array([1.0 - 0.6 * d * 1.5, 2.0 - 0.8 * d * 1.5])
        t = np.array([1 - 0.36 * d, 1 - 0.64 * d])
        assert np.isclose(float(out["rss"][m, 0]), np.sum(r * r), rtol=1e-15) and np.isclose(float(out["loo"][m, 0]), np.sum((r / t) ** 2), rtol=1e-15)
    assert np.all(out["bound_loo"] > 0) and np.all(out["bound_loo"] < 1e-13) and np.all(out["bound_rss"] < 1e-13)
    assert np.allclose(lm.dof(sg, mus), [1.0, 0.5])
    assert lm.d_factor([2.0, 1e-3], [0.0], 1e-2)[:, 0].tolist() == [1.0, 0.0]     # mu == 0: 1, or 0 below the cut


def test_selection_rules():
    inf, nan = np.inf, np.nan
    crit = np.array([[3.0, nan, 2.0], [1.0, inf, 2.0], [1.0, 5.0, nan], [2.0, 4.0, 7.0]])
    assert lm.select(crit).tolist() == [1, 3, 0]                             # a tie goes to the lower index; entries that are not finite are skipped
    with pytest.raises(ValueError):
        lm.select(np.array([[1.0, nan], [2.0, inf]]))
    with pytest.raises(ValueError):
        lm.select(np.array([[1.0, -inf]]))
    # generalized cross-validation: n rss / (n - dof)^2, not finite where dof == n
    g = lm.criterion(lm.GCV, 4, None, np.array([[2.0], [8.0]]), np.array([2.0, 4.0]))
    assert g[0, 0] == 4 * 2.0 / 4.0 and not np.isfinite(g[1, 0])
    assert lm.select(g).tolist() == [0]
    assert np.array_equal(lm.criterion(lm.LOO, 4, np.array([[2.0]]), None, None), [[2.0]])


@functools.lru_cache(maxsize=None)
def _driver_case(shape, kind, prec):
    T = DT[prec]
    n, rows_x, k, b, s = shape
    X, H = lm.problem(n, rows_x, s, T)
    l = BANDWIDTH[n][kind]
    fT = rm.factor(kind, X, l, k, b, T, key=KEY)
    assert fT["k"] == k
    blocks = [fT["S"][p:p + b] for p in range(0, k, b)]
    f64 = rm.factor(kind, X, l, k, b, np.float64, forced_S=blocks)
    return lm.path(f64["F"], H, lm.GRID, np.float64, n_for_rcond=n), lm.path(fT["F"], H, lm.GRID, T)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("crit", [lm.LOO, lm.GCV], ids=["loo", "gcv"])
@pytest.mark.parametrize("kind", pk.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_driver_inputs_have_an_interior_minimum_and_a_clear_runner_up(shape, kind, crit, prec):
    """what tests/test_gpu_krr_loo.py relies on, on the model's own centres: per case at least one column whose minimum lies strictly inside
    the grid, and on every column a gap to the runner-up of at least 100 times the table error that test allows -- max(8 x the error of the model in T, 64
    eps_T) of the column's largest entry -- and the model in T selects what float64 selects on every such column"""
    T = DT[prec]
    n = shape[0]
    p64, pT = _driver_case(shape, kind, prec)
    name = "loo" if crit == lm.LOO else "rss"
    t64, tT = p64[name].astype(np.float64), pT[name].astype(np.float64)
    colmax = np.max(np.abs(t64), axis=0)
    e_mod = np.max(np.abs(tT - t64), axis=0) / colmax
    allowed = np.maximum(8 * e_mod, 64 * float(np.finfo(T).eps))
    c64 = lm.criterion(crit, n, p64["loo"], p64["rss"], p64["dof"])
    cT = lm.criterion(crit, n, pT["loo"], pT["rss"], pT["dof"])
    best, gaps = lm.select(c64), lm.runner_up_gap(c64)
    used = gaps >= 100 * allowed
    interior = (best > 0) & (best < len(lm.GRID) - 1)
    print(f"{shape} kind={kind} {prec} {name}: best {best.tolist()}, gap {gaps}, 100 x allowed {100 * allowed}, model-T error {e_mod}, "
          f"min (1 - s_i) {p64['min_t']:.3g}")
    assert np.all(used) and np.any(interior)
    assert np.array_equal(lm.select(cT)[used], best[used])


def test_cxx_layer_instantiates_in_both_precisions():
    """krill_restricted_rpchol_cv and krill_restricted_cv, double and float, host compiler only"""
    src = """#include "RandLAPACK_amd.hh"
namespace RL = RandLAPACK;
using RNG = r123::Philox4x32;
template <typename T>
void use(blas::Queue& q, const T* X, const T* H, T* alpha, int64_t* S) {
    std::vector<T> regs{(T)0};
    RL::linops::RBFKernelMatrix<T> G(100, X, 5, (T)1.5, regs, q, 8);
    G.set_kernel(RL::PDKernel::Matern32);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t k = 10;
    const T grid[3] = {(T)1e-3, (T)1e-2, (T)1e-1};
    RL::KrillRestrictedInfo info;
    RL::KrillRidgePath path;
    state = RL::krill_restricted_rpchol_cv(100, G, 3, H, 104, 3, grid, RL::KrillCriterion::LeaveOneOut, k, S, alpha, 12, path, state);
    state = RL::krill_restricted_rpchol_cv(100, G, 3, H, 104, 3, grid, RL::KrillCriterion::GCV, k, S, alpha, 12, path, state, 4, &info);
    int64_t rc = RL::krill_restricted_cv(100, G, 3, H, 104, 3, grid, RL::KrillCriterion::GCV, k, (const int64_t*)S, alpha, 12, path);
    (void)rc;
    static_assert(std::is_same<decltype(path.loo), std::vector<double>>::value && std::is_same<decltype(path.rss), std::vector<double>>::value &&
                  std::is_same<decltype(path.dof), std::vector<double>>::value && std::is_same<decltype(path.best), std::vector<int64_t>>::value &&
                  std::is_same<decltype(path.best_mu), std::vector<double>>::value, "the path's members");
}
template void use<double>(blas::Queue&, const double*, const double*, double*, int64_t*);
template void use<float>(blas::Queue&, const float*, const float*, float*, int64_t*);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_library_exports_the_path_entry_points():
    from randlapack_amd import _lib

    lib = _lib.load()
    for name in ("rlhip_ridge_loo", "rlhip_drv_krill_restricted_rpchol_cv_pdk", "rlhip_drv_krill_restricted_cv_pdk"):
        for suf in ("f64", "f32"):
            assert hasattr(lib, f"{name}_{suf}") and f"{name}_{suf}" in _lib.SIGNATURES
    assert lib.rlhip_ridge_loo_f64(None, 1, 1, 1, 1, None, 1, None, None, 1, None, 1, None, ctypes.c_double(0.0), None, None) == -1
    assert lib.rlhip_ridge_loo_f32(None, 1, 1, 1, 1, None, 1, None, None, 1, None, 1, None, ctypes.c_float(0.0), None, None) == -1
    from randlapack_amd import device as dev

    for fn in ("ridge_loo", "krill_restricted_rpchol_cv_pdk", "krill_restricted_cv_pdk"):
        assert callable(getattr(dev, fn))
    hdr = (ROOT / "include" / "RandLAPACK_amd" / "rl_krill.hh").read_text()
    for name in ("krill_restricted_rpchol_cv", "krill_restricted_cv", "struct KrillRidgePath", "enum class KrillCriterion"):
        assert name in hdr
