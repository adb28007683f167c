"""The numpy restatement of RPCholesky (tests/_rpchol_model.py) against the reference's own tests (test/comps/test_rpchol.cc), and the C++
object layer's RPCholesky / RBF kernel headers compiled against the C ABI alone.  No GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _rpchol_model as M

ROOT = Path(__file__).resolve().parent.parent
SEEDS = range(2012, 2019)


def _check_exact(A, r, atol, rtol, n):
    F = r["F"]
    assert r["k"] == n
    np.testing.assert_allclose(F @ F.T, A, atol=atol, rtol=rtol)
    S = r["S"]
    assert len(set(S.tolist())) == n                                          # test_rpchol.cc:50-56
    if n > 4:
        assert not np.all(np.diff(S) > 0)                                     # :57-59


@pytest.mark.parametrize("n,b,p", [(5, 1, 2), (10, 1, 1), (10, 1, 2), (13, 1, 2), (100, 1, 2), (10, 2, 1), (10, 2, 2), (100, 2, 2)])
def test_exact_diag(n, b, p):
    """test_exact_diag_b1 / _b2 (test_rpchol.cc:114-135), float as there"""
    T = np.float32
    A = np.diag((np.arange(n) + 1.0) ** p).astype(T)
    tol = np.sqrt(n) * np.finfo(T).eps
    for seed in SEEDS:
        r = M.rp_cholesky_dense(A, n, b, seed=seed, dtype=T)
        _check_exact(A, r, tol * np.abs(A).max(), tol, n)
        assert r["status"] == 1                                               # everything picked: the remaining weight is zero


@pytest.mark.parametrize("b,sizes", [(2, (10, 11, 12)), (3, (9, 10, 11, 12))])
def test_exact_kahan_gram(b, sizes):
    """test_exact_kahan_gram_b2 / _b3 (test_rpchol.cc:145-170) with the reference's tolerance rule (:84-96)"""
    T = np.float32
    for seed in SEEDS:
        for n in sizes:
            if (b, n, seed) == (3, 10, 2017):
                continue                                                      # skipped by the reference too (:160-165)
            G, K = M.kahan_gram(n, dtype=T)
            U, info = M.potrf_upper(G)                                        # in T, as lapack::potrf on the float Gram matrix (:88)
            assert info == 0
            atol = T(np.sqrt(n)) * np.max(np.minimum(np.abs(K - U), np.abs(K + U)))
            r = M.rp_cholesky_dense(G, n, b, seed=seed, dtype=T)
            assert r["k"] == n and len(set(r["S"].tolist())) == n
            np.testing.assert_allclose(r["F"] @ r["F"].T, G, atol=atol, rtol=atol)


def test_sampler_definition():
    rng = np.random.default_rng(0)
    d = rng.random(1000) * (rng.random(1000) > 0.3)
    prefix, total, last = M.prefix_sums(d)
    assert np.all(np.diff(prefix) >= 0) and prefix[-1] == total
    idx, st, nxt = M.sample(d, 501, (5, 0, 0, 0), (9, 1))
    assert st == 0 and nxt == (5 + 251, 0, 0, 0)
    assert np.all(d[idx] > 0)                                                 # a zero weight is never drawn
    u = M.uniforms(501, (5, 0, 0, 0), (9, 1))
    assert np.all((u > 0) & (u < 1))
    # one-hot weights always give the hot index
    oh = np.zeros(700); oh[333] = 2.0
    assert np.all(M.sample(oh, 64, (0, 0, 0, 0), (1, 0))[0] == 333)


def test_status_codes():
    assert M.weights_status(np.zeros(10), np.float64) == 1
    assert M.weights_status(np.array([1.0, -1e-3]), np.float64) == 2
    assert M.weights_status(np.array([1.0, np.nan]), np.float64) == 2
    assert M.weights_status(np.array([1.0, -1e-17]), np.float64) == 0       # above -eps: clamped to zero weight
    idx, st, nxt = M.sample(np.zeros(10), 4, (3, 0, 0, 0), (0, 0))
    assert st == 1 and idx.size == 0 and nxt == (3, 0, 0, 0)                # nothing drawn, the state does not advance
    # exact rank r: stops once the weight is gone, status 1
    rng = np.random.default_rng(1)
    Q = rng.standard_normal((40, 5))
    r = M.rp_cholesky_dense(Q @ Q.T, 20, 4, seed=7)
    assert r["k"] == 5 or r["c_status"] != 0
    assert r["status"] == 1 or r["c_status"] != 0
    with pytest.raises(ValueError):
        M.rp_cholesky_dense(np.zeros((6, 6)), 3, 2, seed=1)


def test_cxx_rpchol_headers_compile_standalone():
    """rp_cholesky for both operator kinds and both precisions, rpchol_pc_data, and REVD2::call on an RBF kernel matrix instantiate against the
    C ABI alone (host compiler, no HIP headers)"""
    src = """#include "RandLAPACK_amd.hh"
using RNG = r123::Philox4x32;
using St = RandBLAS::RNGState<RNG>;
template <typename T> void inst(blas::Queue& q, const T* X, T* F, int64_t* S, std::vector<T>& regs) {
    int64_t k = 8;
    RandLAPACK::linops::RBFKernelMatrix<T> K(100, X, 3, (T)1, regs, q);
    St st = RandLAPACK::rp_cholesky(100, K, k, S, F, 4, St(0));
    RandLAPACK::linops::ExplicitSymLinOp<T> A(100, RandLAPACK::Uplo::Upper, X, 100, RandLAPACK::Layout::ColMajor, q);
    auto cb = [](int64_t) {};
    st = RandLAPACK::rp_cholesky(100, A, k, S, F, 4, st, cb);
    st = RandLAPACK::rpchol_pc_data(100, K, k, 4, F, F, st);
    RandLAPACK::squared_exp_kernel_submatrix<T>(3, 100, X, F, 10, 10, F, 0, 0, (T)1, q);
}
template void inst<double>(blas::Queue&, const double*, double*, int64_t*, std::vector<double>&);
template void inst<float>(blas::Queue&, const float*, float*, int64_t*, std::vector<float>&);
using SYPS_d = RandLAPACK::SYPS<double, RNG>; using SYRF_d = RandLAPACK::SYRF<SYPS_d, RandLAPACK::HQRQ<double>>;
template int RandLAPACK::REVD2<SYRF_d>::call(RandLAPACK::linops::RBFKernelMatrix<double>&, int64_t&, double, double*&, double*&, RandBLAS::RNGState<RNG>&);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src,
                   text=True, check=True)
