"""No GPU.  (1) The numpy model of block / lockstep PCG (tests/_pcg_model.py) meets the reference's own check
(test/drivers/test_krill.cc:60-65) on the cases the GPU tests run; (2) its posm_square returns the reference's codes; (3) the C++ object
layer of the feature instantiates in both precisions with the host compiler alone; (4) the host half of posm_square
(include/RandLAPACK_amd/rl_determiter_host.hh) agrees with numpy when run as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _pcg_model as pm

ROOT = Path(__file__).resolve().parent.parent
DTYPES = {"f64": np.float64, "f32": np.float32}


@functools.lru_cache(maxsize=None)
def _case(name):
    c = {"dense300": lambda: pm.dense_case(), "rbf333": lambda: pm.rbf_case(333, 64), "rbf1037": lambda: pm.rbf_case(1037, 100)}[name]()
    c["V"], c["ev"] = pm.top_eigs(c["K"], c["k"])
    return c


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", pm.MODES)
@pytest.mark.parametrize("name", ["dense300", "rbf333", "rbf1037"])
def test_model_meets_the_reference_check(name, mode, s, prec):
    dt = DTYPES[prec]
    c = _case(name)
    mus = pm.mode_mus(c, mode)
    G = pm.reg_op(c["K"], mus, dt)
    N = pm.SpectralPrecond(c["V"], c["ev"], mus, dt)
    Xstar = np.random.default_rng(101).standard_normal((c["n"], s)).astype(dt)
    H = G(Xstar)
    tol = 100 * float(np.finfo(dt).eps)
    X, iters, normR, normNR = pm.pcg(G, H, tol, 30, N, np.zeros_like(H), dt)
    ratio = pm.reference_check(X, Xstar, dt)
    print(f"{name} {mode} s={s} {prec}: iters={iters} error/allowed={ratio:.3g}")
    assert ratio <= 1.0
    assert iters <= 30 and normNR[-1] < dt(tol) * (dt(1) + normNR[0])
    assert normR.size == iters + 1 and normNR.size == iters + 1


def _posm_cases():
    rng = np.random.default_rng(7)
    M = rng.standard_normal((5, 5))
    sing = np.eye(5)
    sing[:2, :2] = 1.0
    return {"pd": M @ M.T + 5 * np.eye(5), "singular": sing, "indefinite": np.diag([1.0, -1.0]), "zero": np.zeros((4, 4))}


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_model_posm_square_codes(prec):
    dt = DTYPES[prec]
    eps = float(np.finfo(dt).eps)
    cases = _posm_cases()
    for name, want in (("pd", 5), ("singular", 4), ("indefinite", -3), ("zero", -6)):
        L = cases[name]
        s = L.shape[0]
        B = np.random.default_rng(3).integers(-3, 4, size=(s, s)).astype(dt)
        code, out = pm.posm_square(L, B, dt)
        assert code == want, (name, code)
        if code < 0:
            assert np.array_equal(out, B)
        else:
            ref = np.linalg.pinv(L) @ B.astype(np.float64)
            assert np.max(np.abs(out - ref)) <= 100 * s * eps * max(1.0, np.max(np.abs(ref))), name
    # lockstep form: only the diagonals take part
    L = cases["pd"]
    B = np.arange(25, dtype=dt).reshape(5, 5) + dt(1)
    code, out = pm.posm_square(L, B, dt, diag_only=True)
    assert code == 5 and np.array_equal(out, np.diag(np.diag(out)))
    assert np.allclose(np.diag(out), np.diag(B) / np.diag(L), rtol=8 * eps)


def test_cxx_layer_instantiates_in_both_precisions():
    """SpectralPrecond, pcg over both operators and krill_full_rpchol, double and float, host compiler only (fails before the feature)"""
    src = """#include "RandLAPACK_amd.hh"
using RNG = r123::Philox4x32;
using State = RandBLAS::RNGState<RNG>;
namespace RL = RandLAPACK;
#define INST(T) \\
  template struct RL::linops::SpectralPrecond<T>; \\
  template struct RL::StatefulFrobeniusNorm<T>; \\
  template int64_t RL::posm_square<T>(int64_t, const T*, T*, T*, blas::Queue&, bool); \\
  template void RL::pcg<T, RL::linops::RegExplicitSymLinOp<T>, RL::StatefulFrobeniusNorm<T>, RL::linops::SpectralPrecond<T>>( \\
      RL::linops::RegExplicitSymLinOp<T>&, const T*, int64_t, RL::StatefulFrobeniusNorm<T>&, T, int64_t, RL::linops::SpectralPrecond<T>&, T*, bool, int64_t*); \\
  template void RL::pcg<T, RL::linops::RBFKernelMatrix<T>, RL::StatefulFrobeniusNorm<T>, RL::linops::SpectralPrecond<T>>( \\
      RL::linops::RBFKernelMatrix<T>&, const T*, int64_t, RL::StatefulFrobeniusNorm<T>&, T, int64_t, RL::linops::SpectralPrecond<T>&, T*, bool, int64_t*); \\
  template State RL::krill_full_rpchol<T, RL::linops::RBFKernelMatrix<T>, RL::StatefulFrobeniusNorm<T>, State>( \\
      int64_t, RL::linops::RBFKernelMatrix<T>&, int64_t, const T*, T*, T, State, RL::StatefulFrobeniusNorm<T>&, int64_t, int64_t, int64_t, bool, int64_t*, int64_t*);
INST(double)
INST(float)
// any other seminorm is called as in the reference, and a preconditioner without the fused norms gets a pass of its own
template <typename T> struct PlainNorm { T operator()(int64_t, int64_t, const T*) { return T(1); } };
template <typename T> struct Identity {
    void operator()(RL::Layout, int64_t, T, const T*, int64_t, T, T*, int64_t) {}
};
template void RL::pcg<double, RL::linops::RBFKernelMatrix<double>, PlainNorm<double>, Identity<double>>(
    RL::linops::RBFKernelMatrix<double>&, const double*, int64_t, PlainNorm<double>&, double, int64_t, Identity<double>&, double*, bool, int64_t*);
template void RL::pcg<float, RL::linops::RegExplicitSymLinOp<float>, RL::StatefulFrobeniusNorm<float>, Identity<float>>(
    RL::linops::RegExplicitSymLinOp<float>&, const float*, int64_t, RL::StatefulFrobeniusNorm<float>&, float, int64_t, Identity<float>&, float*, bool, int64_t*);
template RL::StatefulFrobeniusNorm<double> RL::pcg<double, RL::linops::RegExplicitSymLinOp<double>, RL::linops::SpectralPrecond<double>>(
    RL::linops::RegExplicitSymLinOp<double>&, const std::vector<double>&, double, int64_t, RL::linops::SpectralPrecond<double>&, std::vector<double>&, bool);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def _host_matrices():
    rng = np.random.default_rng(11)
    mats = list(_posm_cases().values())
    Q = np.linalg.qr(rng.standard_normal((64, 64)))[0]
    w = np.concatenate([np.linspace(0.5, 2.0, 40), np.zeros(24)])
    A = (Q * w) @ Q.T
    mats.append(0.5 * (A + A.T))                                   # PSD, rank 40
    return [(M, rng.integers(-3, 4, size=M.shape).astype(np.float64)) for M in mats]


@pytest.fixture(scope="module")
def host_program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcg_host")
    exe, data = d / "pcg_host_check", d / "mats.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    str(ROOT / "include"), str(ROOT / "tests" / "cxx" / "pcg_host_check.cpp"), "-o", str(exe)], check=True)
    mats = _host_matrices()
    with open(data, "wb") as f:
        np.array([len(mats)], dtype=np.float64).tofile(f)
        for M, B in mats:
            np.array([M.shape[0]], dtype=np.float64).tofile(f)
            np.ascontiguousarray(M.T, dtype=np.float64).tofile(f)          # column-major on disk
            np.ascontiguousarray(B.T, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(data)], check=True, capture_output=True, text=True)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    recs = {}
    for line in out.stdout.splitlines():
        head, vals = line.split(":")
        what, prec, n, code = head.split()
        recs.setdefault((what, prec), []).append((int(n), int(code), np.array(vals.split(), dtype=np.float64)))
    return mats, recs


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_eigensolver_and_fallback_under_sanitizers(host_program_output, prec):
    mats, recs = host_program_output
    dt = DTYPES[prec]
    eps = float(np.finfo(dt).eps)
    assert all(len(recs[(w, prec)]) == len(mats) for w in ("eig", "pinv", "posm"))
    for idx, (M, B) in enumerate(mats):
        n = M.shape[0]
        Mt = M.astype(dt).astype(np.float64)
        scale = max(1.0, np.linalg.norm(Mt))
        tol = 100 * n * eps * scale            # backward error of an orthogonal-similarity eigensolver: a modest multiple of n eps ||A||
        # -- eigenvalues ascending, eigenvectors orthonormal, A = V diag(w) V^T
        _, sweeps, v = recs[("eig", prec)][idx]
        assert 0 <= sweeps <= 60
        w, V = v[:n], v[n:].reshape(n, n).T
        assert np.all(np.diff(w) >= 0)
        assert np.max(np.abs(w - np.linalg.eigvalsh(Mt))) <= tol
        assert np.max(np.abs(V.T @ V - np.eye(n))) <= 100 * n * eps
        assert np.max(np.abs((V * w) @ V.T - Mt)) <= tol
        # -- psd_sqrt_pinv_host: the model's code, and pinv(A) = B B^T over the trailing columns
        code_m, _, _ = pm.psd_sqrt_pinv(Mt, dt)
        _, code, b = recs[("pinv", prec)][idx]
        assert code == code_m
        if code >= 0:
            Bm = b.reshape(n, n).T[:, code:]
            ref = np.linalg.pinv(Mt, rcond=1e-4, hermitian=True)
            assert np.max(np.abs(Bm @ Bm.T - ref)) <= 100 * n * eps * max(1.0, np.linalg.norm(ref)) ** 2
        # -- posm_square_fallback: the reference's rank / codes and pinv(LHS) RHS
        _, rank, r = recs[("posm", prec)][idx]
        Rm = r.reshape(n, n).T
        if code_m < 0:
            assert rank == code_m and np.array_equal(Rm, B)
        else:
            assert rank == n - code_m
            pinv = np.linalg.pinv(Mt, rcond=1e-4, hermitian=True)
            assert np.max(np.abs(Rm - pinv @ B)) <= 100 * n * eps * max(1.0, np.linalg.norm(pinv)) ** 2 * np.max(np.abs(B))
    codes = [c for _, c, _ in recs[("posm", prec)]]
    assert codes == [5, 4, -3, -6, 40]
