"""Gradients of kernel ridge regression predictions from a C++ caller: tests/cxx/test_krr_grad_caller.cpp is a user program
written against RandLAPACK_amd.hh (RBFCrossKernel::grad, krr_predict_grad, krr_predict_restricted_grad).  Built here with plain g++ against
librlhip.so by `make -C tests/cxx -f krr_grad.mk` and run on the device; it prints every entry of its three results, and they are compared
here with the float64 model by differences of tests/_pdk_grad_model.py under the rule of tests/test_gpu_pdk_grad.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _pdk_grad_model as gm
import _pdk_model as pk

CXX = Path(__file__).resolve().parent / "cxx"
N, ROWS_X, MZ, S, K, L = 40, 3, 9, 2, 13, 0.5


def _build():
    subprocess.run(["make", "-C", str(CXX), "-f", "krr_grad.mk", "-s"], check=True)
    return CXX / "test_krr_grad_caller"


def test_krr_grad_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    exe = _build()
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_pdk_cross_grad_f64" in out and "rlhip_pdk_cross_grad_f32" in out


def _inputs():
    """the program's data, exact in float32"""
    j, r = np.arange(N)[None, :], np.arange(ROWS_X)[:, None]
    X = ((7 * j + 3 * r * r + 1) % 64) / 64.0
    i = np.arange(MZ)[None, :]
    Z = ((3 * i + 5 * r + 2) % 128) / 128.0
    Z[:, 0] = X[:, 6]
    c = np.arange(S)[None, :]
    coef = ((5 * np.arange(N)[:, None] + 11 * c) % 32 - 16) / 16.0
    alpha = ((3 * np.arange(K)[:, None] + 7 * c) % 16 - 8) / 8.0
    return X, Z, coef, alpha, 3 * np.arange(K)


@pytest.mark.gpu
def test_gradients_from_a_cxx_caller_match_the_model():
    from test_gpu_pdk_grad import _within_model

    r = subprocess.run([str(_build())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-2000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        call, name, c, rhs, i, v = line.split()
        got.setdefault((call, name), np.full((ROWS_X, S, MZ), np.nan))[int(c), int(rhs), int(i)] = float(v)
    X, Z, coef, alpha, Sidx = _inputs()
    cases = {"grad": (pk.MATERN52, X, coef, 0.5), "predict_grad": (pk.SQEXP, X, coef, 1.0), "restricted_grad": (pk.MATERN32, X[:, Sidx], alpha, 1.0)}
    assert set(got) == {(call, name) for call in cases for name in ("double", "float")}
    for (call, name), G in got.items():
        T = np.float64 if name == "double" else np.float32
        kind, pts, B, a = cases[call]
        truth, mag = gm.cross_grad(kind, Z, pts, L, B, a)
        model = gm.emulate_grad(kind, Z, pts, L, B, T, a).astype(np.float64)
        _within_model(f"{call} <{name}>", G, model, truth, mag, T)
