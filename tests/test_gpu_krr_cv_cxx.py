"""Restricted kernel ridge regression with the regularization chosen from a grid, from a C++ caller: tests/cxx/krr_cv_caller.cpp
is a user program written against RandLAPACK_amd.hh (RBFKernelMatrix -> krill_restricted_rpchol_cv -> krr_predict_restricted, and
krill_restricted_cv on the same centres).  Built here with plain g++ against librlhip.so by `make -C tests/cxx -f krr_cv.mk` and run on the
device."""
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def _build():
    subprocess.run(["make", "-C", str(CXX), "-f", "krr_cv.mk", "-s"], check=True)
    return CXX / "krr_cv_caller"


def test_krr_cv_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    exe = _build()
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_ridge_loo_f64" in out and "rlhip_ridge_loo_f32" in out and "rlhip_ridge_filter_f64" in out


@pytest.mark.gpu
def test_fit_with_selection_and_predict_from_a_cxx_caller():
    """every check is made by the program itself: the path, the choice, the bit-identical existing fit, the prediction, three refused calls"""
    r = subprocess.run([str(_build())], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    assert "KRR cv<double>" in r.stdout and "KRR cv<float>" in r.stdout
