"""The predictive variance of restricted kernel ridge regression from a C++ caller: tests/cxx/krr_var_caller.cpp is a user
program written against RandLAPACK_amd.hh (each of the four restricted fits with a KrillRestrictedBasis -> krr_predict_restricted_var).  Built
here with plain g++ against librlhip.so by `make -C tests/cxx -f krr_var.mk` and run on the device."""
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def _build():
    subprocess.run(["make", "-C", str(CXX), "-f", "krr_var.mk", "-s"], check=True)
    return CXX / "krr_var_caller"


def test_krr_var_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    exe = _build()
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_pdk_cross_var_f64" in out and "rlhip_pdk_cross_var_f32" in out


@pytest.mark.gpu
def test_fits_with_a_basis_and_variance_from_a_cxx_caller():
    """every check is made by the program itself: the four fits keep their bits, the variance's range, the far points, the k = n identity with
    the full Gaussian process, three refused calls"""
    r = subprocess.run([str(_build())], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    assert "KRR var<double>" in r.stdout and "KRR var<float>" in r.stdout
