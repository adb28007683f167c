"""Restricted kernel ridge regression from a C++ caller: tests/cxx/krr_restricted_caller.cpp is a user program written against
RandLAPACK_amd.hh (RBFKernelMatrix -> krill_restricted_rpchol / krill_restricted -> krr_predict_restricted, compared with krill_full_rpchol +
krr_predict at k = n), built with plain g++ against librlhip.so by `make -C tests/cxx -f krr_restricted.mk` (__graft_entry__.build()) and
run on the device here."""
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def test_krr_restricted_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    subprocess.run(["make", "-C", str(CXX), "-f", "krr_restricted.mk", "-s"], check=True)
    exe = CXX / "krr_restricted_caller"
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_ridge_filter_f64" in out and "rlhip_ridge_filter_f32" in out and "rlhip_gather_cols_f64" in out


@pytest.mark.gpu
def test_krr_restricted_fit_and_predict_from_a_cxx_caller():
    """every check is made by the program itself: k = n against the full fit, given centres against the pivoted fit, three refused calls"""
    exe = CXX / "krr_restricted_caller"
    if not exe.exists():
        subprocess.run(["make", "-C", str(CXX), "-f", "krr_restricted.mk", "-s"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    assert "KRR restricted<double>" in r.stdout and "KRR restricted<float>" in r.stdout
