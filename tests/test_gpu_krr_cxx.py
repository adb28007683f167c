"""Kernel ridge regression from a C++ caller: tests/cxx/krr_caller.cpp is a user program written from scratch against RandLAPACK_amd.hh
(RBFKernelMatrix -> krill_full_rpchol -> RBFCrossKernel -> krr_predict), built with plain g++ against librlhip.so by `make -C tests/cxx -f krr.mk`
(__graft_entry__.build()) and run on the device here."""
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def test_krr_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    subprocess.run(["make", "-C", str(CXX), "-f", "krr.mk", "-s"], check=True)
    exe = CXX / "krr_caller"
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_rbf_cross_apply_f64" in out and "rlhip_rbf_cross_apply_f32" in out and "rlhip_sqexp_cross_submatrix_f64" in out


@pytest.mark.gpu
def test_krr_fit_and_predict_from_a_cxx_caller():
    """every check is made by the program itself: the fit, the prediction, Op::Trans against the swapped operator bit for bit"""
    exe = CXX / "krr_caller"
    if not exe.exists():
        subprocess.run(["make", "-C", str(CXX), "-f", "krr.mk", "-s"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    assert "KRR<double>" in r.stdout and "KRR<float>" in r.stdout
