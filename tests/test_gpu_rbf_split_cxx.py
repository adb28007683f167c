"""The fused cross apply split over X from a C++ caller: tests/cxx/rbf_split_caller.cpp is a user program written against
RandLAPACK_amd.hh that calls set_split_x(true) on an RBFCrossKernel and on a matrix-free RBFKernelMatrix, reads the split counter and checks
that RLHIP_OPT_RBF_FUSED is restored after every call.  Built here with plain g++ against librlhip.so by `make -C tests/cxx -f rbf_split.mk`
and run on the device."""
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def _build():
    subprocess.run(["make", "-C", str(CXX), "-f", "rbf_split.mk", "-s"], check=True)
    return CXX / "rbf_split_caller"


def test_rbf_split_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    exe = _build()
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    assert "rlhip_rbf_split_count" in out and "rlhip_rbf_split_chunks" in out and "rlhip_rbf_cross_apply_f32" in out


@pytest.mark.gpu
def test_set_split_x_from_a_cxx_caller():
    """every check is made by the program itself: the products, the split counter, the restored option"""
    r = subprocess.run([str(_build())], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    assert "SPLIT<double>" in r.stdout and "SPLIT<float>" in r.stdout
