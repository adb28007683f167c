"""Kernel ridge regression with a Matern 5/2 kernel from a C++ caller: tests/cxx/pdk_caller.cpp is a user program written from scratch against
RandLAPACK_amd.hh (RBFKernelMatrix::set_kernel -> krill_full_rpchol -> RBFCrossKernel::set_kernel -> krr_predict), built with plain g++ against
librlhip.so by `make -C tests/cxx -f pdk.mk` (__graft_entry__.build()) and run on the device here."""
import re
import subprocess
from pathlib import Path

import pytest

CXX = Path(__file__).resolve().parent / "cxx"


def test_pdk_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only, the Matern entries among it"""
    subprocess.run(["make", "-C", str(CXX), "-f", "pdk.mk", "-s"], check=True)
    exe = CXX / "pdk_caller"
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    for name in ("rlhip_pdk_columns", "rlhip_pdk_apply", "rlhip_pdk_cross_apply", "rlhip_pdk_cross_submatrix"):
        assert f"{name}_f64" in out and f"{name}_f32" in out


@pytest.mark.gpu
def test_matern_fit_and_predict_from_a_cxx_caller():
    """the program checks itself; the residual of (K + mu I) x = h is asserted here once more from the line it prints: PCG stopped below
    tol (1 + |N R_0|), the preconditioner's eigenvalues lie in [(lambda_k + mu) / (lambda_1 + mu), 1] and lambda_1 <= n, so
    |H - (K + mu I) X|_F < tol (1 + |H|_F) (n + mu) / mu"""
    exe = CXX / "pdk_caller"
    if not exe.exists():
        subprocess.run(["make", "-C", str(CXX), "-f", "pdk.mk", "-s"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr
    lines = re.findall(r"PDK<(\w+)> kernel=matern52 n=(\d+) k=(\d+) iters=(\d+) max_iters=(\d+) tol=(\S+) mu=(\S+) normH=(\S+) resid=(\S+)", r.stdout)
    assert [ln[0] for ln in lines] == ["double", "float"]
    for _, n, _, iters, max_iters, tol, mu, normH, resid in lines:
        assert int(iters) < int(max_iters)
        assert float(resid) <= float(tol) * (1 + float(normH)) * (int(n) + float(mu)) / float(mu)
