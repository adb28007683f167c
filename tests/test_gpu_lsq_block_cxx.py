"""Least squares with several right-hand sides from a C++ caller: tests/cxx/lsq_block_caller.cpp is a user program written
against RandLAPACK_amd.hh (the sap_lstsq overload with s = 4 right-hand sides).  Built here with plain g++ against librlhip.so by
`make -C tests/cxx -f lsq_block.mk` and run on the device; it prints the rank, the iteration counts and every entry of X and Y, which are
compared here with numpy's least-squares solution of the same data."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

CXX = Path(__file__).resolve().parent / "cxx"
M, N, S = 600, 10, 4
TOL = {"double": 1e-10, "float": 1e-4}


def _build():
    subprocess.run(["make", "-C", str(CXX), "-f", "lsq_block.mk", "-s"], check=True)
    return CXX / "lsq_block_caller"


def test_lsq_block_caller_builds_and_links():
    """no GPU needed: the program compiles with the host compiler and links against the C ABI only"""
    exe = _build()
    assert exe.exists()
    out = subprocess.check_output(["nm", "-D", "--undefined-only", str(exe)], text=True)
    assert "rlhip_drv" not in out and "hip" not in out.replace("rlhip", "")
    for suf in ("f64", "f32"):
        assert f"rlhip_normal_matmat_{suf}" in out and f"rlhip_pcg_saddle_block_step_d_{suf}" in out


def _inputs():
    """the program's data, exact in float32"""
    i, j = np.arange(M)[:, None], np.arange(N)[None, :]
    A = ((7 * i + 3 * j * j + i * j) % 17 - 8) / 8.0 + 2.0 * (i % N == j)
    c = np.arange(S)[None, :]
    B = ((5 * i + 11 * c + i * c) % 32 - 16) / 16.0
    return A, B


@pytest.mark.gpu
def test_sap_lstsq_with_four_right_hand_sides_from_a_cxx_caller():
    """x against numpy's least-squares solution: conjugate gradients stopped at a relative preconditioned residual of tol leaves a relative
    error of at most cond(A M) tol <= 10 tol in the preconditioned variable, cond(A) times that in x; 10 times that is allowed.  y against
    b - A x of the returned x within the rounding of that product, (n + 2) eps (|b| + |A| |x|)."""
    r = subprocess.run([str(_build())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-2000:] + r.stderr
    A, B = _inputs()
    cond = np.linalg.cond(A)
    Xs = np.linalg.lstsq(A, B, rcond=None)[0]
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        f = line.split()
        if f[1] == "rank":
            got.setdefault(f[0], dict(X=np.full((N, S), np.nan), Y=np.full((M, S), np.nan), iters={}))["rank"] = int(f[2])
        elif f[1] == "iters":
            got[f[0]]["iters"][int(f[2])] = int(f[3])
        else:
            got[f[0]][f[1]][int(f[3]), int(f[2])] = float(f[4])
    assert set(got) == {"double", "float"}
    for name, g in got.items():
        T = np.float64 if name == "double" else np.float32
        eps = float(np.finfo(T).eps)
        assert g["rank"] == N and sorted(g["iters"]) == list(range(S)) and all(1 <= v < 50 for v in g["iters"].values())
        err = np.linalg.norm(g["X"] - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
        allowed = 10 * 10 * TOL[name] * cond
        yerr = np.abs(g["Y"] - (B - A @ g["X"]))
        ybound = (N + 2) * eps * (np.abs(B) + np.abs(A) @ np.abs(g["X"]))
        print(f"<{name}> cond(A) {cond:.3g}, iters {g['iters']}: relative error of x per column {np.array2string(err, precision=3)}, allowed {allowed:.3g}; "
              f"max |y - (b - A x)| / bound {np.max(yerr / ybound):.3g}")
        assert np.all(err <= allowed) and np.all(yerr <= ybound)
