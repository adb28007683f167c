"""The no-GPU half of least squares with several right-hand sides: the model of the block solver (tests/_lsq_block_model.py) on
the right-hand sides the device test uses, the C++ templates instantiated with g++ alone, the ctypes table, and the shape rule of the
one-pass normal product, which answers without a device."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _lsq_block_model as bm
import _lsq_model as lm

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("m,n,d", lm.CONV_SHAPES)
def test_iteration_counts_of_the_five_right_hand_sides(m, n, d, prec):
    """with the model's own preconditioner M: a right-hand side W u (W = A M, u eigenvectors of W^T W) spanning 1, 2 and 4 eigenvectors
    takes that many iterations in both precisions, the Gaussian column 23-30 (fp64, tol 1e-10) or 11-12 (fp32, tol 1e-4), the zero column
    none -- the numbers the device test's bounds (6, 20, 8) are set against"""
    model = lm.conv_model(m, n, d, prec)
    B = bm.conv_rhs(model["A"], model["M"], model["b"])
    r = bm.conv_block_model(model["A"], model["M"], B, prec)
    print(f"({m}, {n}, {d}) {prec}: iters {r['iters']} ratios {[None if v is None else float(f'{v:.3g}') for v in r['ratio']]}")
    assert r["iters"][1:4] == [1, 2, 4] and r["iters"][4] == 0
    lo, hi = (23, 30) if prec == "f64" else (11, 12)
    assert lo <= r["iters"][0] <= hi
    assert np.array_equal(r["X"][:, 4], np.zeros(n)) and np.array_equal(r["Y"][:, 4], np.zeros(m))
    tol = lm.CONV_TOL[bm.DT[prec]]
    assert all(v <= 10 * tol for v in r["ratio"][:4])


def test_block_model_is_the_single_model_column_by_column():
    A, B, C, delta, M, X0 = bm.three_step_block("dense300", np.float64)
    X, Y, iters, resid = bm.pcg_saddle_block(A, B, C, delta, 3, 1e-30, M, X0, np.float64)
    for j in range(3):
        x, y, it, r = lm.pcg_saddle(A, B[:, j].copy(), C[:, j].copy(), delta, 3, 1e-30, M, X0[:, j].copy(), np.float64)
        assert np.array_equal(X[:, j], x) and np.array_equal(Y[:, j], y) and iters[j] == it == 3 and np.array_equal(resid[j], r)
    assert np.any(X0[:, 1]) and not np.any(X0[:, 0])


def test_block_templates_instantiate_with_gxx_alone():
    src = """#include "RandLAPACK_amd.hh"
using RNG = r123::Philox4x32;
using State = RandBLAS::RNGState<RNG>;
#define INST(T) \\
  template void RandLAPACK::pcg_saddle_block<T>(int64_t, int64_t, const T*, int64_t, int64_t, const T*, int64_t, const T*, int64_t, T, int64_t, T*, \\
                                          int64_t, T, int64_t, const T*, int64_t, const T*, int64_t, T*, int64_t, T*, int64_t, blas::Queue&, int64_t*); \\
  template void RandLAPACK::pcg_saddle_block<T, RandLAPACK::linops::DenseLinOp<T>>(RandLAPACK::linops::DenseLinOp<T>&, int64_t, const T*, int64_t, \\
                                          const T*, int64_t, T, int64_t, T*, int64_t, T, int64_t, const T*, int64_t, const T*, int64_t, T*, int64_t, T*, \\
                                          int64_t, int64_t*); \\
  template RandLAPACK::SapLstsqBlockResult RandLAPACK::sap_lstsq<T, RNG>(int64_t, int64_t, const T*, int64_t, int64_t, const T*, int64_t, const T*, \\
                                          int64_t, T, T, int64_t, T, int64_t, T*, int64_t, T*, int64_t, State&, blas::Queue&, T*); \\
  template void RandLAPACK::linops::DenseLinOp<T>::matmat(RandLAPACK::Op, int64_t, T, const T*, int64_t, T, T*, int64_t); \\
  template void RandLAPACK::linops::DenseLinOp<T>::normal_matmat(int64_t, const T*, int64_t, T, T*, int64_t, T*, int64_t, T*);
INST(double)
INST(float)
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_ctypes_table_has_the_block_entry_points():
    from randlapack_amd import _lib

    want = ["rlhip_normal_matmat_fused", "rlhip_normal_matmat_default", "rlhip_normal_matmat_set_route", "rlhip_lsq_block_path_count"]
    for suf in ("f64", "f32"):
        want += [f"rlhip_{name}_{suf}" for name in ("normal_matmat", "pcg_saddle_block_step_xr", "pcg_saddle_block_step_refresh",
                                                   "pcg_saddle_block_step_d", "drv_pcg_saddle_block", "drv_sap_lstsq_block")]
    missing = [n for n in want if n not in _lib.SIGNATURES]
    assert not missing, missing
    lib = _lib.load()
    assert lib.rlhip_lsq_block_path_count(None, 76) == -1
    assert lib.rlhip_normal_matmat_set_route(None, 1) == -1
    assert lib.rlhip_lsq_path_count(None, 76) == -1


def _header_int(name):
    import re

    text = (ROOT / "include" / "rlhip.h").read_text()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_one_pass_shape_rule_answers_without_a_device():
    """rlhip_normal_matmat_fused(n, s, elem_bytes): 0 outside the limits stated in include/rlhip.h, else a chunk width that is at least 1,
    never larger than s and never larger than the precision's widest chunk"""
    from randlapack_amd import device as dev

    max_n = _header_int("RLHIP_NORMAL_MATMAT_FUSED_MAX_N")
    sc = {8: _header_int("RLHIP_NORMAL_MATMAT_FUSED_SC_F64"), 4: _header_int("RLHIP_NORMAL_MATMAT_FUSED_SC_F32")}
    for eb in (8, 4):
        for n in (1, 2, 33, 64, max_n - 1, max_n):
            for s in (1, 2, 3, sc[eb], sc[eb] + 1, 2 * sc[eb] + 1, 1000):
                got = dev.normal_matmat_fused(n, s, eb)
                assert got == min(s, sc[eb]) and 1 <= got <= s, (n, s, eb, got)
        for n, s in ((0, 3), (-1, 3), (max_n + 1, 3), (10 * max_n, 1), (5, 0), (5, -2)):
            assert dev.normal_matmat_fused(n, s, eb) == 0, (n, s, eb)
    for eb in (0, 2, 16, -4):
        assert dev.normal_matmat_fused(8, 4, eb) == 0 and dev.normal_matmat_default(64, 4, eb) == 0
    # the default takes the one-pass route only inside the kernel's limits, and only in the measured ranges
    for eb, lo in ((8, 33), (4, 129)):
        for n in (1, 32, 33, 64, 128, 129, 256, 257, max_n, max_n + 1):
            for s in (0, 1, 2, 3, 8, 9, 32):
                want = int(lo <= n <= 256 and 2 <= s <= 8)
                assert dev.normal_matmat_default(n, s, eb) == want and (not want or dev.normal_matmat_fused(n, s, eb)), (n, s, eb)


def test_option_count_is_unchanged():
    text = (ROOT / "include" / "rlhip.h").read_text()
    assert "RLHIP_OPT_COUNT = 15" in text
