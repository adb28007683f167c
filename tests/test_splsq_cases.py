"""The no-GPU half of sparse least squares (randlapack_amd/csrc/spmv.hip; SparseLinOp overloads of pcg_saddle, rpc_data_svd_saso and
sap_lstsq): the cases the device test runs are what it says they are, the numpy model converges on the sparse problems it is the yardstick
for, the new C++ overloads instantiate with g++ alone and the ctypes table knows the new entry points."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _lsq_model as lm
import _splsq_cases as sc

ROOT = Path(__file__).resolve().parent.parent


def test_constants_match_the_header():
    text = (ROOT / "include" / "rlhip.h").read_text()
    assert f"#define RLHIP_SPMV_CHUNK {sc.CH}\n" in text and f"#define RLHIP_SPMV_X_LDS_BYTES {sc.X_LDS_BYTES}\n" in text
    assert "RLHIP_OPT_SPMV_LANES = 13," in text and "RLHIP_OPT_COUNT = 14" in text


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_exact_cases_are_exact_in_any_order(prec):
    """values, operands and scalars are such that every partial sum of every product the device test checks is an integer or a half-integer
    below 2^23 in absolute value: fp32 and fp64 then hold each of them exactly, whatever the order of summation"""
    cases = sc.exact_cases(prec)
    T = {"f64": np.float64, "f32": np.float32}[prec]
    lim = sc.lds_limit(T)
    seen_rows, seen_cols, seen_len = set(), set(), set()
    for cs in cases:
        rp, ci, v = cs["rowptr"], cs["colidx"], cs["vals"]
        assert rp[0] == 0 and rp[-1] == ci.size == v.size and np.all(np.diff(rp) >= 0)
        assert ci.size == 0 or (ci.min() >= 0 and ci.max() < cs["ncols"])
        assert set(np.unique(v)) <= {-1.0, 0.0, 1.0}
        assert sc.exact_sum_bound(cs) < 2 ** 23, cs["name"]
        # the transpose holds the same entries, each transposed row in ascending source row
        rpt, cit, vt = cs["rowptr_t"], cs["colidx_t"], cs["vals_t"]
        assert rpt[-1] == ci.size and np.array_equal(sc.densify(cs["ncols"], cs["nrows"], rpt, cit, vt), cs["A"].T)
        assert all(np.all(np.diff(cit[rpt[j]:rpt[j + 1]]) >= 0) for j in range(cs["ncols"]))
        seen_rows.add(cs["nrows"])
        seen_cols.add(cs["ncols"])
        seen_len |= set(np.diff(rp).tolist())
    assert set(sc.NROWS) <= seen_rows and set(sc.NCOLS) | {lim, lim + 1} <= seen_cols
    assert set(sc.ROW_LENGTHS) | set(sc.LONG_LENGTHS) <= seen_len
    assert any(np.any(cs["vals"] == 0.0) for cs in cases)                          # explicit stored zeros
    assert any(cs["name"] == "all-empty" and cs["colidx"].size == 0 for cs in cases)
    # the default routes met on the forward or the transposed structures: 64 lanes per row are the default only beyond 512 rows of mean
    # length 1024 and more, which no exact case has (the device test forces it)
    routes = {sc.default_route(cs["nrows"], cs["colidx"].size) for cs in cases if cs["colidx"].size}
    routes |= {sc.default_route(cs["ncols"], cs["colidx"].size) for cs in cases if cs["colidx"].size}
    assert routes == {0, 4, 16}


@pytest.mark.parametrize("idx", range(len(lm.CONV_SHAPES)))
def test_sparse_convergence_cases_in_the_model(idx):
    """the yardstick of the device test: the model on the densified matrix converges inside lm.CONV_ITER_LIM, with rank n in fp64"""
    cs = sc.conv_case(idx)
    m, n = cs["m"], cs["n"]
    lengths = np.diff(cs["rowptr"])
    assert np.all(lengths[::97] == 0) and lengths[5] == n and set(lengths.tolist()) == {0, sc.CONV_ROW_NNZ[idx], n}
    assert all(np.all(np.diff(cs["colidx"][cs["rowptr"][r]:cs["rowptr"][r + 1]]) > 0) for r in range(m))    # canonical: sorted, no duplicates
    r = sc.conv_model(idx, "f64")
    cnd = lm.cond(r["A"].astype(np.float64) @ r["M"].astype(np.float64))
    print(f"({m}, {n}) {sc.CONV_ROW_NNZ[idx]} per row: fp64 iters={r['iters']} rank={r['rank']} ratio={r['ratio']:.3g} cond(A M)={cnd:.3g}")
    assert r["rank"] == n and r["iters"] < lm.CONV_ITER_LIM and r["ratio"] <= 10 * lm.CONV_TOL[np.float64]
    r32 = sc.conv_model(idx, "f32")
    print(f"  fp32: iters={r32['iters']} rank={r32['rank']} ratio={r32['ratio']:.3g}")
    assert r32["iters"] < lm.CONV_ITER_LIM
    rd = sc.conv_model(idx, "f64", 0.1)
    print(f"  delta = 0.1: iters={rd['iters']} rank={rd['rank']} ratio={rd['ratio']:.3g}")
    assert rd["rank"] == n and rd["iters"] < lm.CONV_ITER_LIM


def test_sparse_overloads_instantiate_with_gxx_alone():
    src = """#include "RandLAPACK_amd.hh"
using RNG = r123::Philox4x32;
using State = RandBLAS::RNGState<RNG>;
namespace lo = RandLAPACK::linops;
#define INST(T) \\
  template void lo::SparseLinOp<T>::matvec(RandLAPACK::Op, T, const T*, T, T*); \\
  template void lo::SparseLinOp<T>::normal_matvec(const T*, T, T*, T*, T*); \\
  template void lo::DenseLinOp<T>::matvec(RandLAPACK::Op, T, const T*, T, T*); \\
  template void lo::DenseLinOp<T>::normal_matvec(const T*, T, T*, T*, T*); \\
  template void RandLAPACK::pcg_saddle<T, lo::SparseLinOp<T>>(lo::SparseLinOp<T>&, const T*, const T*, T, int64_t, T*, T, int64_t, const T*, int64_t, \\
                                          const T*, T*, T*, int64_t*); \\
  template void RandLAPACK::pcg_saddle<T, lo::DenseLinOp<T>>(lo::DenseLinOp<T>&, const T*, const T*, T, int64_t, T*, T, int64_t, const T*, int64_t, \\
                                          const T*, T*, T*, int64_t*); \\
  template void RandLAPACK::rpc_data_svd<T, RandBLAS::SparseSkOp<T, RNG>>(RandLAPACK::Layout, lo::SparseLinOp<T>&, RandBLAS::SparseSkOp<T, RNG>&, T*, T*); \\
  template State RandLAPACK::rpc_data_svd_saso<T, RNG>(RandLAPACK::Layout, lo::SparseLinOp<T>&, int64_t, int64_t, T*, T*, State); \\
  template RandLAPACK::SapLstsqResult RandLAPACK::sap_lstsq<T, RNG>(lo::SparseLinOp<T>&, const T*, const T*, T, T, int64_t, T, int64_t, T*, T*, State&, T*);
INST(double)
INST(float)
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)


def test_ctypes_table_has_the_sparse_entry_points():
    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    want = ["rlhip_spmv_path_count"]
    for suf in ("f64", "f32"):
        want += [f"rlhip_{name}_{suf}" for name in ("csr_spmv", "csr_normal_matvec", "drv_pcg_saddle_linop", "drv_rpc_data_svd_saso_linop",
                                                   "drv_sap_lstsq_linop")]
    missing = [n for n in want if n not in _lib.SIGNATURES]
    assert not missing, missing
    lib = _lib.load()
    assert lib.rlhip_spmv_path_count(None, 50) == -1
    assert dev.Context.OPT["spmv_lanes"] == 13
    for name in ("csr_spmv", "csr_normal_matvec", "pcg_saddle_op", "rpc_data_svd_saso_op", "sap_lstsq_op"):
        assert callable(getattr(dev, name))
