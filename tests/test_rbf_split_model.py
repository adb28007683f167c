"""No GPU.  The split rule of the fused cross apply: rlhip_rbf_split_chunks is a pure function of (mz, nx), restated here in
numpy and compared with the library; the header documents value 2 of RLHIP_OPT_RBF_FUSED; the C++ setters instantiate in both precisions
with the host compiler alone.  Everything here fails before the feature: the two symbols do not exist."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
W, CH_MIN = 1024, 512

# every (mz, nx) that tests/test_gpu_krr.py hands to the cross apply: SHAPES, the limits test, the bit contract (mz = 70 and Z = X), the
# scale test, the argument codes, the matrix-free operator (999 points) and fit-then-predict (130 points against 1000)
KRR_TEST_SHAPES = [(1, 1), (17, 63), (65, 67), (200, 1000), (130, 130), (70, 1000), (1000, 1000), (5, 6), (999, 999), (130, 1000), (65, 0), (0, 67)]


def _rule(mz, nx):
    """the rule of include/rlhip.h, restated: (g, CH); CH is None where nothing is split"""
    if mz == 0 or nx == 0:
        return 1, None
    ztiles = -(-mz // 64)
    g = min(-(-W // ztiles), nx // CH_MIN)
    if g < 2:
        return 1, None
    ch = 64 * -(-nx // (64 * g))
    return -(-nx // ch), ch


@pytest.fixture(scope="module")
def lib():
    from randlapack_amd import _lib

    return _lib.load()


def test_library_exports_the_split_entries(lib):
    from randlapack_amd import device as dev

    assert hasattr(lib, "rlhip_rbf_split_chunks") and hasattr(lib, "rlhip_rbf_split_count")
    assert lib.rlhip_rbf_split_count(None) == -1
    assert lib.rlhip_rbf_split_chunks(-1, 5) <= 0 and lib.rlhip_rbf_split_chunks(5, -1) <= 0
    assert callable(dev.Context.rbf_split_count) and dev.rbf_split_chunks(70, 1100) == lib.rlhip_rbf_split_chunks(70, 1100)
    assert dev.Context.OPT["rbf_fused"] == 14 and len(dev.Context.OPT) == 15          # no option was added


def test_header_documents_value_2_and_keeps_the_option_count():
    hdr = (ROOT / "include" / "rlhip.h").read_text()
    assert "RLHIP_OPT_RBF_FUSED = 14" in hdr and "RLHIP_OPT_COUNT = 15" in hdr
    assert "RLHIP_OPT_RBF_FUSED = 2" in hdr and "Bit contract of value 2" in hdr
    assert f"#define RLHIP_RBF_SPLIT_W {W}" in hdr and f"#define RLHIP_RBF_SPLIT_CH_MIN {CH_MIN}" in hdr
    assert "int64_t rlhip_rbf_split_chunks(int64_t mz, int64_t nx);" in hdr and "int64_t rlhip_rbf_split_count(rlhip_ctx* ctx);" in hdr


def test_short_x_is_never_split(lib):
    for mz, nx in KRR_TEST_SHAPES:
        assert lib.rlhip_rbf_split_chunks(mz, nx) == 1, (mz, nx)
    for mz in (1, 63, 64, 65, 1000, 1 << 17):
        for nx in (1, 511, 512, 1000, 1023):
            assert lib.rlhip_rbf_split_chunks(mz, nx) == 1, (mz, nx)


def test_long_x_with_few_z_is_split(lib):
    for mz, nx in [(1, 1024), (70, 1100), (17, 4113)]:
        assert lib.rlhip_rbf_split_chunks(mz, nx) >= 2, (mz, nx)
    assert lib.rlhip_rbf_split_chunks(1, 1024) == 2 and lib.rlhip_rbf_split_chunks(70, 1100) == 2
    assert lib.rlhip_rbf_split_chunks(17, 4113) == 8 and lib.rlhip_rbf_split_chunks(200, 2500) == 4
    assert lib.rlhip_rbf_split_chunks(1 << 14, 1 << 17) == 4 and lib.rlhip_rbf_split_chunks(1 << 17, 1 << 17) == 1
    assert lib.rlhip_rbf_split_chunks(1, 1 << 17) == 256 and lib.rlhip_rbf_split_chunks(65537, 1 << 17) == 1


def test_rule_agrees_with_its_restatement_and_leaves_no_empty_chunk(lib):
    rng = np.random.default_rng(0)
    pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 70000, 300), rng.integers(0, 300000, 300))]
    pairs += [(mz, nx) for mz in (1, 64, 65, 1000, 4096, 16384, 65536, 65537) for nx in (1023, 1024, 1025, 1087, 1088, 4113, 65536, 131071, 131072)]
    split = 0
    for mz, nx in pairs:
        g = lib.rlhip_rbf_split_chunks(mz, nx)
        want, ch = _rule(mz, nx)
        assert g == want, (mz, nx, g, want)
        if g > 1:
            split += 1
            assert ch % 64 == 0 and ch >= CH_MIN                  # a staged tile (16, 32 or 64 points) never straddles two chunks
            assert (g - 1) * ch < nx <= g * ch                    # the last chunk is not empty, and the chunks cover X
            assert -(-mz // 64) * g <= 2 * W                      # the grid stays near the aimed-at number of work items
    assert split > 100


def test_cxx_setters_instantiate_in_both_precisions():
    """RBFCrossKernel::set_split_x, RBFKernelMatrix::set_split_x and the paths that read them, double and float, host compiler only"""
    src = """#include "RandLAPACK_amd.hh"
namespace RL = RandLAPACK;
template <typename T>
void use(blas::Queue& q, const T* Z, const T* X, const T* B, T* C, T* K, const int64_t* S) {
    RL::linops::RBFCrossKernel<T> Kzx(5, 30, Z, 2000, X, (T)1.5, q);
    Kzx.set_split_x(true);
    Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, 3, (T)1, B, 2000, (T)0, C, 30);
    Kzx.matvec(blas::Op::NoTrans, (T)1, B, (T)0, C);
    RL::krr_predict(Kzx, 3, B, 2000, C, 30);
    Kzx.set_split_x(false);
    std::vector<T> regs{(T)0.1};
    RL::linops::RBFKernelMatrix<T> G(2000, X, 5, (T)1.5, regs, q);
    G.set_matrix_free(true);
    G.set_split_x(true);
    G(blas::Layout::ColMajor, 3, (T)1, const_cast<T*>(B), 2000, (T)0, K, 2000);
    RL::krr_predict_restricted(G, 7, S, 30, Z, 5, 3, B, 7, C, 30);
}
template void use<double>(blas::Queue&, const double*, const double*, const double*, double*, double*, const int64_t*);
template void use<float>(blas::Queue&, const float*, const float*, const float*, float*, float*, const int64_t*);
int main(){return 0;}
"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-x", "c++", "-"], input=src, text=True,
                   check=True)
