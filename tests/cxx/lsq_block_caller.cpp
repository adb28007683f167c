// A user program for least squares with several right-hand sides, written against RandLAPACK_amd.hh: the sap_lstsq overload
// with s = 4 right-hand sides, in double and float, on data given by closed formulas (exact in both precisions) that
// tests/test_gpu_lsq_block_cxx.py restates in numpy.  The program prints the rank, the iterations of every column and every entry of X and
// Y, one per line: `<precision> rank <r>`, `<precision> iters <column> <count>`, `<precision> X|Y <column> <row> <value>`; the test compares
// them with numpy's least-squares solution.  Checked here: the padding of X and Y stays untouched, the state moved, and two invalid calls throw.
// Built with the host compiler by `make -C tests/cxx -f lsq_block.mk`; ends with PASSED.
#include "RandLAPACK_amd.hh"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace RL = RandLAPACK;

template <typename T>
struct dev_array {
    T* p;
    dev_array(std::vector<T> const& h) : p(blas::device_malloc<T>((int64_t)h.size())) { blas::copy_to_device((int64_t)h.size(), h.data(), p); }
    dev_array(dev_array const&) = delete;
    ~dev_array() { blas::device_free(p); }
    std::vector<T> host(int64_t n) const {
        std::vector<T> h((size_t)n);
        blas::copy_to_host(n, p, h.data());
        blas::default_queue().sync();
        return h;
    }
};

static int failures = 0;

template <typename T>
void run(const char* name, T tol) {
    const int64_t m = 600, n = 10, s = 4, ldb = m + 3, ldx = n + 2, ldy = m + 1;
    std::vector<T> A((size_t)(m * n)), B((size_t)(ldb * s), (T)0);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) A[(size_t)(i + j * m)] = (T)((7 * i + 3 * j * j + i * j) % 17 - 8) / (T)8 + (i % n == j ? (T)2 : (T)0);
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < m; ++i) B[(size_t)(i + c * ldb)] = (T)((5 * i + 11 * c + i * c) % 32 - 16) / (T)16;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    blas::Queue& q = blas::default_queue();
    dev_array<T> Ad(A), Bd(B), Xd(std::vector<T>((size_t)(ldx * s), nan)), Yd(std::vector<T>((size_t)(ldy * s), nan));

    RandBLAS::RNGState<r123::Philox4x32> state(11);
    const auto before = state;
    const RL::SapLstsqBlockResult res =
        RL::sap_lstsq(m, n, (const T*)Ad.p, m, s, (const T*)Bd.p, ldb, (const T*)nullptr, n, (T)0, (T)4, (int64_t)4, tol, (int64_t)50, Xd.p, ldx, Yd.p, ldy, state, q);
    std::printf("%s rank %lld\n", name, (long long)res.rank);
    if ((int64_t)res.iters.size() != s) { ++failures; std::printf("FAILED %s: iters has %zu entries\n", name, res.iters.size()); }
    for (int64_t c = 0; c < (int64_t)res.iters.size(); ++c) std::printf("%s iters %lld %lld\n", name, (long long)c, (long long)res.iters[(size_t)c]);
    bool moved = false;
    for (int i = 0; i < 4; ++i) moved = moved || state.counter[i] != before.counter[i];
    if (!moved) { ++failures; std::printf("FAILED %s: the state was not advanced\n", name); }
    const std::vector<T> X = Xd.host(ldx * s), Y = Yd.host(ldy * s);
    for (int64_t c = 0; c < s; ++c) {
        for (int64_t i = 0; i < n; ++i) std::printf("%s X %lld %lld %.17g\n", name, (long long)c, (long long)i, (double)X[(size_t)(i + c * ldx)]);
        for (int64_t i = 0; i < m; ++i) std::printf("%s Y %lld %lld %.17g\n", name, (long long)c, (long long)i, (double)Y[(size_t)(i + c * ldy)]);
        for (int64_t i = n; i < ldx; ++i)
            if (!std::isnan((double)X[(size_t)(i + c * ldx)])) { ++failures; std::printf("FAILED %s: the padding of X column %lld was written\n", name, (long long)c); }
        for (int64_t i = m; i < ldy; ++i)
            if (!std::isnan((double)Y[(size_t)(i + c * ldy)])) { ++failures; std::printf("FAILED %s: the padding of Y column %lld was written\n", name, (long long)c); }
    }
    // refused: more columns than rows, and a negative number of right-hand sides
    int thrown = 0;
    try { RL::sap_lstsq(n - 1, n, (const T*)Ad.p, m, s, (const T*)Bd.p, ldb, (const T*)nullptr, n, (T)0, (T)4, (int64_t)4, tol, (int64_t)5, Xd.p, ldx, Yd.p, ldy, state, q); } catch (RL::Error const&) { ++thrown; }
    try { RL::sap_lstsq(m, n, (const T*)Ad.p, m, (int64_t)-1, (const T*)Bd.p, ldb, (const T*)nullptr, n, (T)0, (T)4, (int64_t)4, tol, (int64_t)5, Xd.p, ldx, Yd.p, ldy, state, q); } catch (RL::Error const&) { ++thrown; }
    if (thrown != 2) { ++failures; std::printf("FAILED %s: %d of 2 invalid calls threw\n", name, thrown); }
}

int main() {
    run<double>("double", 1e-10);
    run<float>("float", 1e-4f);
    std::printf(failures ? "FAILED\n" : "PASSED\n");
    return failures ? 1 : 0;
}
