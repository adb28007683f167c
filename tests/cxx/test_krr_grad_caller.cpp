// A user program for the gradients of kernel ridge regression predictions, written against RandLAPACK_amd.hh:
//   linops::RBFCrossKernel::grad, krr_predict_grad and krr_predict_restricted_grad, in double and float, on data given by closed formulas
//   (exact in both precisions) that tests/test_gpu_krr_grad_cxx.py restates in numpy.  The program prints every entry of the three results,
//   one per line: `<call> <precision> <coordinate> <right-hand side> <point> <value>`; the test compares them with its float64 model.
//   Checked here: the padding of G stays untouched, and two invalid calls throw.
// Built with the host compiler by `make -C tests/cxx -f krr_grad.mk`; ends with PASSED.
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

// prints G (rows_x x (mz s), ldg) and checks that the rows past rows_x still hold the NaN they were given
template <typename T>
void report(const char* call, const char* name, std::vector<T> const& G, int64_t rows_x, int64_t mz, int64_t s, int64_t ldg) {
    for (int64_t r = 0; r < s; ++r)
        for (int64_t i = 0; i < mz; ++i) {
            const T* col = &G[(size_t)((r * mz + i) * ldg)];
            for (int64_t c = 0; c < rows_x; ++c) std::printf("%s %s %lld %lld %lld %.17g\n", call, name, (long long)c, (long long)r, (long long)i, (double)col[c]);
            for (int64_t c = rows_x; c < ldg; ++c)
                if (!std::isnan((double)col[c])) {
                    ++failures;
                    std::printf("FAILED %s %s: the padding of column %lld was written\n", call, name, (long long)(r * mz + i));
                }
        }
}

template <typename T>
void run(const char* name) {
    const int64_t n = 40, rows_x = 3, mz = 9, s = 2, k = 13, ldg = rows_x + 2;
    const T l = (T)0.5;
    std::vector<T> X((size_t)(rows_x * n)), Z((size_t)(rows_x * mz)), coef((size_t)(n * s)), alpha((size_t)(k * s));
    for (int64_t j = 0; j < n; ++j)
        for (int64_t r = 0; r < rows_x; ++r) X[(size_t)(r + j * rows_x)] = (T)((7 * j + 3 * r * r + 1) % 64) / (T)64;
    for (int64_t i = 0; i < mz; ++i)
        for (int64_t r = 0; r < rows_x; ++r) Z[(size_t)(r + i * rows_x)] = i == 0 ? X[(size_t)(r + 6 * rows_x)] : (T)((3 * i + 5 * r + 2) % 128) / (T)128;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t j = 0; j < n; ++j) coef[(size_t)(j + c * n)] = (T)((5 * j + 11 * c) % 32 - 16) / (T)16;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t j = 0; j < k; ++j) alpha[(size_t)(j + c * k)] = (T)((3 * j + 7 * c) % 16 - 8) / (T)8;
    std::vector<int64_t> S((size_t)k);
    for (int64_t j = 0; j < k; ++j) S[(size_t)j] = 3 * j;      // Z(:, 0) = X(:, 6) is the centre S[2]
    const std::vector<T> nan((size_t)(ldg * mz * s), std::numeric_limits<T>::quiet_NaN());

    blas::Queue& q = blas::default_queue();
    dev_array<T> Xd(X), Zd(Z), Cd(coef), Ad(alpha);

    // 1. the operator's own entry, alpha = 1/2, Matern 5/2
    RL::linops::RBFCrossKernel<T> Kzx(rows_x, mz, Zd.p, n, Xd.p, l, q);
    Kzx.set_kernel(RL::PDKernel::Matern52);
    dev_array<T> G1(nan);
    Kzx.grad(s, (T)0.5, Cd.p, n, G1.p, ldg);
    report("grad", name, G1.host(ldg * mz * s), rows_x, mz, s, ldg);

    // 2. krr_predict_grad, squared exponential
    Kzx.set_kernel(RL::PDKernel::SquaredExp);
    dev_array<T> G2(nan);
    RL::krr_predict_grad(Kzx, s, Cd.p, n, G2.p, ldg);
    report("predict_grad", name, G2.host(ldg * mz * s), rows_x, mz, s, ldg);

    // 3. krr_predict_restricted_grad on k centres, Matern 3/2
    std::vector<T> regs{(T)0};
    RL::linops::RBFKernelMatrix<T> G(n, Xd.p, rows_x, l, regs, q);
    G.set_kernel(RL::PDKernel::Matern32);
    dev_array<T> G3(nan);
    RL::krr_predict_restricted_grad(G, k, S.data(), mz, Zd.p, rows_x, s, Ad.p, k, G3.p, ldg);
    report("restricted_grad", name, G3.host(ldg * mz * s), rows_x, mz, s, ldg);

    // 4. invalid calls raise: a leading dimension below rows_x, a centre that is no point
    int raised = 0;
    try { Kzx.grad(s, (T)1, Cd.p, n, G1.p, rows_x - 1); } catch (RL::Error const&) { ++raised; }
    S[1] = n;
    try { RL::krr_predict_restricted_grad(G, k, S.data(), mz, Zd.p, rows_x, s, Ad.p, k, G3.p, ldg); } catch (RL::Error const&) { ++raised; }
    if (raised != 2) {
        ++failures;
        std::printf("FAILED %s: %d of 2 invalid calls raised\n", name, raised);
    }
}

int main() {
    try {
        run<double>("double");
        run<float>("float");
    } catch (std::exception const& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("PASSED\n");
    return 0;
}
