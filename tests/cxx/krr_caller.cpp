// A user program for kernel ridge regression written against RandLAPACK_amd.hh: fit with krill_full_rpchol over an RBFKernelMatrix,
// predict at new points with krr_predict over an RBFCrossKernel, in double and float.  Every check is made here, against sums formed on the
// host in double:
//   - the coefficients meet the reference's own check of the solve (test/drivers/test_krill.cc:60-65);
//   - the prediction is within 64 eps (|K(Z, X)| |coeffs|) of K(Z, X) * coeffs, componentwise;
//   - Op::Trans of the cross kernel equals the operator constructed with the point sets swapped, bit for bit, and matvec equals operator()
//     with one column, bit for bit.
// Built with the host compiler by `make -C tests/cxx -f krr.mk`; prints one line per precision and PASSED.
#include "RandLAPACK_amd.hh"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

namespace RL = RandLAPACK;
using RNG = r123::Philox4x32;

template <typename T>
struct dev_array {
    T* p;
    explicit dev_array(int64_t n) : p(blas::device_malloc<T>(n)) {}
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
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            ++failures;                                    \
            std::printf("FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

// K(A, B)(i, j) in double from points already rounded to T
template <typename T>
std::vector<double> host_kernel(int64_t rows_x, std::vector<T> const& A, int64_t ma, std::vector<T> const& B, int64_t nb, double h) {
    std::vector<double> K((size_t)(ma * nb));
    for (int64_t j = 0; j < nb; ++j)
        for (int64_t i = 0; i < ma; ++i) {
            double d2 = 0;
            for (int64_t r = 0; r < rows_x; ++r) {
                const double d = (double)A[(size_t)(r + i * rows_x)] - (double)B[(size_t)(r + j * rows_x)];
                d2 += d * d;
            }
            K[(size_t)(i + j * ma)] = std::exp(-d2 / (2 * h * h));
        }
    return K;
}

template <typename T>
void run(const char* name) {
    const int64_t n = 600, rows_x = 4, s = 2, mz = 70, k = 96, b = 16;
    const T h = (T)2;
    const double eps = (double)std::numeric_limits<T>::epsilon();
    std::mt19937_64 gen(12345);
    std::normal_distribution<double> nd;
    auto draw = [&](int64_t cnt) {
        std::vector<T> v((size_t)cnt);
        for (auto& x : v) x = (T)nd(gen);
        return v;
    };
    std::vector<T> P = draw(rows_x * n), Zh = draw(rows_x * mz), Xstar = draw(n * s), Wh = draw(mz * s);
    std::vector<T> mus{(T)1e-2, (T)1e-1};

    // H = (K + mu_i I) Xstar on the host
    std::vector<double> K = host_kernel<T>(rows_x, P, n, P, n, (double)h);
    std::vector<T> Hh((size_t)(n * s));
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < n; ++i) {
            double acc = (double)mus[(size_t)c] * (double)Xstar[(size_t)(i + c * n)];
            for (int64_t j = 0; j < n; ++j) acc += K[(size_t)(i + j * n)] * (double)Xstar[(size_t)(j + c * n)];
            Hh[(size_t)(i + c * n)] = (T)acc;
        }

    blas::Queue& q = blas::default_queue();
    dev_array<T> Pd(P), Zd(Zh), Hd(Hh), Xd(n * s), Yd(mz * s), Wd(Wh);
    blas::device_memset(Xd.p, 0, n * s);

    // fit
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, h, mus, q);
    RL::StatefulFrobeniusNorm<T> seminorm(q);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t iters = 0, k_out = 0;
    RL::krill_full_rpchol(n, G, s, Hd.p, Xd.p, (T)(100 * eps), state, seminorm, b, (int64_t)40, k, false, &iters, &k_out);
    std::vector<T> X = Xd.host(n * s);
    const double atol = std::sqrt((double)n) * std::sqrt(eps), rtol = std::sqrt((double)n) * atol;
    double fit_ratio = 0;
    for (size_t i = 0; i < X.size(); ++i)
        fit_ratio = std::max(fit_ratio, std::fabs((double)X[i] - (double)Xstar[i]) / (atol + rtol * std::fabs((double)Xstar[i])));
    EXPECT(fit_ratio <= 1.0, "%s: coefficients off by %.3g of the allowance", name, fit_ratio);
    EXPECT(k_out == k && iters <= 40, "%s: k=%lld iters=%lld", name, (long long)k_out, (long long)iters);

    // predict
    RL::linops::RBFCrossKernel<T> Kzx(rows_x, mz, Zd.p, n, Pd.p, h, q);
    EXPECT(Kzx.n_rows == mz && Kzx.n_cols == n, "%s: operator shape", name);
    RL::krr_predict(Kzx, s, Xd.p, n, Yd.p, mz);
    std::vector<T> Y = Yd.host(mz * s);
    std::vector<double> Kz = host_kernel<T>(rows_x, Zh, mz, P, n, (double)h);
    double pred_ratio = 0;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < mz; ++i) {
            double want = 0, mag = 0;
            for (int64_t j = 0; j < n; ++j) {
                const double t = Kz[(size_t)(i + j * mz)] * (double)X[(size_t)(j + c * n)];
                want += t;
                mag += std::fabs(t);
            }
            pred_ratio = std::max(pred_ratio, std::fabs((double)Y[(size_t)(i + c * mz)] - want) / (64 * eps * mag));
        }
    EXPECT(pred_ratio <= 1.0, "%s: prediction off by %.3g of the bound", name, pred_ratio);

    // Op::Trans against the swapped construction, matvec against operator() with one column: the same bits
    dev_array<T> C1(n * s), C2(n * s), y1(n), y2(mz);
    Kzx(blas::Layout::ColMajor, blas::Op::Trans, s, (T)1, Wd.p, mz, (T)0, C1.p, n);
    RL::linops::RBFCrossKernel<T> Kxz(rows_x, n, Pd.p, mz, Zd.p, h, q);
    Kxz(blas::Layout::ColMajor, blas::Op::NoTrans, s, (T)1, Wd.p, mz, (T)0, C2.p, n);
    std::vector<T> c1 = C1.host(n * s), c2 = C2.host(n * s);
    EXPECT(std::memcmp(c1.data(), c2.data(), c1.size() * sizeof(T)) == 0, "%s: Op::Trans differs from the swapped operator", name);
    double tr_ratio = 0;      // and it is the transposed product
    for (int64_t c = 0; c < s; ++c)
        for (int64_t j = 0; j < n; ++j) {
            double want = 0, mag = 0;
            for (int64_t i = 0; i < mz; ++i) {
                const double t = Kz[(size_t)(i + j * mz)] * (double)Wh[(size_t)(i + c * mz)];
                want += t;
                mag += std::fabs(t);
            }
            tr_ratio = std::max(tr_ratio, std::fabs((double)c1[(size_t)(j + c * n)] - want) / (64 * eps * mag));
        }
    EXPECT(tr_ratio <= 1.0, "%s: transposed product off by %.3g of the bound", name, tr_ratio);
    Kzx.matvec(blas::Op::Trans, (T)1, Wd.p, (T)0, y1.p);
    std::vector<T> v1 = y1.host(n);
    EXPECT(std::memcmp(v1.data(), c1.data(), (size_t)n * sizeof(T)) == 0, "%s: matvec(Trans) differs from operator()", name);
    Kzx.matvec(blas::Op::NoTrans, (T)1, Xd.p, (T)0, y2.p);
    std::vector<T> v2 = y2.host(mz);
    EXPECT(std::memcmp(v2.data(), Y.data(), (size_t)mz * sizeof(T)) == 0, "%s: matvec(NoTrans) differs from krr_predict", name);

    // a block of the operator
    dev_array<T> Ks(20 * 30);
    Kzx.submatrix(20, 30, Ks.p, 5, 11);
    std::vector<T> ks = Ks.host(20 * 30);
    double sub_err = 0;
    for (int64_t j = 0; j < 30; ++j)
        for (int64_t i = 0; i < 20; ++i) sub_err = std::max(sub_err, std::fabs((double)ks[(size_t)(i + j * 20)] - Kz[(size_t)(5 + i + (11 + j) * mz)]));
    EXPECT(sub_err <= 64 * eps, "%s: submatrix off by %.3g", name, sub_err);

    // invalid calls raise
    int raised = 0;
    try { RL::linops::RBFCrossKernel<T> bad(rows_x, mz, Zd.p, n, Pd.p, (T)0, q); } catch (RL::Error const&) { ++raised; }
    try { Kzx(blas::Layout::RowMajor, blas::Op::NoTrans, s, (T)1, Xd.p, n, (T)0, Yd.p, mz); } catch (RL::Error const&) { ++raised; }
    try { Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, s, (T)1, Xd.p, n - 1, (T)0, Yd.p, mz); } catch (RL::Error const&) { ++raised; }
    EXPECT(raised == 3, "%s: %d of 3 invalid calls raised", name, raised);

    std::printf("KRR<%s> n=%lld k=%lld iters=%lld fit=%.3g predict=%.3g trans=%.3g submatrix=%.3g\n", name, (long long)n, (long long)k_out,
                (long long)iters, fit_ratio, pred_ratio, tr_ratio, sub_err);
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
