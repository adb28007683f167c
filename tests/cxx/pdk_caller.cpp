// A user program for kernel ridge regression with a Matern 5/2 kernel, written against RandLAPACK_amd.hh: set_kernel(PDKernel::Matern52) on an
// RBFKernelMatrix, fit with krill_full_rpchol, predict with krr_predict over an RBFCrossKernel with the same kernel, in double and float.
// Nothing else changes against a squared-exponential program: rp_cholesky, the preconditioner, PCG and the prediction reach the kernel through
// the two objects only.  The checks, against sums formed on the host in double:
//   - the residual H - (K + mu I) X of the fit.  PCG stops when |N R|_F < tol (1 + |N R_0|_F); the spectral preconditioner N has its
//     eigenvalues in [(lambda_k + mu) / (lambda_1 + mu), 1] and R_0 = H, so |R|_F < tol (1 + |H|_F) (lambda_1 + mu) / (lambda_k + mu)
//     <= tol (1 + |H|_F) (n + mu) / mu, as lambda_1 <= trace K = n: that is what is asserted, here and by tests/test_gpu_pdk_cxx.py;
//   - the prediction is within 64 eps (|K(Z, X)| |coeffs|) of K(Z, X) * coeffs, componentwise;
//   - a block of the cross operator against the host kernel, and the default kernel of a fresh object is the squared exponential.
// Built with the host compiler by `make -C tests/cxx -f pdk.mk`; prints one line per precision and PASSED.
#include "RandLAPACK_amd.hh"

#include <cmath>
#include <cstdio>
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

// Matern 5/2 K(A, B)(i, j) in double, by differences, from points already rounded to T
template <typename T>
std::vector<double> host_matern52(int64_t rows_x, std::vector<T> const& A, int64_t ma, std::vector<T> const& B, int64_t nb, double l) {
    std::vector<double> K((size_t)(ma * nb));
    for (int64_t j = 0; j < nb; ++j)
        for (int64_t i = 0; i < ma; ++i) {
            double d2 = 0;
            for (int64_t r = 0; r < rows_x; ++r) {
                const double d = (double)A[(size_t)(r + i * rows_x)] - (double)B[(size_t)(r + j * rows_x)];
                d2 += d * d;
            }
            const double a = std::sqrt(5.0) * std::sqrt(d2) / l;
            K[(size_t)(i + j * ma)] = (1.0 + a + a * a / 3.0) * std::exp(-a);
        }
    return K;
}

template <typename T>
void run(const char* name) {
    const int64_t n = 600, rows_x = 4, s = 2, mz = 70, k = 96, b = 16, max_iters = 60;
    const T l = (T)2;
    const double mu = 0.1;
    const double eps = (double)std::numeric_limits<T>::epsilon();
    const double tol = 100 * eps;
    std::mt19937_64 gen(4321);
    std::normal_distribution<double> nd;
    auto draw = [&](int64_t cnt) {
        std::vector<T> v((size_t)cnt);
        for (auto& x : v) x = (T)nd(gen);
        return v;
    };
    std::vector<T> P = draw(rows_x * n), Zh = draw(rows_x * mz), Xstar = draw(n * s);
    std::vector<T> mus{(T)mu};

    // H = (K + mu I) Xstar on the host
    std::vector<double> K = host_matern52<T>(rows_x, P, n, P, n, (double)l);
    std::vector<T> Hh((size_t)(n * s));
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < n; ++i) {
            double acc = (double)mus[0] * (double)Xstar[(size_t)(i + c * n)];
            for (int64_t j = 0; j < n; ++j) acc += K[(size_t)(i + j * n)] * (double)Xstar[(size_t)(j + c * n)];
            Hh[(size_t)(i + c * n)] = (T)acc;
        }

    blas::Queue& q = blas::default_queue();
    dev_array<T> Pd(P), Zd(Zh), Hd(Hh), Xd(n * s), Yd(mz * s);
    blas::device_memset(Xd.p, 0, n * s);

    // fit
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, l, mus, q);
    EXPECT(G.kernel == RL::PDKernel::SquaredExp, "%s: the default kernel", name);
    G.set_kernel(RL::PDKernel::Matern52);
    RL::StatefulFrobeniusNorm<T> seminorm(q);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t iters = 0, k_out = 0;
    RL::krill_full_rpchol(n, G, s, Hd.p, Xd.p, (T)tol, state, seminorm, b, max_iters, k, false, &iters, &k_out);
    std::vector<T> X = Xd.host(n * s);
    double res2 = 0, h2 = 0;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < n; ++i) {
            double acc = (double)Hh[(size_t)(i + c * n)] - (double)mus[0] * (double)X[(size_t)(i + c * n)];
            for (int64_t j = 0; j < n; ++j) acc -= K[(size_t)(i + j * n)] * (double)X[(size_t)(j + c * n)];
            res2 += acc * acc;
            h2 += (double)Hh[(size_t)(i + c * n)] * (double)Hh[(size_t)(i + c * n)];
        }
    const double resid = std::sqrt(res2), normH = std::sqrt(h2);
    const double allowed = tol * (1 + normH) * ((double)n + (double)mus[0]) / (double)mus[0];
    EXPECT(resid <= allowed, "%s: residual %.3g exceeds %.3g", name, resid, allowed);
    EXPECT(k_out == k && iters >= 1 && iters < max_iters, "%s: k=%lld iters=%lld", name, (long long)k_out, (long long)iters);

    // predict
    RL::linops::RBFCrossKernel<T> Kzx(rows_x, mz, Zd.p, n, Pd.p, l, q);
    EXPECT(Kzx.kernel == RL::PDKernel::SquaredExp, "%s: the default kernel of the cross operator", name);
    Kzx.set_kernel(RL::PDKernel::Matern52);
    RL::krr_predict(Kzx, s, Xd.p, n, Yd.p, mz);
    std::vector<T> Y = Yd.host(mz * s);
    std::vector<double> Kz = host_matern52<T>(rows_x, Zh, mz, P, n, (double)l);
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

    // a block of the operator: entries within 16 eps (1 + L (|z|^2 + |x|^2)), L = 5 / (6 l^2)
    dev_array<T> Ks(20 * 30);
    Kzx.submatrix(20, 30, Ks.p, 5, 11);
    std::vector<T> ks = Ks.host(20 * 30);
    auto norm2 = [&](std::vector<T> const& A, int64_t i) {
        double v = 0;
        for (int64_t r = 0; r < rows_x; ++r) v += (double)A[(size_t)(r + i * rows_x)] * (double)A[(size_t)(r + i * rows_x)];
        return v;
    };
    double sub_ratio = 0;
    for (int64_t j = 0; j < 30; ++j)
        for (int64_t i = 0; i < 20; ++i) {
            const double scale = 1 + 5.0 / (6.0 * (double)l * (double)l) * (norm2(Zh, 5 + i) + norm2(P, 11 + j));
            sub_ratio = std::max(sub_ratio, std::fabs((double)ks[(size_t)(i + j * 20)] - Kz[(size_t)(5 + i + (11 + j) * mz)]) / (16 * eps * scale));
        }
    EXPECT(sub_ratio <= 1.0, "%s: submatrix off by %.3g of the bound", name, sub_ratio);

    std::printf("PDK<%s> kernel=matern52 n=%lld k=%lld iters=%lld max_iters=%lld tol=%.6g mu=%.6g normH=%.9g resid=%.6g predict=%.3g submatrix=%.3g\n",
                name, (long long)n, (long long)k_out, (long long)iters, (long long)max_iters, tol, (double)mus[0], normH, resid, pred_ratio, sub_ratio);
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
