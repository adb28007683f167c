// A user program for restricted kernel ridge regression written against RandLAPACK_amd.hh: fit with krill_restricted_rpchol over an
// RBFKernelMatrix (Matern 5/2), predict at new points with krr_predict_restricted, in double and float.  Every check is made here:
//   - with k = n the restricted coefficients are the full ones in pivot order: alpha(j, :) against X(S[j], :) of krill_full_rpchol on the same
//     problem, and the restricted prediction against krr_predict on the full coefficients.  Both fits solve (K + mu_i I) x = h_i, the full
//     one iteratively to 100 eps, so the allowance is 64 cond(K) eps relative to the largest coefficient, cond(K) <= (n + mu) / mu;
//   - with k < n the fit reproduces itself through krill_restricted on the same centres;
//   - three invalid calls throw.
// Built with the host compiler by `make -C tests/cxx -f krr_restricted.mk`; prints one line per precision and PASSED.
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

template <typename T>
void run(const char* name) {
    const int64_t n = 48, rows_x = 2, s = 2, mz = 70, b = 8;
    const T h = (T)0.1;
    const double eps = (double)std::numeric_limits<T>::epsilon();
    std::mt19937_64 gen(4321);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::normal_distribution<double> nd;
    std::vector<T> P((size_t)(rows_x * n)), Zh((size_t)(rows_x * mz)), Hh((size_t)(n * s));
    for (auto& x : P) x = (T)ud(gen);
    for (auto& x : Zh) x = (T)ud(gen);
    for (auto& x : Hh) x = (T)nd(gen);
    std::vector<T> mus{(T)1e-2, (T)1e-1};

    blas::Queue& q = blas::default_queue();
    dev_array<T> Pd(P), Zd(Zh), Hd(Hh), Xd(n * s), Ad(n * s), Yf(mz * s), Yr(mz * s);
    blas::device_memset(Xd.p, 0, n * s);
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, h, mus, q);
    G.set_kernel(RL::PDKernel::Matern52);

    // the full fit and its prediction
    RL::StatefulFrobeniusNorm<T> seminorm(q);
    auto state = RandBLAS::RNGState<RNG>(7);
    int64_t iters = 0, k_full = 0;
    RL::krill_full_rpchol(n, G, s, Hd.p, Xd.p, (T)(100 * eps), state, seminorm, b, (int64_t)200, (int64_t)24, false, &iters, &k_full);
    RL::linops::RBFCrossKernel<T> Kzx(rows_x, mz, Zd.p, n, Pd.p, h, q);
    Kzx.set_kernel(RL::PDKernel::Matern52);
    RL::krr_predict(Kzx, s, Xd.p, n, Yf.p, mz);
    std::vector<T> X = Xd.host(n * s), yf = Yf.host(mz * s);

    // the restricted fit with every point a centre, and its prediction
    std::vector<int64_t> S((size_t)n, -7);
    int64_t k = n;
    RL::KrillRestrictedInfo info;
    RL::krill_restricted_rpchol(n, G, s, Hd.p, n, k, S.data(), Ad.p, n, RandBLAS::RNGState<RNG>(7), b, &info);
    EXPECT(k == n && info.w_status <= 1 && info.c_status == 0, "%s: k=%lld w_status=%d c_status=%d", name, (long long)k, info.w_status, info.c_status);
    EXPECT(G._eval_includes_reg, "%s: the operator is left without its regularization", name);
    RL::krr_predict_restricted(G, k, S.data(), mz, Zd.p, rows_x, s, Ad.p, n, Yr.p, mz);
    std::vector<T> A = Ad.host(n * s), yr = Yr.host(mz * s);
    const double cond = ((double)n + (double)mus[0]) / (double)mus[0];
    double amax = 0, fit = 0, ymax = 0, pred = 0;
    for (auto v : X) amax = std::max(amax, std::fabs((double)v));
    for (int64_t c = 0; c < s; ++c)
        for (int64_t j = 0; j < k; ++j) fit = std::max(fit, std::fabs((double)A[(size_t)(j + c * n)] - (double)X[(size_t)(S[(size_t)j] + c * n)]));
    for (auto v : yf) ymax = std::max(ymax, std::fabs((double)v));
    for (size_t i = 0; i < yf.size(); ++i) pred = std::max(pred, std::fabs((double)yf[i] - (double)yr[i]));
    const double fit_ratio = fit / (64 * cond * eps * amax), pred_ratio = pred / (64 * cond * eps * std::max(ymax, amax));
    EXPECT(fit_ratio <= 1.0, "%s: restricted coefficients off the full ones by %.3g of the allowance", name, fit_ratio);
    EXPECT(pred_ratio <= 1.0, "%s: restricted prediction off the full one by %.3g of the allowance", name, pred_ratio);

    // k < n: the same centres handed to krill_restricted give the same coefficients (both run the same tail on the same factor up to rounding)
    int64_t k2 = 12;
    std::vector<int64_t> S2((size_t)k2, -7);
    dev_array<T> A1(k2 * s), A2(k2 * s);
    RL::krill_restricted_rpchol(n, G, s, Hd.p, n, k2, S2.data(), A1.p, k2, RandBLAS::RNGState<RNG>(9), b);
    EXPECT(k2 == 12, "%s: achieved rank %lld", name, (long long)k2);
    const int64_t rc = RL::krill_restricted(n, G, s, Hd.p, n, k2, S2.data(), A2.p, k2);
    EXPECT(rc == 0, "%s: krill_restricted returned %lld", name, (long long)rc);
    std::vector<T> a1 = A1.host(k2 * s), a2 = A2.host(k2 * s);
    double a1max = 0, same = 0;
    for (auto v : a1) a1max = std::max(a1max, std::fabs((double)v));
    for (size_t i = 0; i < a1.size(); ++i) same = std::max(same, std::fabs((double)a1[i] - (double)a2[i]));
    const double same_ratio = same / (64 * cond * eps * a1max);
    EXPECT(same_ratio <= 1.0, "%s: given centres differ from the pivoted fit by %.3g of the allowance", name, same_ratio);

    // invalid calls raise
    int raised = 0;
    int64_t kbad = n + 1;
    try { RL::krill_restricted_rpchol(n, G, s, Hd.p, n, kbad, S.data(), Ad.p, n + 1, RandBLAS::RNGState<RNG>(1), b); } catch (RL::Error const&) { ++raised; }
    try { RL::krill_restricted_rpchol(n, G, s + 1, Hd.p, n, k2, S2.data(), A1.p, k2, RandBLAS::RNGState<RNG>(1), b); } catch (RL::Error const&) { ++raised; }
    std::vector<int64_t> Sbad{0, n};
    try { RL::krr_predict_restricted(G, 2, Sbad.data(), mz, Zd.p, rows_x, s, Ad.p, n, Yr.p, mz); } catch (RL::Error const&) { ++raised; }
    EXPECT(raised == 3, "%s: %d of 3 invalid calls raised", name, raised);
    EXPECT(G._eval_includes_reg, "%s: the operator is left without its regularization after a refused call", name);

    std::printf("KRR restricted<%s> n=%lld k=%lld full iters=%lld fit=%.3g predict=%.3g given=%.3g\n", name, (long long)n, (long long)k, (long long)iters,
                fit_ratio, pred_ratio, same_ratio);
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
