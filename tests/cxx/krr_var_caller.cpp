// A user program for the predictive variance of restricted kernel ridge regression, written against RandLAPACK_amd.hh: each of the four
// restricted fits with a KrillRestrictedBasis, then krr_predict_restricted_var at new points, in double and float.  Every check is made here:
//   - with a basis, S and alpha of each fit are bit for bit those of the same fit without one;
//   - the variance is finite, >= 0, exactly 1 at points 50 away from the data, and does not decrease when the regularization grows;
//   - the fit on given centres gives the variance of the pivoted fit on the same centres (both carry 8 cond(K_SS) eps with cond <= 1e3);
//   - after the _cv fits the variance is taken with path.best_mu;
//   - with every point a centre (k = n) the variance at training point i is mu (K (K + mu I)^-1)_ii = mu (1 - mu ((K + mu I)^-1)_ii), the
//     full Gaussian process, computed here in double by Gauss-Jordan, within 8 cond_1(K) eps;
//   - three invalid calls throw.
// Built with the host compiler by `make -C tests/cxx -f krr_var.mk`; prints one line per precision and PASSED.
#include "RandLAPACK_amd.hh"

#include <algorithm>
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

// A (n x n, column-major) <- A^-1 by Gauss-Jordan with partial pivoting; returns |A|_1 |A^-1|_1
static double invert(std::vector<double>& A, int64_t n) {
    auto norm1 = [&](std::vector<double> const& M) {
        double best = 0;
        for (int64_t j = 0; j < n; ++j) {
            double s = 0;
            for (int64_t i = 0; i < n; ++i) s += std::fabs(M[(size_t)(i + j * n)]);
            best = std::max(best, s);
        }
        return best;
    };
    const double na = norm1(A);
    std::vector<double> I((size_t)(n * n), 0.0);
    for (int64_t i = 0; i < n; ++i) I[(size_t)(i + i * n)] = 1.0;
    for (int64_t c = 0; c < n; ++c) {
        int64_t piv = c;
        for (int64_t i = c + 1; i < n; ++i)
            if (std::fabs(A[(size_t)(i + c * n)]) > std::fabs(A[(size_t)(piv + c * n)])) piv = i;
        for (int64_t j = 0; j < n; ++j) {
            std::swap(A[(size_t)(c + j * n)], A[(size_t)(piv + j * n)]);
            std::swap(I[(size_t)(c + j * n)], I[(size_t)(piv + j * n)]);
        }
        const double d = 1.0 / A[(size_t)(c + c * n)];
        for (int64_t j = 0; j < n; ++j) {
            A[(size_t)(c + j * n)] *= d;
            I[(size_t)(c + j * n)] *= d;
        }
        for (int64_t i = 0; i < n; ++i) {
            if (i == c) continue;
            const double f = A[(size_t)(i + c * n)];
            if (f == 0.0) continue;
            for (int64_t j = 0; j < n; ++j) {
                A[(size_t)(i + j * n)] -= f * A[(size_t)(c + j * n)];
                I[(size_t)(i + j * n)] -= f * I[(size_t)(c + j * n)];
            }
        }
    }
    A = I;
    return na * norm1(A);
}

// Matern 3/2 by differences, in double
static double matern32(const double* x, const double* y, int64_t rows, double l) {
    double s = 0;
    for (int64_t r = 0; r < rows; ++r) s += (x[r] - y[r]) * (x[r] - y[r]);
    const double a = std::sqrt(3.0 * s) / l;
    return (1.0 + a) * std::exp(-a);
}

template <typename T>
void check_variance(const char* name, const char* what, std::vector<T> const& v, int64_t mz, int64_t s, int64_t far) {
    int bad = 0, not_one = 0;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < mz; ++i) {
            const double x = (double)v[(size_t)(i + c * mz)];
            bad += !(std::isfinite(x) && x >= 0.0 && x <= 1.0 + 64 * (double)std::numeric_limits<T>::epsilon());
            if (i >= mz - far) not_one += x != 1.0;
        }
    EXPECT(bad == 0 && not_one == 0, "%s %s: %d values outside [0, 1], %d far points not exactly 1", name, what, bad, not_one);
}

template <typename T>
void run(const char* name) {
    const int64_t n = 300, rows_x = 2, s = 2, mz = 90, far = 5, b = 8, g = 6, k_in = 40;
    const double eps = (double)std::numeric_limits<T>::epsilon();
    const T h = (T)0.2;
    std::mt19937_64 gen(41);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::normal_distribution<double> nd;
    std::vector<T> P((size_t)(rows_x * n)), Zh((size_t)(rows_x * mz)), Hh((size_t)(n * s));
    for (auto& x : P) x = (T)ud(gen);
    for (auto& x : Zh) x = (T)ud(gen);
    for (int64_t i = mz - far; i < mz; ++i)
        for (int64_t r = 0; r < rows_x; ++r) Zh[(size_t)(r + i * rows_x)] += (T)50;
    for (auto& x : Hh) x = (T)nd(gen);
    std::vector<T> grid((size_t)g);
    for (int64_t m = 0; m < g; ++m) grid[(size_t)m] = (T)std::pow(10.0, (double)(m - 5));

    blas::Queue& q = blas::default_queue();
    dev_array<T> Pd(P), Zd(Zh), Hd(Hh);
    std::vector<T> regs{(T)1e-3, (T)1e-1};
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, h, regs, q);
    G.set_kernel(RL::PDKernel::Matern52);

    // 1. the pivoted fit, with and without a basis
    int64_t k = k_in, k0 = k_in;
    std::vector<int64_t> S((size_t)k_in, -7), S0((size_t)k_in, -7);
    dev_array<T> Ad(k_in * s), A0(k_in * s), Gb(k_in * k_in), sg(k_in), Vd(mz * s), Vd2(mz * s);
    RL::KrillRestrictedBasis<T> basis{Gb.p, k_in, sg.p};
    RL::krill_restricted_rpchol(n, G, s, Hd.p, n, k0, S0.data(), A0.p, k_in, RandBLAS::RNGState<RNG>(7), b);
    RL::krill_restricted_rpchol(n, G, s, Hd.p, n, k, S.data(), Ad.p, k_in, RandBLAS::RNGState<RNG>(7), b, (RL::KrillRestrictedInfo*)nullptr, &basis);
    EXPECT(k == k_in && k0 == k_in, "%s: k=%lld", name, (long long)k);
    std::vector<T> a = Ad.host(k_in * s), a0 = A0.host(k_in * s);
    EXPECT(S == S0 && std::memcmp(a.data(), a0.data(), a.size() * sizeof(T)) == 0, "%s: the fit with a basis differs from the fit without", name);
    RL::krr_predict_restricted_var(G, k, S.data(), basis, mz, Zd.p, rows_x, s, regs.data(), s, Vd.p, mz);
    std::vector<T> v = Vd.host(mz * s);
    check_variance(name, "pivoted fit", v, mz, s, far);
    int decreasing = 0;
    for (int64_t i = 0; i < mz; ++i) decreasing += (double)v[(size_t)(i + mz)] < (double)v[(size_t)i] - 64 * eps;      // regs ascend
    EXPECT(decreasing == 0, "%s: the variance decreases with the regularization at %d points", name, decreasing);
    // the fused kernel on request: the same values in another order of summation (each carries 8 cond(K_SS) eps, cond <= 1e3)
    RL::krr_predict_restricted_var(G, k, S.data(), basis, mz, Zd.p, rows_x, s, regs.data(), s, Vd2.p, mz, true);
    std::vector<T> vf = Vd2.host(mz * s);
    check_variance(name, "fused kernel", vf, mz, s, far);
    double gapf = 0;
    for (size_t i = 0; i < v.size(); ++i) gapf = std::max(gapf, std::fabs((double)v[i] - (double)vf[i]));
    EXPECT(gapf <= 2 * 8 * 1e3 * eps && rlhip_pdk_var_set_fused(q.ctx(), 0) == 0, "%s: the fused kernel differs by %g, or its request outlived the call", name, gapf);

    // 2. the same centres given
    dev_array<T> A2(k * s), A2p(k * s), Gb2(k * k), sg2(k);
    RL::KrillRestrictedBasis<T> basis2{Gb2.p, k, sg2.p};
    const int64_t rc2p = RL::krill_restricted(n, G, s, Hd.p, n, k, S.data(), A2p.p, k);
    const int64_t rc2 = RL::krill_restricted(n, G, s, Hd.p, n, k, S.data(), A2.p, k, &basis2);
    std::vector<T> a2 = A2.host(k * s), a2p = A2p.host(k * s);
    EXPECT(rc2 == 0 && rc2p == 0 && std::memcmp(a2.data(), a2p.data(), a2.size() * sizeof(T)) == 0, "%s: krill_restricted with a basis differs", name);
    RL::krr_predict_restricted_var(G, k, S.data(), basis2, mz, Zd.p, rows_x, s, regs.data(), s, Vd2.p, mz);
    std::vector<T> v2 = Vd2.host(mz * s);
    check_variance(name, "given centres", v2, mz, s, far);
    double gap = 0;
    for (size_t i = 0; i < v.size(); ++i) gap = std::max(gap, std::fabs((double)v[i] - (double)v2[i]));
    EXPECT(gap <= 2 * 8 * 1e3 * eps, "%s: the two fits' variances differ by %g", name, gap);

    // 3. the regularization chosen from a grid: the variance with path.best_mu
    int64_t k3 = k_in, k3p = k_in;
    std::vector<int64_t> S3((size_t)k_in, -7), S3p((size_t)k_in, -7);
    dev_array<T> A3(k_in * s), A3p(k_in * s), Gb3(k_in * (k_in + 2)), sg3(k_in), Vd3(mz * s);
    RL::KrillRestrictedBasis<T> basis3{Gb3.p, k_in + 2, sg3.p};
    RL::KrillRidgePath path, pathp;
    RL::krill_restricted_rpchol_cv(n, G, s, Hd.p, n, g, grid.data(), RL::KrillCriterion::LeaveOneOut, k3p, S3p.data(), A3p.p, k_in, pathp,
                                   RandBLAS::RNGState<RNG>(7), b);
    RL::krill_restricted_rpchol_cv(n, G, s, Hd.p, n, g, grid.data(), RL::KrillCriterion::LeaveOneOut, k3, S3.data(), A3.p, k_in, path,
                                   RandBLAS::RNGState<RNG>(7), b, (RL::KrillRestrictedInfo*)nullptr, &basis3);
    std::vector<T> a3 = A3.host(k_in * s), a3p = A3p.host(k_in * s);
    EXPECT(k3 == k_in && S3 == S3p && path.best == pathp.best && std::memcmp(a3.data(), a3p.data(), a3.size() * sizeof(T)) == 0,
           "%s: krill_restricted_rpchol_cv with a basis differs", name);
    std::vector<T> chosen(path.best_mu.begin(), path.best_mu.end());
    RL::krr_predict_restricted_var(G, k3, S3.data(), basis3, mz, Zd.p, rows_x, s, chosen.data(), s, Vd3.p, mz);
    std::vector<T> v3 = Vd3.host(mz * s);
    check_variance(name, "cv fit", v3, mz, s, far);

    // 4. the centres given, generalized cross-validation
    dev_array<T> A4(k * s), Gb4(k * k), sg4(k), Vd4(mz * s);
    RL::KrillRestrictedBasis<T> basis4{Gb4.p, k, sg4.p};
    RL::KrillRidgePath path4;
    const int64_t rc4 = RL::krill_restricted_cv(n, G, s, Hd.p, n, g, grid.data(), RL::KrillCriterion::GCV, k, S.data(), A4.p, k, path4, &basis4);
    EXPECT(rc4 == 0 && (int64_t)path4.best_mu.size() == s, "%s: krill_restricted_cv returned %lld", name, (long long)rc4);
    std::vector<T> chosen4(path4.best_mu.begin(), path4.best_mu.end());
    RL::krr_predict_restricted_var(G, k, S.data(), basis4, mz, Zd.p, rows_x, s, chosen4.data(), s, Vd4.p, mz);
    std::vector<T> v4 = Vd4.host(mz * s);
    check_variance(name, "cv fit on given centres", v4, mz, s, far);
    // one basis serves every regularization: the pivoted fit's basis with the values chosen here gives what basis4 gives, to the bound of 2.
    RL::krr_predict_restricted_var(G, k, S.data(), basis, mz, Zd.p, rows_x, s, chosen4.data(), s, Vd2.p, mz);
    std::vector<T> v4b = Vd2.host(mz * s);
    double gap4 = 0;
    for (size_t i = 0; i < v4.size(); ++i) gap4 = std::max(gap4, std::fabs((double)v4[i] - (double)v4b[i]));
    EXPECT(gap4 <= 2 * 8 * 1e3 * eps, "%s: the variance from two bases of the same centres differs by %g", name, gap4);

    // 5. k = n: the full Gaussian process at the training points
    const int64_t n5 = 48;
    const double l5 = 0.12, mu5 = 1e-2;
    std::vector<T> P5(P.begin(), P.begin() + rows_x * n5);
    dev_array<T> P5d(P5), H5d(std::vector<T>(Hh.begin(), Hh.begin() + n5)), A5(n5), Gb5(n5 * n5), sg5(n5), V5(n5);
    std::vector<T> regs5{(T)mu5};
    RL::linops::RBFKernelMatrix<T> G5(n5, P5d.p, rows_x, (T)l5, regs5, q);
    G5.set_kernel(RL::PDKernel::Matern32);
    int64_t k5 = n5;
    std::vector<int64_t> S5((size_t)n5, -7);
    RL::KrillRestrictedBasis<T> basis5{Gb5.p, n5, sg5.p};
    RL::krill_restricted_rpchol(n5, G5, 1, H5d.p, n5, k5, S5.data(), A5.p, n5, RandBLAS::RNGState<RNG>(3), b, (RL::KrillRestrictedInfo*)nullptr, &basis5);
    EXPECT(k5 == n5, "%s: k = n fit stopped at %lld", name, (long long)k5);
    double err5 = 0, bound5 = 0;
    if (k5 == n5) {
        RL::krr_predict_restricted_var(G5, k5, S5.data(), basis5, n5, P5d.p, rows_x, 1, regs5.data(), 1, V5.p, n5);
        std::vector<T> v5 = V5.host(n5);
        std::vector<double> Pd5(P5.begin(), P5.end()), K((size_t)(n5 * n5)), A((size_t)(n5 * n5));
        const double l5t = (double)(T)l5, mu5t = (double)(T)mu5;
        for (int64_t j = 0; j < n5; ++j)
            for (int64_t i = 0; i < n5; ++i) {
                K[(size_t)(i + j * n5)] = matern32(&Pd5[(size_t)(rows_x * i)], &Pd5[(size_t)(rows_x * j)], rows_x, l5t);
                A[(size_t)(i + j * n5)] = K[(size_t)(i + j * n5)] + (i == j ? mu5t : 0.0);
            }
        const double cond = invert(K, n5);
        invert(A, n5);
        bound5 = 8 * cond * eps;
        for (int64_t i = 0; i < n5; ++i) err5 = std::max(err5, std::fabs((double)v5[(size_t)i] - mu5t * (1.0 - mu5t * A[(size_t)(i + i * n5)])));
        EXPECT(err5 <= bound5, "%s: k = n: the variance is %g away from the full Gaussian process (bound %g, cond_1(K) %g)", name, err5, bound5, cond);
    }

    // 6. invalid calls raise
    int raised = 0;
    std::vector<T> neg{(T)1e-2, (T)-1e-2}, three{(T)1e-3, (T)1e-2, (T)1e-1};
    RL::KrillRestrictedBasis<T> narrow{Gb.p, k_in - 1, sg.p};
    int64_t kk = k_in;
    try { RL::krr_predict_restricted_var(G, k, S.data(), basis, mz, Zd.p, rows_x, s, neg.data(), s, Vd.p, mz); } catch (RL::Error const&) { ++raised; }
    try { RL::krr_predict_restricted_var(G, k, S.data(), basis, mz, Zd.p, rows_x, s, three.data(), (int64_t)3, Vd.p, mz); } catch (RL::Error const&) { ++raised; }
    try { RL::krill_restricted_rpchol(n, G, s, Hd.p, n, kk, S0.data(), A0.p, k_in, RandBLAS::RNGState<RNG>(7), b, (RL::KrillRestrictedInfo*)nullptr, &narrow); } catch (RL::Error const&) { ++raised; }
    EXPECT(raised == 3, "%s: %d of 3 invalid calls raised", name, raised);
    EXPECT(G._eval_includes_reg, "%s: the operator is left without its regularization after a refused call", name);

    double vmin = 1, vmax = 0;
    for (int64_t i = 0; i < mz - far; ++i) {
        vmin = std::min(vmin, (double)v[(size_t)i]);
        vmax = std::max(vmax, (double)v[(size_t)i]);
    }
    std::printf("KRR var<%s> n=%lld k=%lld var(mu=%g) in [%.3g, %.3g] fits agree to %.3g / %.3g, k = n error %.3g (bound %.3g)\n", name, (long long)n,
                (long long)k, (double)regs[0], vmin, vmax, gap, gap4, err5, bound5);
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
