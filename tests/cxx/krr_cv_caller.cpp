// A user program for restricted kernel ridge regression with the regularization chosen from a grid, written against RandLAPACK_amd.hh:
// krill_restricted_rpchol_cv over an RBFKernelMatrix (Matern 5/2) on noisy samples of a smooth function, then krr_predict_restricted at new
// points, in double and float.  Every check is made here:
//   - the path has the stated shapes, every entry is finite, rss <= loo entry by entry (a leave-one-out residual is the residual divided by
//     1 - s_i in (0, 1]) and dof decreases as the grid value grows;
//   - best is the lowest index of the smallest leave-one-out sum of each column, and alpha is bit for bit what krill_restricted_rpchol
//     returns with G.regs = best_mu on the same state;
//   - the prediction of the chosen model is closer to the noise-free function than that of the worst grid value;
//   - krill_restricted_cv on the same centres (generalized cross-validation) agrees with krill_restricted at its own choice;
//   - three invalid calls throw.
// Built with the host compiler by `make -C tests/cxx -f krr_cv.mk`; prints one line per precision and PASSED.
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

static double truth(double x0, double x1, int64_t c) { return std::sin(2 * M_PI * (double)(c + 1) * x0) * std::cos(M_PI * x1); }

template <typename T>
void run(const char* name) {
    const int64_t n = 400, rows_x = 2, s = 2, mz = 90, b = 8, g = 8;
    const T h = (T)0.25;
    std::mt19937_64 gen(97);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    std::normal_distribution<double> nd;
    std::vector<T> P((size_t)(rows_x * n)), Zh((size_t)(rows_x * mz)), Hh((size_t)(n * s));
    for (auto& x : P) x = (T)ud(gen);
    for (auto& x : Zh) x = (T)ud(gen);
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < n; ++i) Hh[(size_t)(i + c * n)] = (T)(truth((double)P[(size_t)(2 * i)], (double)P[(size_t)(2 * i + 1)], c) + 0.3 * nd(gen));
    std::vector<T> grid((size_t)g);
    for (int64_t m = 0; m < g; ++m) grid[(size_t)m] = (T)std::pow(10.0, (double)(m - 6));

    blas::Queue& q = blas::default_queue();
    dev_array<T> Pd(P), Zd(Zh), Hd(Hh);
    std::vector<T> regs{(T)123};                        // not read by the _cv fits
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, h, regs, q);
    G.set_kernel(RL::PDKernel::Matern52);

    // fit with selection
    int64_t k = 32;
    std::vector<int64_t> S((size_t)k, -7);
    dev_array<T> Ad(k * s);
    RL::KrillRidgePath path;
    RL::KrillRestrictedInfo info;
    RL::krill_restricted_rpchol_cv(n, G, s, Hd.p, n, g, grid.data(), RL::KrillCriterion::LeaveOneOut, k, S.data(), Ad.p, k, path, RandBLAS::RNGState<RNG>(7), b,
                                   &info);
    EXPECT(k == 32 && info.c_status == 0, "%s: k=%lld c_status=%d", name, (long long)k, info.c_status);
    EXPECT(G._eval_includes_reg, "%s: the operator is left without its regularization", name);
    EXPECT(path.g == g && path.ell == s && (int64_t)path.loo.size() == g * s && (int64_t)path.rss.size() == g * s && (int64_t)path.dof.size() == g &&
               (int64_t)path.best.size() == s && (int64_t)path.best_mu.size() == s, "%s: the path's shapes", name);
    int interior = 0;
    for (int64_t c = 0; c < s; ++c) {
        int64_t arg = 0;
        for (int64_t m = 0; m < g; ++m) {
            const double lo = path.loo[(size_t)(m + c * g)], rs = path.rss[(size_t)(m + c * g)];
            EXPECT(std::isfinite(lo) && std::isfinite(rs) && rs > 0 && rs <= lo, "%s: loo=%g rss=%g at (%lld, %lld)", name, lo, rs, (long long)m, (long long)c);
            if (lo < path.loo[(size_t)(arg + c * g)]) arg = m;
        }
        EXPECT(path.best[(size_t)c] == arg && path.best_mu[(size_t)c] == (double)grid[(size_t)arg], "%s: column %lld chose %lld, the smallest is %lld", name,
               (long long)c, (long long)path.best[(size_t)c], (long long)arg);
        interior += arg > 0 && arg < g - 1;
    }
    EXPECT(interior >= 1, "%s: no column has its minimum inside the grid", name);
    for (int64_t m = 1; m < g; ++m) EXPECT(path.dof[(size_t)m] < path.dof[(size_t)(m - 1)] && path.dof[(size_t)m] > 0, "%s: dof[%lld]", name, (long long)m);
    EXPECT(path.dof[0] <= (double)k, "%s: dof[0]=%g", name, path.dof[0]);

    // the existing fit with the chosen values: bit for bit
    std::vector<T> chosen{(T)path.best_mu[0], (T)path.best_mu[1]};
    RL::linops::RBFKernelMatrix<T> G2(n, Pd.p, rows_x, h, chosen, q);
    G2.set_kernel(RL::PDKernel::Matern52);
    int64_t k2 = 32;
    std::vector<int64_t> S2((size_t)k2, -7);
    dev_array<T> A2(k2 * s);
    RL::krill_restricted_rpchol(n, G2, s, Hd.p, n, k2, S2.data(), A2.p, k2, RandBLAS::RNGState<RNG>(7), b);
    std::vector<T> a1 = Ad.host(k * s), a2 = A2.host(k2 * s);
    EXPECT(S == S2 && std::memcmp(a1.data(), a2.data(), a1.size() * sizeof(T)) == 0, "%s: the fit differs from krill_restricted_rpchol with the chosen values", name);

    // prediction: the chosen model against the worst grid value, measured on the noise-free function
    dev_array<T> Yd(mz * s), Yw(mz * s), Aw(k * s);
    RL::krr_predict_restricted(G, k, S.data(), mz, Zd.p, rows_x, s, Ad.p, k, Yd.p, mz);
    int64_t worst[2] = {0, 0};
    for (int64_t c = 0; c < s; ++c)
        for (int64_t m = 0; m < g; ++m)
            if (path.loo[(size_t)(m + c * g)] > path.loo[(size_t)(worst[c] + c * g)]) worst[c] = m;
    std::vector<T> bad{grid[(size_t)worst[0]], grid[(size_t)worst[1]]};
    RL::linops::RBFKernelMatrix<T> G3(n, Pd.p, rows_x, h, bad, q);
    G3.set_kernel(RL::PDKernel::Matern52);
    const int64_t rc3 = RL::krill_restricted(n, G3, s, Hd.p, n, k, S.data(), Aw.p, k);
    EXPECT(rc3 == 0, "%s: krill_restricted returned %lld", name, (long long)rc3);
    RL::krr_predict_restricted(G3, k, S.data(), mz, Zd.p, rows_x, s, Aw.p, k, Yw.p, mz);
    std::vector<T> yd = Yd.host(mz * s), yw = Yw.host(mz * s);
    double err_best = 0, err_worst = 0;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < mz; ++i) {
            const double t = truth((double)Zh[(size_t)(2 * i)], (double)Zh[(size_t)(2 * i + 1)], c);
            err_best += std::pow((double)yd[(size_t)(i + c * mz)] - t, 2);
            err_worst += std::pow((double)yw[(size_t)(i + c * mz)] - t, 2);
        }
    EXPECT(err_best < err_worst, "%s: the chosen model predicts worse (%g) than the worst grid value (%g)", name, err_best, err_worst);

    // the centres given, generalized cross-validation
    dev_array<T> A4(k * s), A5(k * s);
    RL::KrillRidgePath path4;
    const int64_t rc4 = RL::krill_restricted_cv(n, G, s, Hd.p, n, g, grid.data(), RL::KrillCriterion::GCV, k, S.data(), A4.p, k, path4);
    EXPECT(rc4 == 0 && (int64_t)path4.best.size() == s, "%s: krill_restricted_cv returned %lld", name, (long long)rc4);
    for (int64_t c = 0; c < s && rc4 == 0; ++c) {
        int64_t arg = 0;
        double best = 0;
        for (int64_t m = 0; m < g; ++m) {
            const double left = (double)n - path4.dof[(size_t)m], v = (double)n * path4.rss[(size_t)(m + c * g)] / (left * left);
            if (m == 0 || v < best) { best = v; arg = m; }
        }
        EXPECT(path4.best[(size_t)c] == arg, "%s: GCV column %lld chose %lld, the smallest is %lld", name, (long long)c, (long long)path4.best[(size_t)c], (long long)arg);
    }
    std::vector<T> chosen4{(T)path4.best_mu[0], (T)path4.best_mu[1]};
    RL::linops::RBFKernelMatrix<T> G5(n, Pd.p, rows_x, h, chosen4, q);
    G5.set_kernel(RL::PDKernel::Matern52);
    const int64_t rc5 = RL::krill_restricted(n, G5, s, Hd.p, n, k, S.data(), A5.p, k);
    std::vector<T> a4 = A4.host(k * s), a5 = A5.host(k * s);
    EXPECT(rc5 == 0 && std::memcmp(a4.data(), a5.data(), a4.size() * sizeof(T)) == 0, "%s: krill_restricted_cv differs from krill_restricted with its choice", name);

    // invalid calls raise
    int raised = 0;
    std::vector<T> neg{(T)1e-2, (T)-1e-2};
    int64_t kk = 32;
    try { RL::krill_restricted_rpchol_cv(n, G, s, Hd.p, n, (int64_t)0, grid.data(), RL::KrillCriterion::LeaveOneOut, kk, S.data(), Ad.p, k, path, RandBLAS::RNGState<RNG>(1), b); } catch (RL::Error const&) { ++raised; }
    try { RL::krill_restricted_rpchol_cv(n, G, s, Hd.p, n, (int64_t)2, neg.data(), RL::KrillCriterion::LeaveOneOut, kk, S.data(), Ad.p, k, path, RandBLAS::RNGState<RNG>(1), b); } catch (RL::Error const&) { ++raised; }
    try { RL::krill_restricted_cv(n, G, s, Hd.p, n, g, (const T*)nullptr, RL::KrillCriterion::GCV, k, S.data(), A4.p, k, path4); } catch (RL::Error const&) { ++raised; }
    EXPECT(raised == 3, "%s: %d of 3 invalid calls raised", name, raised);
    EXPECT(G._eval_includes_reg, "%s: the operator is left without its regularization after a refused call", name);

    std::printf("KRR cv<%s> n=%lld k=%lld best=(%lld, %lld) gcv=(%lld, %lld) dof=%.3g..%.3g err chosen=%.3g worst=%.3g\n", name, (long long)n, (long long)k,
                (long long)path.best[0], (long long)path.best[1], (long long)path4.best[0], (long long)path4.best[1], path.dof[0], path.dof[(size_t)(g - 1)],
                err_best, err_worst);
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
