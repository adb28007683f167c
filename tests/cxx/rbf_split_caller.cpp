// A user program for the fused cross apply split over X, written against RandLAPACK_amd.hh: set_split_x(true) on an
// RBFCrossKernel (prediction at 70 points against 1100 training points) and on a matrix-free RBFKernelMatrix over the same 1100 points, in
// double and float.  Every check is made here:
//   - each product is within 64 eps (|K| |B|) of the sum formed on the host in double, componentwise;
//   - the split counter of the context moves by one per product with set_split_x(true) and not at all without it;
//   - RLHIP_OPT_RBF_FUSED is what it was before each call, whether that was the default or a value the caller had set;
//   - set_split_x without set_matrix_free has no effect on RBFKernelMatrix;
//   - krr_predict_restricted hands the operator's choice on to the cross kernel it builds.
// Built with the host compiler by `make -C tests/cxx -f rbf_split.mk`; prints one line per precision and PASSED.
#include "RandLAPACK_amd.hh"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

namespace RL = RandLAPACK;

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

// max over the entries of |got - K(A, P(:, cols)) W| / (64 eps |K| |W|), K in double from points already rounded to T; cols == nullptr: all of P
template <typename T>
double product_ratio(int64_t rows_x, std::vector<T> const& A, int64_t ma, std::vector<T> const& P, int64_t np, const int64_t* cols, double h,
                     std::vector<T> const& W, int64_t s, std::vector<T> const& got) {
    const double eps = (double)std::numeric_limits<T>::epsilon();
    double ratio = 0;
    for (int64_t c = 0; c < s; ++c)
        for (int64_t i = 0; i < ma; ++i) {
            double want = 0, mag = 0;
            for (int64_t j = 0; j < np; ++j) {
                const int64_t pj = cols ? cols[j] : j;
                double d2 = 0;
                for (int64_t r = 0; r < rows_x; ++r) {
                    const double d = (double)A[(size_t)(r + i * rows_x)] - (double)P[(size_t)(r + pj * rows_x)];
                    d2 += d * d;
                }
                const double t = std::exp(-d2 / (2 * h * h)) * (double)W[(size_t)(j + c * np)];
                want += t;
                mag += std::fabs(t);
            }
            ratio = std::max(ratio, std::fabs((double)got[(size_t)(i + c * ma)] - want) / (64 * eps * mag));
        }
    return ratio;
}

template <typename T>
void run(const char* name) {
    const int64_t n = 1100, rows_x = 4, s = 2, mz = 70, k = 1050;
    const T h = (T)2;
    std::mt19937_64 gen(4321);
    std::normal_distribution<double> nd;
    auto draw = [&](int64_t cnt) {
        std::vector<T> v((size_t)cnt);
        for (auto& x : v) x = (T)nd(gen);
        return v;
    };
    std::vector<T> P = draw(rows_x * n), Zh = draw(rows_x * mz), Wh = draw(n * s);
    blas::Queue& q = blas::default_queue();
    rlhip_ctx* ctx = q.ctx();
    dev_array<T> Pd(P), Zd(Zh), Wd(Wh), Yd(mz * s), Gd(n * s);
    EXPECT(rlhip_rbf_split_chunks(mz, n) == 2 && rlhip_rbf_split_chunks(n, n) == 2 && rlhip_rbf_split_chunks(mz, k) == 2, "%s: the rule", name);
    auto split = [&] { return (long long)rlhip_rbf_split_count(ctx); };
    auto option = [&] { return (long long)rlhip_get_option(ctx, RLHIP_OPT_RBF_FUSED); };
    EXPECT(option() == -1, "%s: the option starts at %lld", name, option());

    // prediction: off by default, on after set_split_x(true), the option restored
    RL::linops::RBFCrossKernel<T> Kzx(rows_x, mz, Zd.p, n, Pd.p, h, q);
    long long c0 = split();
    RL::krr_predict(Kzx, s, Wd.p, n, Yd.p, mz);
    EXPECT(split() == c0, "%s: split by default", name);
    std::vector<T> Y1 = Yd.host(mz * s);
    Kzx.set_split_x(true);
    RL::krr_predict(Kzx, s, Wd.p, n, Yd.p, mz);
    EXPECT(split() == c0 + 1, "%s: krr_predict with set_split_x(true) moved the split counter by %lld", name, split() - c0);
    EXPECT(option() == -1, "%s: the option is %lld after the call", name, option());
    std::vector<T> Y2 = Yd.host(mz * s);
    const double r1 = product_ratio<T>(rows_x, Zh, mz, P, n, nullptr, (double)h, Wh, s, Y1);
    const double r2 = product_ratio<T>(rows_x, Zh, mz, P, n, nullptr, (double)h, Wh, s, Y2);
    EXPECT(r1 <= 1.0 && r2 <= 1.0, "%s: prediction off by %.3g (one launch) / %.3g (split) of the bound", name, r1, r2);
    // a value the caller had set comes back too, here the composed route: the object's choice wins during its call only
    rlhip_set_option(ctx, RLHIP_OPT_RBF_FUSED, 0);
    const long long composed0 = (long long)rlhip_rbf_path_count(ctx, 56);
    Kzx.matvec(blas::Op::NoTrans, (T)1, Wd.p, (T)0, Yd.p);
    EXPECT(split() == c0 + 2 && option() == 0, "%s: after matvec the counter moved by %lld and the option is %lld", name, split() - c0, option());
    Kzx.set_split_x(false);
    Kzx.matvec(blas::Op::NoTrans, (T)1, Wd.p, (T)0, Yd.p);
    EXPECT(split() == c0 + 2 && (long long)rlhip_rbf_path_count(ctx, 56) == composed0 + 1, "%s: set_split_x(false) did not give the route back", name);
    rlhip_set_option(ctx, RLHIP_OPT_RBF_FUSED, -1);
    // a call that the library refuses (C is NULL) raises, and the option is restored on that path as well
    Kzx.set_split_x(true);
    int raised = 0;
    try { Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, s, (T)1, Wd.p, n, (T)0, (T*)nullptr, mz); } catch (blas::Error const&) { ++raised; }
    EXPECT(raised == 1 && option() == -1, "%s: raised %d, option %lld", name, raised, option());

    // the square operator: set_split_x alone changes nothing, with set_matrix_free(true) the product is split
    std::vector<T> regs{(T)0.5};
    RL::linops::RBFKernelMatrix<T> G(n, Pd.p, rows_x, h, regs, q);
    G.set_split_x(true);
    c0 = split();
    G(blas::Layout::ColMajor, s, (T)1, Wd.p, n, (T)0, Gd.p, n);
    EXPECT(split() == c0, "%s: set_split_x had an effect without set_matrix_free", name);
    G.set_matrix_free(true);
    G(blas::Layout::ColMajor, s, (T)1, Wd.p, n, (T)0, Gd.p, n);
    EXPECT(split() == c0 + 1 && option() == -1, "%s: matrix-free: counter moved by %lld, option %lld", name, split() - c0, option());
    std::vector<T> Gh = Gd.host(n * s);
    const double r3 = product_ratio<T>(rows_x, P, n, P, n, nullptr, (double)h, Wh, s, Gh);
    EXPECT(r3 <= 1.0, "%s: matrix-free split product off by %.3g of the bound", name, r3);

    // restricted prediction on k centres: the operator's choice reaches the cross kernel built inside
    std::vector<int64_t> S((size_t)k);
    for (int64_t j = 0; j < k; ++j) S[(size_t)j] = (7 * j) % n;      // 7 and 1100 are coprime: k distinct centres
    std::vector<T> Ah(Wh.begin(), Wh.begin() + k * s);
    dev_array<T> Ad(Ah);
    c0 = split();
    RL::krr_predict_restricted(G, k, S.data(), mz, Zd.p, rows_x, s, Ad.p, k, Yd.p, mz);
    EXPECT(split() == c0 + 1 && option() == -1, "%s: restricted: counter moved by %lld, option %lld", name, split() - c0, option());
    std::vector<T> Y3 = Yd.host(mz * s);
    const double r4 = product_ratio<T>(rows_x, Zh, mz, P, k, S.data(), (double)h, Ah, s, Y3);
    EXPECT(r4 <= 1.0, "%s: restricted split prediction off by %.3g of the bound", name, r4);

    std::printf("SPLIT<%s> predict=%.3g split_predict=%.3g matrix_free=%.3g restricted=%.3g splits=%lld\n", name, r1, r2, r3, r4, split());
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
