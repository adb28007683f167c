// Host-only check of include/RandLAPACK_amd/rl_determiter_host.hh (tests/test_pcg_model.py builds it with the address and undefined-
// behaviour sanitizers and links it against nothing).  argv[1]: a binary file of doubles -- count, then per matrix n, the n x n symmetric
// matrix LHS (column-major) and an n x n RHS.  For each matrix, in double and then in float, it prints
//   eig <prec> <n> <sweeps> : eigenvalues (n), eigenvectors (n x n, column-major)        jacobi_syev
//   pinv <prec> <n> <code>  : the matrix psd_sqrt_pinv_host leaves (n x n)                on a fresh copy
//   posm <prec> <n> <code>  : RHS after posm_square_fallback (n x n)                      on a fresh copy
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "RandLAPACK_amd/rl_determiter_host.hh"

template <typename T>
static void print_vec(const std::vector<T>& v, size_t cnt) {
    for (size_t i = 0; i < cnt; ++i) std::printf(" %.17g", (double)v[i]);
    std::printf("\n");
}

template <typename T>
static void run(const char* prec, int64_t n, const double* lhs, const double* rhs) {
    const size_t nn = (size_t)(n * n);
    std::vector<T> A(lhs, lhs + nn), w((size_t)n);
    const int sweeps = RandLAPACK::jacobi_syev<T>(n, A.data(), n, w.data());
    std::printf("eig %s %lld %d :", prec, (long long)n, sweeps);
    std::vector<T> out(w);
    out.insert(out.end(), A.begin(), A.end());
    print_vec(out, out.size());

    std::vector<T> B(lhs, lhs + nn), work((size_t)n);
    const int64_t code = RandLAPACK::psd_sqrt_pinv_host<T>(n, B.data(), n, work.data());
    std::printf("pinv %s %lld %lld :", prec, (long long)n, (long long)code);
    print_vec(B, nn);

    std::vector<T> L(lhs, lhs + nn), R(rhs, rhs + nn), wk(nn);
    const int64_t rank = RandLAPACK::posm_square_fallback<T>(n, L.data(), R.data(), wk.data());
    std::printf("posm %s %lld %lld :", prec, (long long)n, (long long)rank);
    print_vec(R, nn);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    double cnt = 0;
    if (std::fread(&cnt, sizeof(double), 1, f) != 1) return 4;
    for (int m = 0; m < (int)cnt; ++m) {
        double dn = 0;
        if (std::fread(&dn, sizeof(double), 1, f) != 1) return 4;
        const int64_t n = (int64_t)dn;
        std::vector<double> lhs((size_t)(n * n)), rhs((size_t)(n * n));
        if (std::fread(lhs.data(), sizeof(double), lhs.size(), f) != lhs.size()) return 4;
        if (std::fread(rhs.data(), sizeof(double), rhs.size(), f) != rhs.size()) return 4;
        run<double>("f64", n, lhs.data(), rhs.data());
        run<float>("f32", n, lhs.data(), rhs.data());
    }
    std::fclose(f);
    return 0;
}
