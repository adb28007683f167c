// Host half of posm_square (RandLAPACK/comps/rl_determiter.hh:154-281): what runs after the device Cholesky has failed on the s x s
// system of a PCG step.  Plain C++17, no call into the C ABI and no BLAS / LAPACK (the product links none on the host), so a host-only
// program can test it.  s is the PCG block size -- 64 at the most in practice -- so the eigensolver is a cyclic Jacobi iteration.
//
//   zero_off_diagonal    :154-161
//   jacobi_syev          stands in for lapack::syevd(Job::Vec, Uplo::Lower, ...) at :187: eigenvalues ascending, eigenvectors in the columns
//   psd_sqrt_pinv_host   :181-207
//   posm_square_fallback :258-281
//
// Return codes follow the reference's CODE, not its comment (:166-168 has the two swapped): -(n + 1) the matrix is not positive
// semidefinite, -(n + 2) it is zero up to rounding, otherwise dim(ker) (psd_sqrt_pinv_host) or the rank (posm_square_fallback).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace RandLAPACK {

template <typename T>
void zero_off_diagonal(T* mat, int64_t s) {                                                                                     // :154-161
    for (int64_t i = 0; i < s - 1; ++i) {
        T* ptr_to_next_diag = mat + i + i * s;
        for (int64_t j = 0; j < s; ++j) ptr_to_next_diag[j + 1] = (T)0.0;
    }
}

/// Eigendecomposition of the symmetric n x n matrix whose LOWER triangle is stored in A (column-major, lda): on return the columns of A are
/// orthonormal eigenvectors and w their eigenvalues in ascending order.  Cyclic Jacobi by rows; a rotation is skipped, and its entry set
/// to zero, once the entry no longer changes either diagonal entry or lies below 1e-3 eps ||A||_F, and the iteration ends with the first
/// sweep that rotates nothing.  Returns the number of sweeps, -1 if 60 did not suffice.
template <typename T>
int jacobi_syev(int64_t n, T* A, int64_t lda, T* w) {
    if (n <= 0) return 0;
    std::vector<T> S((size_t)(n * n)), V((size_t)(n * n), T(0));
    auto a = [&](int64_t i, int64_t j) -> T& { return S[(size_t)(i + j * n)]; };
    auto v = [&](int64_t i, int64_t j) -> T& { return V[(size_t)(i + j * n)]; };
    T fro2 = 0;
    for (int64_t j = 0; j < n; ++j) {
        for (int64_t i = j; i < n; ++i) {
            const T x = A[i + j * lda];
            a(i, j) = x;
            a(j, i) = x;
            fro2 += (i == j ? T(1) : T(2)) * x * x;
        }
        v(j, j) = T(1);
    }
    const T eps = std::numeric_limits<T>::epsilon();
    const T floor_abs = T(1e-3) * eps * std::sqrt(fro2);
    int sweeps = 0;
    bool done = false;
    while (!done && sweeps < 60) {
        done = true;
        ++sweeps;
        for (int64_t p = 0; p < n - 1; ++p) {
            for (int64_t q = p + 1; q < n; ++q) {
                const T apq = a(p, q);
                if (apq == T(0)) continue;
                const T g = T(100) * std::abs(apq);
                if (std::abs(apq) <= floor_abs || (std::abs(a(p, p)) + g == std::abs(a(p, p)) && std::abs(a(q, q)) + g == std::abs(a(q, q)))) {
                    a(p, q) = a(q, p) = T(0);
                    continue;
                }
                done = false;
                const T h = a(q, q) - a(p, p);
                T t;
                if (std::abs(h) + g == std::abs(h)) {
                    t = apq / h;
                } else {
                    const T theta = T(0.5) * h / apq;
                    t = T(1) / (std::abs(theta) + std::sqrt(T(1) + theta * theta));
                    if (theta < T(0)) t = -t;
                }
                const T c = T(1) / std::sqrt(T(1) + t * t), sn = t * c;
                for (int64_t k = 0; k < n; ++k) {                       // S <- S J (columns p, q)
                    const T skp = a(k, p), skq = a(k, q);
                    a(k, p) = c * skp - sn * skq;
                    a(k, q) = sn * skp + c * skq;
                }
                for (int64_t k = 0; k < n; ++k) {                       // S <- J^T S (rows p, q)
                    const T spk = a(p, k), sqk = a(q, k);
                    a(p, k) = c * spk - sn * sqk;
                    a(q, k) = sn * spk + c * sqk;
                }
                a(p, q) = a(q, p) = T(0);
                for (int64_t k = 0; k < n; ++k) {                       // V <- V J
                    const T vkp = v(k, p), vkq = v(k, q);
                    v(k, p) = c * vkp - sn * vkq;
                    v(k, q) = sn * vkp + c * vkq;
                }
            }
        }
    }
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return a(x, x) < a(y, y); });
    for (int64_t j = 0; j < n; ++j) {
        const int64_t src = order[(size_t)j];
        w[j] = a(src, src);
        for (int64_t i = 0; i < n; ++i) A[i + j * lda] = v(i, src);
    }
    return done ? sweeps : -1;
}

/// rl_determiter.hh:181-207 on the host: A (lower triangle stored) is replaced by its eigenvectors, work by its eigenvalues, and the
/// trailing n - ker columns are scaled so that pinv(A) = B B^T for that block B.  Returns ker = dim(ker(A)), or -(n + 1) / -(n + 2).
template <typename T>
int64_t psd_sqrt_pinv_host(int64_t n, T* A, int64_t lda, T* work) {
    jacobi_syev(n, A, lda, work);                                                                                               // :187
    const T rel_tol = 10 * std::numeric_limits<T>::epsilon();                                                                   // :188
    const T abs_tol = rel_tol * std::max<T>(T(1), work[n - 1]);                                                                 // :189
    if (work[0] < -abs_tol) return -(n + 1);                                                                                    // :190-192
    if (work[n - 1] < abs_tol) return -(n + 2);                                                                                 // :193-195
    int64_t ker = n;
    while (ker > 0) {                                                                                                           // :198-205
        if (work[ker - 1] > abs_tol) {
            const T sc = 1 / std::sqrt(work[ker - 1]);
            for (int64_t i = 0; i < n; ++i) A[i + (ker - 1) * lda] *= sc;
            ker = ker - 1;
        } else {
            break;
        }
    }
    return ker;
}

/// rl_determiter.hh:258-281 on the host, after the Cholesky attempt has failed: RHS <- pinv(LHS) RHS through the eigendecomposition of LHS
/// (n x n, ld n, lower triangle read, destroyed).  work holds n * n entries.  Returns the rank, or psd_sqrt_pinv_host's error code; RHS is
/// untouched on an error and zero when the rank is zero.
template <typename T>
int64_t posm_square_fallback(int64_t n, T* LHS, T* RHS, T* work) {
    std::copy(LHS, LHS + n * n, work);
    T* LHS_eigvecs = work;                                                                                                      // :260-261
    T* LHS_eigvals = LHS;
    const int64_t ker = psd_sqrt_pinv_host(n, LHS_eigvecs, n, LHS_eigvals);                                                     // :262
    if (ker < 0) return ker;
    if (ker == n) {                                                                                                             // :265-269
        std::fill(RHS, RHS + n * n, T(0));
        return 0;
    }
    const int64_t rank = n - ker;
    const T* pinv_sqrt = &LHS_eigvecs[ker * n];                                                                                 // :272
    std::vector<T> tmp((size_t)(rank * n));
    for (int64_t j = 0; j < n; ++j)                                                                                             // :275-277
        for (int64_t r = 0; r < rank; ++r) {
            T acc = 0;
            for (int64_t i = 0; i < n; ++i) acc += pinv_sqrt[i + r * n] * RHS[i + j * n];
            tmp[(size_t)(r + j * rank)] = acc;
        }
    for (int64_t j = 0; j < n; ++j)                                                                                             // :278-280
        for (int64_t i = 0; i < n; ++i) {
            T acc = 0;
            for (int64_t r = 0; r < rank; ++r) acc += pinv_sqrt[i + r * n] * tmp[(size_t)(r + j * rank)];
            RHS[i + j * n] = acc;
        }
    return rank;
}

}  // namespace RandLAPACK
