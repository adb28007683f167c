// KRILL, kernel ridge regression on the device (RandLAPACK/drivers/rl_krill.hh).
//
// krill_full_rpchol (:20-55): randomly pivoted Cholesky of the unregularized kernel operator -> spectral preconditioner -> block or
// lockstep PCG on (K + mu_i I) x_i = h_i.  n coefficients per right-hand side.
// krill_restricted_rpchol (:57-141, which the reference documents in prose and leaves as a TODO): the k pivots S of the same factorization
// are the centres, column i solves  min_x |K(:,S) x - h_i|^2 + mu_i x^T K(S,S) x  directly -- no iteration, no tolerance, no preconditioner,
// k coefficients per right-hand side.  krill_restricted is the same fit with the centres given by the caller (the reference's second TODO),
// krr_predict_restricted evaluates either model at new points with mz x k kernel evaluations instead of mz x n.  DESIGN 4.24.
//
// G is a regularized kernel operator as linops::RBFKernelMatrix: G.q, G.num_ops, G.regs (HOST), G.set_eval_includes_reg(bool), the
// operator() of pcg and the diag() / columns() of rp_cholesky.  H and X are DEVICE n x ell arrays with stride n.
// Deviations: V and eigvals stay in device scratch and are handed to SpectralPrecond as they are (the reference keeps host
// vectors); a trailing `verbose` defaults to false (the reference passes true to pcg, :52).
// krr_predict (below) evaluates the fitted functions at new points: the step after the solve, which the reference leaves to its caller.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_util.hh"
#include "rl_revd2.hh"
#include "rl_rpchol.hh"
#include "rl_pdkernels.hh"
#include "rl_determiter.hh"

namespace RandLAPACK {

namespace _krill_impl {
template <typename T>
const T* regs_ptr(const T* r) { return r; }
template <typename T>
const T* regs_ptr(std::vector<T> const& r) { return r.data(); }

inline int ridge_filter(blas::Queue& q, int64_t k, int64_t s, const double* sigma, const double* mus, int64_t num_mus, double rcond, double* C,
                        int64_t ldc) {
    return rlhip_ridge_filter_f64(q.ctx(), k, s, sigma, mus, num_mus, rcond, C, ldc);
}
inline int ridge_filter(blas::Queue& q, int64_t k, int64_t s, const float* sigma, const float* mus, int64_t num_mus, float rcond, float* C,
                        int64_t ldc) {
    return rlhip_ridge_filter_f32(q.ctx(), k, s, sigma, mus, num_mus, rcond, C, ldc);
}
inline int gather_cols(blas::Queue& q, int64_t m, int64_t cnt, const int64_t* idx, const double* A, int64_t lda, double* out, int64_t ldo) {
    return rlhip_gather_cols_f64(q.ctx(), m, cnt, idx, A, lda, out, ldo);
}
inline int gather_cols(blas::Queue& q, int64_t m, int64_t cnt, const int64_t* idx, const float* A, int64_t lda, float* out, int64_t ldo) {
    return rlhip_gather_cols_f32(q.ctx(), m, cnt, idx, A, lda, out, ldo);
}

/// set_eval_includes_reg(false) for a factorization, back to true on every way out of the scope
template <typename FUNC>
struct UnregularizedScope {
    FUNC& G;
    explicit UnregularizedScope(FUNC& g) : G(g) { G.set_eval_includes_reg(false); }
    ~UnregularizedScope() { G.set_eval_includes_reg(true); }
    UnregularizedScope(UnregularizedScope const&) = delete;
    UnregularizedScope& operator=(UnregularizedScope const&) = delete;
};

/// the mu_size (1 or ell) regularization parameters of G, checked as krill_full_rpchol checks them
template <typename T, typename FUNC>
std::vector<T> restricted_mus(FUNC& G, int64_t ell) {
    const int64_t mu_size = G.num_ops;
    randlapack_require(mu_size == 1 || mu_size == ell) << "mu_size=" << mu_size << " must equal 1 or ell=" << ell;
    std::vector<T> mus((size_t)mu_size);
    std::copy(regs_ptr<T>(G.regs), regs_ptr<T>(G.regs) + mu_size, mus.data());
    for (T mu : mus) randlapack_require(mu >= (T)0) << "regularization mu=" << mu << " must be >= 0";
    return mus;
}

/// The tail both restricted fits share.  F (DEVICE, n x k, ldf) is a factor of the Nystrom approximation in the order of the k centres
/// S_dev (DEVICE): with M = F(S, :), M M^T = K(S,S) and F M^T = K(:,S), M lower triangular up to rounding.  With y = M^T x the problem
/// min_x |K(:,S) x - h|^2 + mu x^T K(S,S) x is min_y |F y - h|^2 + mu |y|^2, solved through the thin SVD F = U diag(sigma) W^T:
///   M = F(S, :) (gesdd destroys F, so first);  C = U^T H;  C(j, i) *= sigma_j / (sigma_j^2 + mu_i);  Y = W C;  M^T alpha = Y.
/// It works on F, not on the Gram matrix F^T F: the conditioning is cond(F), not its square.  mu_i == 0 is the pseudo-inverse with the
/// cut-off sigma_j <= n eps sigma_0.  The library's trsm serves Right / Upper / NoTrans only, so the last step is the one posm_square's
/// composed route takes: R = triu(M^T), R^-1 = I R^-1 by that trsm (k x k), alpha = R^-1 Y by one small product.
/// F is destroyed.  O(n k^2) work; scratch: one n x k buffer for U (the footprint of rpchol_pc_data), four k x k and two k x ell blocks.
/// alpha (DEVICE, k x ell, ldalpha).  Host steps: the copy of the mus, and the reads gesdd makes to choose its route.
template <typename T>
void restricted_tail(blas::Queue& q, int64_t n, int64_t k, T* F, int64_t ldf, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh,
                     std::vector<T> const& mus, T* alpha, int64_t ldalpha) {
    blas::Scratch ws(q);
    T* M = ws.alloc<T>(k * k);
    T* R = ws.alloc<T>(k * k);
    T* Rinv = ws.alloc<T>(k * k);
    T* U = ws.alloc<T>(n * k);
    T* VT = ws.alloc<T>(k * k);
    T* sigma = ws.alloc<T>(k);
    T* C = ws.alloc<T>(k * ell);
    T* Y = ws.alloc<T>(k * ell);
    T* mus_dev = ws.alloc<T>((int64_t)mus.size());
    blas::copy_to_device((int64_t)mus.size(), mus.data(), mus_dev, q);
    blas::check(_rpchol_impl::gather_rows(q, k, S_dev, k, F, ldf, M, k), "gather_rows");
    util::transposition(k, k, M, k, R, k, 0, q);
    util::get_U(k, k, R, k, q);                       // what lies above M's diagonal is rounding: it is not used
    lapack::gesdd(Job::SomeVec, n, k, F, ldf, sigma, U, n, VT, k, q);
    blas::gemm(Layout::ColMajor, Op::Trans, Op::NoTrans, k, ell, n, (T)1, U, n, H, ldh, (T)0, C, k, q);
    blas::check(ridge_filter(q, k, ell, sigma, mus_dev, (int64_t)mus.size(), (T)n * std::numeric_limits<T>::epsilon(), C, k), "ridge_filter");
    blas::gemm(Layout::ColMajor, Op::Trans, Op::NoTrans, k, ell, k, (T)1, VT, k, C, k, (T)0, Y, k, q);
    util::eye(k, k, Rinv, q);
    blas::trsm(Layout::ColMajor, Side::Right, Uplo::Upper, Op::NoTrans, Diag::NonUnit, k, k, (T)1, R, k, Rinv, k, q);
    blas::gemm(Layout::ColMajor, Op::NoTrans, Op::NoTrans, k, ell, k, (T)1, Rinv, k, Y, k, (T)0, alpha, ldalpha, q);
}
}  // namespace _krill_impl

template <typename T, typename FUNC, typename SEMINORM, typename STATE>
STATE krill_full_rpchol(int64_t n, FUNC& G, int64_t ell, const T* H, T* X, T tol, STATE state, SEMINORM& seminorm, int64_t rpchol_block_size = -1,
                        int64_t max_iters = 20, int64_t k = -1, bool verbose = false, int64_t* iters = nullptr, int64_t* k_out = nullptr) {
    randlapack_require(n > 0) << "n=" << n << " must be > 0";                                                                       // :28-33
    randlapack_require(ell > 0) << "ell=" << ell << " must be > 0";
    randlapack_require(tol >= (T)0) << "tol=" << tol << " must be >= 0";
    randlapack_require(max_iters > 0) << "max_iters=" << max_iters << " must be > 0";
    randlapack_require(H != nullptr) << "H buffer must not be null";
    randlapack_require(X != nullptr) << "X buffer must not be null";

    int64_t mu_size = G.num_ops;                                                                                                    // :35-38
    std::vector<T> mus((size_t)mu_size);
    std::copy(_krill_impl::regs_ptr<T>(G.regs), _krill_impl::regs_ptr<T>(G.regs) + mu_size, mus.data());
    randlapack_require(mu_size == 1 || mu_size == ell) << "mu_size=" << mu_size << " must equal 1 or ell=" << ell;

    if (rpchol_block_size < 0) rpchol_block_size = std::min((int64_t)64, n / 4);                                                    // :40-43
    if (k < 0) k = (int64_t)std::sqrt(n);
    randlapack_require(k >= 1 && k <= n) << "k=" << k << " must be in [1, n=" << n << "]";

    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* V = ws.alloc<T>(n * k);                                                                                                      // :45-46
    T* eigvals = ws.alloc<T>(k);
    blas::device_memset(V, 0, n * k, q);
    blas::device_memset(eigvals, 0, k, q);
    G.set_eval_includes_reg(false);
    state = rpchol_pc_data(n, G, k, rpchol_block_size, V, eigvals, state);                                                          // :48
    randlapack_require(k >= 1) << "rpchol_pc_data returned an empty factor";
    if (k_out) *k_out = k;
    linops::SpectralPrecond<T> invP(n, q);                                                                                          // :49
    invP.prep(V, n, eigvals, k, mus, ell);                                                                                          // :50
    G.set_eval_includes_reg(true);
    pcg(G, H, ell, seminorm, tol, max_iters, invP, X, verbose, iters);                                                              // :52
    return state;
}

/// Prediction with the coefficients of krill_full_rpchol: Y (mz x s, ldy) = K(Z, X_train) * coeffs (n x s, ldcoef), where Kzx is the
/// cross kernel between the mz evaluation points and the n training points.  Column i of Y is the fitted function of the i-th
/// regularization at the points of Z.  All arrays on the DEVICE.  (The reference stops at the coefficients)
/// Few evaluation points against many training points: Kzx.set_split_x(true) beforehand splits the fused kernel's walk over the training
/// points; the choice travels with the operator, so there is no argument for it here.
template <typename T>
void krr_predict(linops::RBFCrossKernel<T>& Kzx, int64_t s, const T* coeffs, int64_t ldcoef, T* Y, int64_t ldy) {
    randlapack_require(s >= 0) << "s=" << s << " must be >= 0";
    randlapack_require(coeffs != nullptr || s == 0 || Kzx.n_cols == 0) << "coeffs buffer must not be null";
    randlapack_require(Y != nullptr || s == 0 || Kzx.n_rows == 0) << "Y buffer must not be null";
    Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, s, (T)1, coeffs, ldcoef, (T)0, Y, ldy);
}

/// what the factorization inside krill_restricted_rpchol reported, as rlhip_drv_rpchol_* report it: the sampler's status after the last
/// block (0; 1: the residual diagonal is exhausted; 2: it has a negative or NaN entry) and potrf's info of the block that broke down
struct KrillRestrictedInfo { int w_status = 0, c_status = 0; };

/// Restricted kernel ridge regression on the pivots of randomly pivoted Cholesky (see the head of this file and _krill_impl::restricted_tail).
/// k: in = the number of centres asked for (< 0: sqrt(n)), out = the achieved rank.  S (HOST, k_in) receives the centres in selection
/// order, alpha (DEVICE, k_in x ell, ldalpha) the coefficients: the fitted function of column i is sum_j alpha(j, i) K(., x_S[j]).  When the
/// factorization stops early, rows k_out .. k_in of alpha are zero and S[k_out ..] is -1; an achieved rank of 0 throws.  H (DEVICE, n x ell,
/// ldh).  O(n k^2) as rp_cholesky itself; scratch: the n x k factor and one more n x k buffer for the SVD's U.  Returns the advanced state.
template <typename T, typename FUNC, typename STATE>
STATE krill_restricted_rpchol(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t& k, int64_t* S, T* alpha, int64_t ldalpha,
                              STATE state, int64_t rpchol_block_size = -1, KrillRestrictedInfo* info = nullptr) {
    randlapack_require(n > 0) << "n=" << n << " must be > 0";
    randlapack_require(ell > 0) << "ell=" << ell << " must be > 0";
    randlapack_require(H != nullptr) << "H buffer must not be null";
    randlapack_require(ldh >= n) << "ldh=" << ldh << " < n=" << n;
    randlapack_require(S != nullptr) << "S buffer must not be null";
    randlapack_require(alpha != nullptr) << "alpha buffer must not be null";
    const std::vector<T> mus = _krill_impl::restricted_mus<T>(G, ell);
    if (rpchol_block_size < 0) rpchol_block_size = std::max<int64_t>(1, std::min((int64_t)64, n / 4));
    if (k < 0) k = (int64_t)std::sqrt(n);
    randlapack_require(k >= 1 && k <= n) << "k=" << k << " must be in [1, n=" << n << "]";
    randlapack_require(ldalpha >= k) << "ldalpha=" << ldalpha << " < k=" << k;
    const int64_t k_in = k;

    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* F = ws.alloc<T>(n * k_in);
    int64_t* S_dev = ws.alloc<int64_t>(k_in);
    _rpchol_impl::Status st;
    {
        _krill_impl::UnregularizedScope<FUNC> unreg(G);
        st = _rpchol_impl::run(n, G, k, S, F, n, rpchol_block_size, state);
    }
    if (info) {
        info->w_status = st.w_status;
        info->c_status = st.c_status;
    }
    if (st.initial)
        throw Error("krill_restricted_rpchol: the diagonal is not a valid weight vector (weights_to_cdf status " + std::to_string(st.w_status) + ")");
    randlapack_require(k >= 1) << "rp_cholesky returned an empty factor";
    std::fill(S + k, S + k_in, (int64_t)-1);
    lapack::laset(MatrixType::General, k_in, ell, (T)0, (T)0, alpha, ldalpha, q);
    blas::copy_to_device(k, S, S_dev, q);
    _krill_impl::restricted_tail(q, n, k, F, n, S_dev, ell, H, ldh, mus, alpha, ldalpha);
    return state;
}

/// The same fit with the k centres S (HOST, distinct, each in [0, n)) given: one forced-pivot block of randomly pivoted Cholesky -- A =
/// K(:, S), potrf(Upper) of A(S, :), F = A U^-1 -- in front of the same tail.  Returns potrf's info of K(S,S): 0, or the 1-based position of
/// the first centre that depends on the ones before it; then alpha is untouched (nothing is truncated silently).
template <typename T, typename FUNC>
int64_t krill_restricted(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t k, const int64_t* S, T* alpha, int64_t ldalpha) {
    randlapack_require(n > 0) << "n=" << n << " must be > 0";
    randlapack_require(ell > 0) << "ell=" << ell << " must be > 0";
    randlapack_require(H != nullptr) << "H buffer must not be null";
    randlapack_require(ldh >= n) << "ldh=" << ldh << " < n=" << n;
    randlapack_require(S != nullptr) << "S buffer must not be null";
    randlapack_require(alpha != nullptr) << "alpha buffer must not be null";
    randlapack_require(k >= 1 && k <= n) << "k=" << k << " must be in [1, n=" << n << "]";
    randlapack_require(ldalpha >= k) << "ldalpha=" << ldalpha << " < k=" << k;
    for (int64_t j = 0; j < k; ++j) randlapack_require(S[j] >= 0 && S[j] < n) << "S[" << j << "]=" << S[j] << " must be in [0, n=" << n << ")";
    const std::vector<T> mus = _krill_impl::restricted_mus<T>(G, ell);

    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* F = ws.alloc<T>(n * k);
    T* W = ws.alloc<T>(k * k);
    int64_t* S_dev = ws.alloc<int64_t>(k);
    blas::copy_to_device(k, S, S_dev, q);
    {
        _krill_impl::UnregularizedScope<FUNC> unreg(G);
        G.columns(k, S_dev, F, n);
    }
    blas::check(_rpchol_impl::gather_rows(q, k, S_dev, k, F, n, W, k), "gather_rows");
    const int64_t info = lapack::potrf(Uplo::Upper, k, W, k, q);
    if (info) return info;
    util::get_U(k, k, W, k, q);
    blas::trsm(Layout::ColMajor, Side::Right, Uplo::Upper, Op::NoTrans, Diag::NonUnit, n, k, (T)1, W, k, F, n, q);
    _krill_impl::restricted_tail(q, n, k, F, n, S_dev, ell, H, ldh, mus, alpha, ldalpha);
    return 0;
}

/// Prediction with the coefficients of a restricted fit: Y (mz x s, ldy) = K(Z, X(:, S)) alpha (k x s, ldalpha), with G's points, kernel
/// function and bandwidth.  The k centre columns of G.X are gathered into scratch and krr_predict runs on them: mz x k kernel
/// evaluations.  S HOST (every entry in [0, G.dim)), everything else DEVICE.  Z: rows_x x mz, ldz.  G.set_split_x(true) is handed on to
/// the cross kernel built here, as G's kernel function is.
template <typename T>
void krr_predict_restricted(linops::RBFKernelMatrix<T>& G, int64_t k, const int64_t* S, int64_t mz, const T* Z, int64_t ldz, int64_t s,
                            const T* alpha, int64_t ldalpha, T* Y, int64_t ldy) {
    randlapack_require(k >= 0 && k <= 65535) << "k=" << k << " must be in [0, 65535]";
    randlapack_require(S != nullptr || k == 0) << "S buffer must not be null";
    randlapack_require(ldalpha >= k) << "ldalpha=" << ldalpha << " < k=" << k;
    for (int64_t j = 0; j < k; ++j) randlapack_require(S[j] >= 0 && S[j] < G.dim) << "S[" << j << "]=" << S[j] << " must be in [0, " << G.dim << ")";
    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* Xs = ws.alloc<T>(G.rows_x * k);
    int64_t* S_dev = ws.alloc<int64_t>(k);
    if (k > 0) {
        blas::copy_to_device(k, S, S_dev, q);
        blas::check(_krill_impl::gather_cols(q, G.rows_x, k, S_dev, G.X, G.ldx, Xs, G.rows_x), "gather_cols");
    }
    linops::RBFCrossKernel<T> Kzs(G.rows_x, mz, Z, k, Xs, G.bandwidth, q, ldz, G.rows_x);
    Kzs.set_kernel(G.kernel);
    Kzs.set_split_x(G._split_x);
    krr_predict(Kzs, s, alpha, ldalpha > 0 ? ldalpha : 1, Y, ldy);
}

}  // namespace RandLAPACK
