// KRILL, kernel ridge regression on the device (RandLAPACK/drivers/rl_krill.hh).
//
// krill_full_rpchol (:20-55): randomly pivoted Cholesky of the unregularized kernel operator -> spectral preconditioner -> block or
// lockstep PCG on (K + mu_i I) x_i = h_i.  n coefficients per right-hand side.
// krill_restricted_rpchol (:57-141, which the reference documents in prose and leaves as a TODO): the k pivots S of the same factorization
// are the centres, column i solves  min_x |K(:,S) x - h_i|^2 + mu_i x^T K(S,S) x  directly -- no iteration, no tolerance, no preconditioner,
// k coefficients per right-hand side.  krill_restricted is the same fit with the centres given by the caller (the reference's second TODO),
// krr_predict_restricted evaluates either model at new points with mz x k kernel evaluations instead of mz x n.  DESIGN 4.24.
// krill_restricted_rpchol_cv and krill_restricted_cv are the two fits with the regularization of every column chosen from a grid by
// leave-one-out or generalized cross-validation, after one factorization and one SVD.  DESIGN 4.26.
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

/// how krill_restricted_rpchol_cv / krill_restricted_cv choose among the values of their grid: the leave-one-out sum of squares, or
/// generalized cross-validation n rss / (n - dof)^2
enum class KrillCriterion { LeaveOneOut = 0, GCV = 1 };

/// The regularization path of a restricted fit, on the HOST.  loo(m, c) and rss(m, c), g x ell with stride g: the sum over the
/// n points of the squared leave-one-out residuals, and of the squared residuals, of column c fitted with mu_grid[m]; dof[m] = sum_j
/// sigma_j^2 / (sigma_j^2 + mu_grid[m]), the trace of the hat matrix; best[c] the index the criterion chose for column c, best_mu[c] =
/// mu_grid[best[c]].
struct KrillRidgePath {
    int64_t g = 0, ell = 0;
    std::vector<double> loo, rss, dof;
    std::vector<int64_t> best;
    std::vector<double> best_mu;
};

/// The basis a restricted fit leaves behind for krr_predict_restricted_var, DEVICE buffers owned by the caller: G (k_in x
/// k_in, ldg >= k_in) receives M^-T W and sigma (k_in) the singular values, where F = U diag(sigma) W^T is the thin SVD of the fit's factor
/// and M = F(S, :).  Behind the achieved rank the rows and columns of G and the entries of sigma are zero.
template <typename T>
struct KrillRestrictedBasis {
    T* G;
    int64_t ldg;
    T* sigma;
};

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

inline int cross_var(blas::Queue& q, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t k, const double* Xs, int64_t ldx, int kernel,
                     double bandwidth, const double* G, int64_t ldg, const double* sigma, int64_t s, const double* mus, int64_t num_mus, double rcond,
                     double* V, int64_t ldv) {
    return rlhip_pdk_cross_var_f64(q.ctx(), rows_x, mz, Z, ldz, k, Xs, ldx, kernel, bandwidth, G, ldg, sigma, s, mus, num_mus, rcond, V, ldv);
}
inline int cross_var(blas::Queue& q, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t k, const float* Xs, int64_t ldx, int kernel,
                     float bandwidth, const float* G, int64_t ldg, const float* sigma, int64_t s, const float* mus, int64_t num_mus, float rcond,
                     float* V, int64_t ldv) {
    return rlhip_pdk_cross_var_f32(q.ctx(), rows_x, mz, Z, ldz, k, Xs, ldx, kernel, bandwidth, G, ldg, sigma, s, mus, num_mus, rcond, V, ldv);
}

inline int ridge_loo(blas::Queue& q, int64_t n, int64_t k, int64_t ell, int64_t g, const double* U, int64_t ldu, const double* sigma, const double* C,
                     int64_t ldc, const double* H, int64_t ldh, const double* mus, double rcond, double* loo, double* rss) {
    return rlhip_ridge_loo_f64(q.ctx(), n, k, ell, g, U, ldu, sigma, C, ldc, H, ldh, mus, rcond, loo, rss);
}
inline int ridge_loo(blas::Queue& q, int64_t n, int64_t k, int64_t ell, int64_t g, const float* U, int64_t ldu, const float* sigma, const float* C,
                     int64_t ldc, const float* H, int64_t ldh, const float* mus, float rcond, double* loo, double* rss) {
    return rlhip_ridge_loo_f32(q.ctx(), n, k, ell, g, U, ldu, sigma, C, ldc, H, ldh, mus, rcond, loo, rss);
}

/// rlhip_pdk_var_set_fused(on) on q's context while alive; the value found is put back
struct VarFusedScope {
    rlhip_ctx* ctx;
    int found;
    VarFusedScope(blas::Queue& q, bool on) : ctx(q.ctx()), found(rlhip_pdk_var_set_fused(q.ctx(), on ? 1 : 0)) {}
    ~VarFusedScope() { rlhip_pdk_var_set_fused(ctx, found > 0 ? 1 : 0); }
    VarFusedScope(VarFusedScope const&) = delete;
    VarFusedScope& operator=(VarFusedScope const&) = delete;
};

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
/// It is written in three pieces -- restricted_alloc, restricted_head (through C = U^T H) and restricted_finish (from the filter on) -- so
/// that restricted_tail_cv can look at U, sigma and C between the two; restricted_tail issues them in the order it always did.
template <typename T>
struct RestrictedWork { T *M, *R, *Rinv, *U, *VT, *sigma, *C, *Y; };

template <typename T>
RestrictedWork<T> restricted_alloc(blas::Scratch& ws, int64_t n, int64_t k, int64_t ell) {
    RestrictedWork<T> w;
    w.M = ws.alloc<T>(k * k);
    w.R = ws.alloc<T>(k * k);
    w.Rinv = ws.alloc<T>(k * k);
    w.U = ws.alloc<T>(n * k);
    w.VT = ws.alloc<T>(k * k);
    w.sigma = ws.alloc<T>(k);
    w.C = ws.alloc<T>(k * ell);
    w.Y = ws.alloc<T>(k * ell);
    return w;
}

/// the tail in front of the filter: M, R = triu(M^T), the thin SVD of F (U n x k with stride n, sigma, VT) and C = U^T H (k x ell, stride k)
template <typename T>
void restricted_head(blas::Queue& q, int64_t n, int64_t k, T* F, int64_t ldf, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh,
                     RestrictedWork<T> const& w) {
    blas::check(_rpchol_impl::gather_rows(q, k, S_dev, k, F, ldf, w.M, k), "gather_rows");
    util::transposition(k, k, w.M, k, w.R, k, 0, q);
    util::get_U(k, k, w.R, k, q);                     // what lies above M's diagonal is rounding: it is not used
    lapack::gesdd(Job::SomeVec, n, k, F, ldf, w.sigma, w.U, n, w.VT, k, q);
    blas::gemm(Layout::ColMajor, Op::Trans, Op::NoTrans, k, ell, n, (T)1, w.U, n, H, ldh, (T)0, w.C, k, q);
}

/// the tail from the filter on, with the num_mus (1 or ell) regularizations mus_dev (DEVICE); C is overwritten.  With a basis (k_in x k_in,
/// k_in >= k): G = Rinv VT^T = M^-T W and sigma, zero behind k -- issued after everything alpha depends on, from blocks nothing else writes.
template <typename T>
void restricted_finish(blas::Queue& q, int64_t n, int64_t k, int64_t ell, RestrictedWork<T> const& w, const T* mus_dev, int64_t num_mus, T* alpha,
                       int64_t ldalpha, KrillRestrictedBasis<T>* basis = nullptr, int64_t k_in = 0) {
    blas::check(ridge_filter(q, k, ell, w.sigma, mus_dev, num_mus, (T)n * std::numeric_limits<T>::epsilon(), w.C, k), "ridge_filter");
    blas::gemm(Layout::ColMajor, Op::Trans, Op::NoTrans, k, ell, k, (T)1, w.VT, k, w.C, k, (T)0, w.Y, k, q);
    util::eye(k, k, w.Rinv, q);
    blas::trsm(Layout::ColMajor, Side::Right, Uplo::Upper, Op::NoTrans, Diag::NonUnit, k, k, (T)1, w.R, k, w.Rinv, k, q);
    blas::gemm(Layout::ColMajor, Op::NoTrans, Op::NoTrans, k, ell, k, (T)1, w.Rinv, k, w.Y, k, (T)0, alpha, ldalpha, q);
    if (basis) {
        if (k < k_in) {
            lapack::laset(MatrixType::General, k_in, k_in, (T)0, (T)0, basis->G, basis->ldg, q);
            blas::device_memset(basis->sigma, 0, k_in, q);
        }
        blas::gemm(Layout::ColMajor, Op::NoTrans, Op::Trans, k, k, k, (T)1, w.Rinv, k, w.VT, k, (T)0, basis->G, basis->ldg, q);
        blas::device_copy_vector(k, w.sigma, basis->sigma, q);
    }
}

/// the basis argument of a fit, checked before anything is enqueued
template <typename T>
void check_basis(const KrillRestrictedBasis<T>* basis, int64_t k_in) {
    if (!basis) return;
    randlapack_require(basis->G != nullptr && basis->sigma != nullptr) << "basis: G and sigma must not be null";
    randlapack_require(basis->ldg >= k_in) << "basis: ldg=" << basis->ldg << " < k=" << k_in;
}

template <typename T>
void restricted_tail(blas::Queue& q, int64_t n, int64_t k, T* F, int64_t ldf, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh,
                     std::vector<T> const& mus, T* alpha, int64_t ldalpha, KrillRestrictedBasis<T>* basis = nullptr, int64_t k_in = 0) {
    blas::Scratch ws(q);
    const RestrictedWork<T> w = restricted_alloc<T>(ws, n, k, ell);
    T* mus_dev = ws.alloc<T>((int64_t)mus.size());
    blas::copy_to_device((int64_t)mus.size(), mus.data(), mus_dev, q);
    restricted_head(q, n, k, F, ldf, S_dev, ell, H, ldh, w);
    restricted_finish(q, n, k, ell, w, mus_dev, (int64_t)mus.size(), alpha, ldalpha, basis, k_in);
}

/// dof[m] = sum_j d_jm with the d of rlhip_ridge_loo_*: sigma_j^2 / (sigma_j^2 + mu_m); mu_m == 0: 1, or 0 where sigma_j <= rcond sigma_0
template <typename T>
std::vector<double> ridge_dof(std::vector<T> const& sigma, int64_t g, const T* mu_grid, T rcond) {
    std::vector<double> dof((size_t)g, 0.0);
    const double cut = sigma.empty() ? 0.0 : (double)rcond * (double)sigma[0];
    for (int64_t m = 0; m < g; ++m) {
        const double mu = (double)mu_grid[m];
        for (T sj : sigma) {
            const double sg = (double)sj;
            dof[(size_t)m] += mu == 0.0 ? (sg <= cut ? 0.0 : 1.0) : (sg * sg) / std::fma(sg, sg, mu);
        }
    }
    return dof;
}

/// per column the index of the smallest finite criterion, the lower index on a tie; a column without a finite value throws
inline void ridge_select(int64_t n, KrillCriterion criterion, KrillRidgePath& path) {
    const int64_t g = path.g, ell = path.ell;
    path.best.assign((size_t)ell, -1);
    for (int64_t c = 0; c < ell; ++c) {
        double best = 0;
        for (int64_t m = 0; m < g; ++m) {
            double v = path.loo[(size_t)(m + c * g)];
            if (criterion == KrillCriterion::GCV) {
                const double left = (double)n - path.dof[(size_t)m];
                v = (double)n * path.rss[(size_t)(m + c * g)] / (left * left);
            }
            if (std::isfinite(v) && (path.best[(size_t)c] < 0 || v < best)) {
                best = v;
                path.best[(size_t)c] = m;
            }
        }
        if (path.best[(size_t)c] < 0) throw Error("krill_restricted_cv: no value of the grid gives column " + std::to_string(c) + " a finite criterion");
    }
}

template <typename T>
void check_mu_grid(int64_t g, const T* mu_grid, KrillCriterion criterion) {
    randlapack_require(g >= 1) << "g=" << g << ": the grid must hold at least one regularization";
    randlapack_require(mu_grid != nullptr) << "mu_grid buffer must not be null";
    for (int64_t m = 0; m < g; ++m) randlapack_require(mu_grid[m] >= (T)0) << "mu_grid[" << m << "]=" << mu_grid[m] << " must be >= 0";
    randlapack_require(criterion == KrillCriterion::LeaveOneOut || criterion == KrillCriterion::GCV) << "unknown criterion";
}

/// restricted_tail with the regularization of every column chosen from the HOST grid mu_grid[g]: head, rlhip_ridge_loo_* on U, sigma and C,
/// the selection on the host, then the filter with the ell chosen values and the rest of the tail as it is.
template <typename T>
void restricted_tail_cv(blas::Queue& q, int64_t n, int64_t k, T* F, int64_t ldf, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh, int64_t g,
                        const T* mu_grid, KrillCriterion criterion, KrillRidgePath& path, T* alpha, int64_t ldalpha,
                        KrillRestrictedBasis<T>* basis = nullptr, int64_t k_in = 0) {
    blas::Scratch ws(q);
    const RestrictedWork<T> w = restricted_alloc<T>(ws, n, k, ell);
    T* grid_dev = ws.alloc<T>(g);
    T* mus_dev = ws.alloc<T>(ell);
    double* table = ws.alloc<double>(2 * g * ell);
    const T rcond = (T)n * std::numeric_limits<T>::epsilon();
    blas::copy_to_device(g, mu_grid, grid_dev, q);
    restricted_head(q, n, k, F, ldf, S_dev, ell, H, ldh, w);
    blas::check(ridge_loo(q, n, k, ell, g, w.U, n, w.sigma, w.C, k, H, ldh, grid_dev, rcond, table, table + g * ell), "ridge_loo");
    path.g = g;
    path.ell = ell;
    path.loo.assign((size_t)(g * ell), 0.0);
    path.rss.assign((size_t)(g * ell), 0.0);
    std::vector<T> sigma((size_t)k);
    blas::copy_to_host(g * ell, table, path.loo.data(), q);
    blas::copy_to_host(g * ell, table + g * ell, path.rss.data(), q);
    blas::copy_to_host(k, w.sigma, sigma.data(), q);
    q.sync();
    path.dof = ridge_dof(sigma, g, mu_grid, rcond);
    ridge_select(n, criterion, path);
    std::vector<T> mus((size_t)ell);
    path.best_mu.assign((size_t)ell, 0.0);
    for (int64_t c = 0; c < ell; ++c) {
        mus[(size_t)c] = mu_grid[path.best[(size_t)c]];
        path.best_mu[(size_t)c] = (double)mus[(size_t)c];
    }
    blas::copy_to_device(ell, mus.data(), mus_dev, q);
    restricted_finish(q, n, k, ell, w, mus_dev, ell, alpha, ldalpha, basis, k_in);
}

/// what the two pairs of fits differ in: where the regularizations come from (checked by prepare()) and the tail that uses them
template <typename T, typename FUNC>
struct FixedRidge {
    std::vector<T> mus;
    void prepare(FUNC& G, int64_t ell) { mus = restricted_mus<T>(G, ell); }
    void tail(blas::Queue& q, int64_t n, int64_t k, T* F, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh, T* alpha, int64_t ldalpha,
              KrillRestrictedBasis<T>* basis, int64_t k_in) {
        restricted_tail(q, n, k, F, n, S_dev, ell, H, ldh, mus, alpha, ldalpha, basis, k_in);
    }
};
template <typename T, typename FUNC>
struct GridRidge {
    int64_t g;
    const T* mu_grid;
    KrillCriterion criterion;
    KrillRidgePath& path;
    void prepare(FUNC&, int64_t) { check_mu_grid(g, mu_grid, criterion); }
    void tail(blas::Queue& q, int64_t n, int64_t k, T* F, const int64_t* S_dev, int64_t ell, const T* H, int64_t ldh, T* alpha, int64_t ldalpha,
              KrillRestrictedBasis<T>* basis, int64_t k_in) {
        restricted_tail_cv(q, n, k, F, n, S_dev, ell, H, ldh, g, mu_grid, criterion, path, alpha, ldalpha, basis, k_in);
    }
};
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

/// The gradients of krr_predict's fitted functions with respect to the evaluation point: G (rows_x x (mz s), ldg >= rows_x),
/// column c * mz + i = the gradient at Z(:, i) of the fitted function of the c-th regularization, laid out like Z.  One call of
/// RBFCrossKernel::grad: no kernel matrix is formed, and the gradient is exact and smooth at coincident points for every kernel kind.
/// All arrays on the DEVICE.
template <typename T>
void krr_predict_grad(linops::RBFCrossKernel<T>& Kzx, int64_t s, const T* coeffs, int64_t ldcoef, T* G, int64_t ldg) {
    randlapack_require(s >= 0) << "s=" << s << " must be >= 0";
    randlapack_require(coeffs != nullptr || s == 0 || Kzx.n_cols == 0) << "coeffs buffer must not be null";
    randlapack_require(G != nullptr || s == 0 || Kzx.n_rows == 0) << "G buffer must not be null";
    Kzx.grad(s, (T)1, coeffs, ldcoef, G, ldg);
}

/// what the factorization inside krill_restricted_rpchol reported, as rlhip_drv_rpchol_* report it: the sampler's status after the last
/// block (0; 1: the residual diagonal is exhausted; 2: it has a negative or NaN entry) and potrf's info of the block that broke down
struct KrillRestrictedInfo { int w_status = 0, c_status = 0; };

namespace _krill_impl {
/// krill_restricted_rpchol and krill_restricted_rpchol_cv: RIDGE is FixedRidge or GridRidge
template <typename T, typename FUNC, typename STATE, typename RIDGE>
STATE restricted_rpchol(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t& k, int64_t* S, T* alpha, int64_t ldalpha, STATE state,
                        int64_t rpchol_block_size, KrillRestrictedInfo* info, RIDGE& ridge, KrillRestrictedBasis<T>* basis) {
    randlapack_require(n > 0) << "n=" << n << " must be > 0";
    randlapack_require(ell > 0) << "ell=" << ell << " must be > 0";
    randlapack_require(H != nullptr) << "H buffer must not be null";
    randlapack_require(ldh >= n) << "ldh=" << ldh << " < n=" << n;
    randlapack_require(S != nullptr) << "S buffer must not be null";
    randlapack_require(alpha != nullptr) << "alpha buffer must not be null";
    ridge.prepare(G, ell);
    if (rpchol_block_size < 0) rpchol_block_size = std::max<int64_t>(1, std::min((int64_t)64, n / 4));
    if (k < 0) k = (int64_t)std::sqrt(n);
    randlapack_require(k >= 1 && k <= n) << "k=" << k << " must be in [1, n=" << n << "]";
    randlapack_require(ldalpha >= k) << "ldalpha=" << ldalpha << " < k=" << k;
    const int64_t k_in = k;
    check_basis(basis, k_in);

    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* F = ws.alloc<T>(n * k_in);
    int64_t* S_dev = ws.alloc<int64_t>(k_in);
    _rpchol_impl::Status st;
    {
        UnregularizedScope<FUNC> unreg(G);
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
    ridge.tail(q, n, k, F, S_dev, ell, H, ldh, alpha, ldalpha, basis, k_in);
    return state;
}

/// krill_restricted and krill_restricted_cv
template <typename T, typename FUNC, typename RIDGE>
int64_t restricted_given(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t k, const int64_t* S, T* alpha, int64_t ldalpha, RIDGE& ridge,
                         KrillRestrictedBasis<T>* basis) {
    randlapack_require(n > 0) << "n=" << n << " must be > 0";
    randlapack_require(ell > 0) << "ell=" << ell << " must be > 0";
    randlapack_require(H != nullptr) << "H buffer must not be null";
    randlapack_require(ldh >= n) << "ldh=" << ldh << " < n=" << n;
    randlapack_require(S != nullptr) << "S buffer must not be null";
    randlapack_require(alpha != nullptr) << "alpha buffer must not be null";
    randlapack_require(k >= 1 && k <= n) << "k=" << k << " must be in [1, n=" << n << "]";
    randlapack_require(ldalpha >= k) << "ldalpha=" << ldalpha << " < k=" << k;
    for (int64_t j = 0; j < k; ++j) randlapack_require(S[j] >= 0 && S[j] < n) << "S[" << j << "]=" << S[j] << " must be in [0, n=" << n << ")";
    ridge.prepare(G, ell);
    check_basis(basis, k);

    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* F = ws.alloc<T>(n * k);
    T* W = ws.alloc<T>(k * k);
    int64_t* S_dev = ws.alloc<int64_t>(k);
    blas::copy_to_device(k, S, S_dev, q);
    {
        UnregularizedScope<FUNC> unreg(G);
        G.columns(k, S_dev, F, n);
    }
    blas::check(_rpchol_impl::gather_rows(q, k, S_dev, k, F, n, W, k), "gather_rows");
    const int64_t info = lapack::potrf(Uplo::Upper, k, W, k, q);
    if (info) return info;
    util::get_U(k, k, W, k, q);
    blas::trsm(Layout::ColMajor, Side::Right, Uplo::Upper, Op::NoTrans, Diag::NonUnit, n, k, (T)1, W, k, F, n, q);
    ridge.tail(q, n, k, F, S_dev, ell, H, ldh, alpha, ldalpha, basis, k);
    return 0;
}
}  // namespace _krill_impl

/// Restricted kernel ridge regression on the pivots of randomly pivoted Cholesky (see the head of this file and _krill_impl::restricted_tail).
/// k: in = the number of centres asked for (< 0: sqrt(n)), out = the achieved rank.  S (HOST, k_in) receives the centres in selection
/// order, alpha (DEVICE, k_in x ell, ldalpha) the coefficients: the fitted function of column i is sum_j alpha(j, i) K(., x_S[j]).  When the
/// factorization stops early, rows k_out .. k_in of alpha are zero and S[k_out ..] is -1; an achieved rank of 0 throws.  H (DEVICE, n x ell,
/// ldh).  O(n k^2) as rp_cholesky itself; scratch: the n x k factor and one more n x k buffer for the SVD's U.  Returns the advanced state.
template <typename T, typename FUNC, typename STATE>
STATE krill_restricted_rpchol(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t& k, int64_t* S, T* alpha, int64_t ldalpha,
                              STATE state, int64_t rpchol_block_size = -1, KrillRestrictedInfo* info = nullptr,
                              KrillRestrictedBasis<T>* basis = nullptr) {
    _krill_impl::FixedRidge<T, FUNC> ridge;
    return _krill_impl::restricted_rpchol(n, G, ell, H, ldh, k, S, alpha, ldalpha, state, rpchol_block_size, info, ridge, basis);
}

/// The same fit with the k centres S (HOST, distinct, each in [0, n)) given: one forced-pivot block of randomly pivoted Cholesky -- A =
/// K(:, S), potrf(Upper) of A(S, :), F = A U^-1 -- in front of the same tail.  Returns potrf's info of K(S,S): 0, or the 1-based position of
/// the first centre that depends on the ones before it; then alpha is untouched (nothing is truncated silently).
template <typename T, typename FUNC>
int64_t krill_restricted(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t k, const int64_t* S, T* alpha, int64_t ldalpha,
                         KrillRestrictedBasis<T>* basis = nullptr) {
    _krill_impl::FixedRidge<T, FUNC> ridge;
    return _krill_impl::restricted_given(n, G, ell, H, ldh, k, S, alpha, ldalpha, ridge, basis);
}

/// krill_restricted_rpchol with the regularization of every column chosen from a grid: mu_grid (HOST, g >= 1 values >= 0) takes
/// the place of G.regs, which is not read.  One factorization and one thin SVD serve the whole grid: rlhip_ridge_loo_* returns, for every grid
/// value and column, the sum of squared leave-one-out residuals and of squared residuals over the n points (for a centre the centre stays
/// and its target is left out).  Column c is then fitted with the grid value of the smallest finite criterion (the lower index on a tie); a
/// column without a finite value throws.  path receives the tables and the choice; everything else is as in krill_restricted_rpchol.
template <typename T, typename FUNC, typename STATE>
STATE krill_restricted_rpchol_cv(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t g, const T* mu_grid, KrillCriterion criterion,
                                 int64_t& k, int64_t* S, T* alpha, int64_t ldalpha, KrillRidgePath& path, STATE state, int64_t rpchol_block_size = -1,
                                 KrillRestrictedInfo* info = nullptr, KrillRestrictedBasis<T>* basis = nullptr) {
    _krill_impl::GridRidge<T, FUNC> ridge{g, mu_grid, criterion, path};
    return _krill_impl::restricted_rpchol(n, G, ell, H, ldh, k, S, alpha, ldalpha, state, rpchol_block_size, info, ridge, basis);
}

/// krill_restricted with the regularizations chosen from mu_grid in the same way.  A non-zero return (potrf's info) leaves alpha and path untouched.
template <typename T, typename FUNC>
int64_t krill_restricted_cv(int64_t n, FUNC& G, int64_t ell, const T* H, int64_t ldh, int64_t g, const T* mu_grid, KrillCriterion criterion, int64_t k,
                            const int64_t* S, T* alpha, int64_t ldalpha, KrillRidgePath& path, KrillRestrictedBasis<T>* basis = nullptr) {
    _krill_impl::GridRidge<T, FUNC> ridge{g, mu_grid, criterion, path};
    return _krill_impl::restricted_given(n, G, ell, H, ldh, k, S, alpha, ldalpha, ridge, basis);
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

/// The gradients of a restricted fit's functions with respect to the evaluation point: Grad (rows_x x (mz s), ldgrad >=
/// rows_x), laid out as krr_predict_grad lays it out.  The centres are gathered as krr_predict_restricted gathers them; the arguments are
/// its arguments and are checked as it checks them.
template <typename T>
void krr_predict_restricted_grad(linops::RBFKernelMatrix<T>& G, int64_t k, const int64_t* S, int64_t mz, const T* Z, int64_t ldz, int64_t s,
                                 const T* alpha, int64_t ldalpha, T* Grad, int64_t ldgrad) {
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
    krr_predict_grad(Kzs, s, alpha, ldalpha > 0 ? ldalpha : 1, Grad, ldgrad);
}

/// The predictive variance of a restricted fit at new points: the fit is the subset-of-regressors / DTC approximation of a
/// Gaussian process with the kernel of G and noise mu_c, and V (DEVICE, mz x s, ldv) receives the variance of its latent function at the
/// points Z (DEVICE, rows_x x mz, ldz) for the s regularizations mus (HOST, num_mus = 1 or s values >= 0 -- an argument, because the _cv fits
/// choose them: path.best_mu):
///   V(i, c) = (1 - sum_j t_ij^2) + sum_j mus_c / (sigma_j^2 + mus_c) t_ij^2,   t_i = K(Z(:, i), X(:, S)) basis.G,
/// the Nystrom residual at the point, clamped at 0, plus the weighted part; k(z, z) = 1 for every kernel kind.  basis is what the fit on the
/// centres S (HOST, k) left; k the achieved rank or the k_in of the fit (the basis is zero behind the rank).  mu == 0 follows the fit's
/// pseudo-inverse with its cut-off G.dim eps.  The centre columns are gathered as krr_predict_restricted gathers them; the rest is one call
/// of rlhip_pdk_cross_var_*.  By default that is its composed route (blocks of t in scratch); fused_kernel = true asks for its fused kernel,
/// which keeps neither the kernel entries nor t in memory and gives every row the same bits whatever mz is, but measured slower.
template <typename T>
void krr_predict_restricted_var(linops::RBFKernelMatrix<T>& G, int64_t k, const int64_t* S, KrillRestrictedBasis<T> const& basis, int64_t mz,
                                const T* Z, int64_t ldz, int64_t s, const T* mus, int64_t num_mus, T* V, int64_t ldv, bool fused_kernel = false) {
    randlapack_require(k >= 0 && k <= 65535) << "k=" << k << " must be in [0, 65535]";
    randlapack_require(S != nullptr || k == 0) << "S buffer must not be null";
    randlapack_require(s >= 0) << "s=" << s << " must be >= 0";
    randlapack_require(mus != nullptr || s == 0) << "mus buffer must not be null";
    randlapack_require(s == 0 || num_mus == 1 || num_mus == s) << "num_mus=" << num_mus << " must equal 1 or s=" << s;
    for (int64_t c = 0; c < (s == 0 ? 0 : num_mus); ++c) randlapack_require(mus[c] >= (T)0) << "regularization mu=" << mus[c] << " must be >= 0";
    randlapack_require((basis.G != nullptr && basis.sigma != nullptr) || k == 0) << "basis: G and sigma must not be null";
    randlapack_require(basis.ldg >= k || k == 0) << "basis: ldg=" << basis.ldg << " < k=" << k;
    for (int64_t j = 0; j < k; ++j) randlapack_require(S[j] >= 0 && S[j] < G.dim) << "S[" << j << "]=" << S[j] << " must be in [0, " << G.dim << ")";
    if (s == 0) return;
    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* Xs = ws.alloc<T>(G.rows_x * k);
    int64_t* S_dev = ws.alloc<int64_t>(k);
    T* mus_dev = ws.alloc<T>(num_mus);
    if (k > 0) {
        blas::copy_to_device(k, S, S_dev, q);
        blas::check(_krill_impl::gather_cols(q, G.rows_x, k, S_dev, G.X, G.ldx, Xs, G.rows_x), "gather_cols");
    }
    blas::copy_to_device(num_mus, mus, mus_dev, q);
    _krill_impl::VarFusedScope fused(q, fused_kernel);
    blas::check(_krill_impl::cross_var(q, G.rows_x, mz, Z, ldz, k, Xs, G.rows_x, (int)G.kernel, G.bandwidth, basis.G, k > 0 ? basis.ldg : 1, basis.sigma,
                                       s, mus_dev, num_mus, (T)G.dim * std::numeric_limits<T>::epsilon(), V, ldv),
                "pdk_cross_var");
}

}  // namespace RandLAPACK
