// Sketch-and-precondition least squares on the device: sap_lstsq chains rpc_data_svd_saso, make_right_orthogonalizer and pcg_saddle.
// This is the one function of the solver layer WITHOUT a counterpart in the reference, whose tests chain the three by hand
// (test/comps/test_determiter.cc, test_preconditioners.cc and the pcgls helper built on them).  The overload with s right-hand sides builds
// the preconditioner once and runs pcg_saddle_block: s conjugate-gradient iterations in lockstep on one normal product.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_randblas.hh"
#include "rl_linops.hh"
#include "rl_preconditioners.hh"
#include "rl_determiter.hh"

namespace RandLAPACK {

struct SapLstsqResult {
    int64_t rank = 0;    // columns of the orthogonalizer M
    int64_t iters = 0;   // pcg_saddle iterations run
};

/// min ||A x - b||^2 + delta ||x||^2 + 2 c'x, i.e. (A'A + delta I) x = A'b - c, for a tall A (m x n, lda, DEVICE): a sparse sign sketch with
/// d = ceil(d_factor n) rows and nnz nonzeros per column, its SVD as the right preconditioner (mu = delta), then pcg_saddle from x0 = 0 with
/// the relative tolerance tol and at most iter_lim iterations.  b, y: m; c, x: n; all DEVICE.  `state` is advanced as rpc_data_svd_saso
/// advances it.  resid_vec (DEVICE, iter_lim + 1 entries; may be NULL) receives pcg_saddle's residual history.
template <typename T, typename RNG>
SapLstsqResult sap_lstsq(int64_t m, int64_t n, const T* A, int64_t lda, const T* b, const T* c, T delta, T d_factor, int64_t nnz, T tol, int64_t iter_lim,
                         T* x, T* y, RandBLAS::RNGState<RNG>& state, blas::Queue& q = blas::default_queue(), T* resid_vec = nullptr) {
    randlapack_require(m >= n && n >= 1) << "sap_lstsq needs m=" << m << " >= n=" << n << " >= 1";
    randlapack_require(d_factor >= (T)1.0) << "d_factor=" << d_factor << " must be >= 1";
    randlapack_require(iter_lim >= 0) << "iter_lim=" << iter_lim << " must be >= 0";
    int64_t d = (int64_t)std::ceil((double)d_factor * (double)n);
    blas::Scratch ws(q);
    T* V_sk = ws.alloc<T>(d * n);
    T* sigma_sk = ws.alloc<T>(n);
    T* x0 = ws.alloc<T>(n);
    T* resid = resid_vec ? resid_vec : ws.alloc<T>(iter_lim + 1);
    state = rpc_data_svd_saso(Layout::ColMajor, m, n, d, nnz, A, lda, V_sk, sigma_sk, state, q);
    SapLstsqResult out;
    out.rank = make_right_orthogonalizer(Layout::ColMajor, n, V_sk, sigma_sk, delta, n, q);
    randlapack_require(out.rank >= 1) << "sap_lstsq: the sketch of A has numerical rank 0";
    blas::device_memset(x0, 0, n, q);
    pcg_saddle(m, n, A, lda, b, c, delta, iter_lim, resid, tol, out.rank, V_sk, n, x0, x, y, q, &out.iters);
    return out;
}

struct SapLstsqBlockResult {
    int64_t rank = 0;              // columns of the orthogonalizer M
    std::vector<int64_t> iters;    // pcg_saddle_block iterations each column ran
};

/// The same for s right-hand sides: B, Y: m x s (ldb, ldy); C: n x s (ldc; NULL: zero); X: n x s (ldx); resid (DEVICE,
/// (iter_lim + 1) x s with stride iter_lim + 1; may be NULL) receives the residual histories.  ONE rpc_data_svd_saso and one
/// make_right_orthogonalizer serve all columns -- `state` is advanced exactly as the single-column call advances it -- then
/// pcg_saddle_block runs from X0 = 0: one normal product per iteration for all columns.
template <typename T, typename RNG>
SapLstsqBlockResult sap_lstsq(int64_t m, int64_t n, const T* A, int64_t lda, int64_t s, const T* B, int64_t ldb, const T* C, int64_t ldc, T delta,
                              T d_factor, int64_t nnz, T tol, int64_t iter_lim, T* X, int64_t ldx, T* Y, int64_t ldy, RandBLAS::RNGState<RNG>& state,
                              blas::Queue& q = blas::default_queue(), T* resid = nullptr) {
    randlapack_require(m >= n && n >= 1) << "sap_lstsq needs m=" << m << " >= n=" << n << " >= 1";
    randlapack_require(s >= 0) << "s=" << s << " must be >= 0";
    randlapack_require(d_factor >= (T)1.0) << "d_factor=" << d_factor << " must be >= 1";
    randlapack_require(iter_lim >= 0) << "iter_lim=" << iter_lim << " must be >= 0";
    int64_t d = (int64_t)std::ceil((double)d_factor * (double)n);
    blas::Scratch ws(q);
    T* V_sk = ws.alloc<T>(d * n);
    T* sigma_sk = ws.alloc<T>(n);
    T* res = resid ? resid : ws.alloc<T>((iter_lim + 1) * (s > 0 ? s : 1));
    state = rpc_data_svd_saso(Layout::ColMajor, m, n, d, nnz, A, lda, V_sk, sigma_sk, state, q);
    SapLstsqBlockResult out;
    out.rank = make_right_orthogonalizer(Layout::ColMajor, n, V_sk, sigma_sk, delta, n, q);
    randlapack_require(out.rank >= 1) << "sap_lstsq: the sketch of A has numerical rank 0";
    out.iters.assign((size_t)s, 0);
    pcg_saddle_block(m, n, A, lda, s, B, ldb, C, ldc, delta, iter_lim, res, iter_lim + 1, tol, out.rank, (const T*)V_sk, n, (const T*)nullptr, n, X, ldx, Y,
                     ldy, q, out.iters.data());
    return out;
}

/// The same chain for a sparse operator A (m x n, m >= n; linops::SparseLinOp over CSR, CSC or COO storage): the sketch is the operator's
/// own scatter, every product of the iteration a sparse matrix-vector product (csrc/spmv.hip).  A is never densified.
template <typename T, typename RNG>
SapLstsqResult sap_lstsq(linops::SparseLinOp<T>& A, const T* b, const T* c, T delta, T d_factor, int64_t nnz, T tol, int64_t iter_lim, T* x, T* y,
                         RandBLAS::RNGState<RNG>& state, T* resid_vec = nullptr) {
    const int64_t m = A.n_rows, n = A.n_cols;
    blas::Queue& q = A.q;
    randlapack_require(!(A.row_sharded && q.world() > 1)) << "sap_lstsq is not defined for a row-sharded operator";
    randlapack_require(m >= n && n >= 1) << "sap_lstsq needs m=" << m << " >= n=" << n << " >= 1";
    randlapack_require(d_factor >= (T)1.0) << "d_factor=" << d_factor << " must be >= 1";
    randlapack_require(iter_lim >= 0) << "iter_lim=" << iter_lim << " must be >= 0";
    int64_t d = (int64_t)std::ceil((double)d_factor * (double)n);
    blas::Scratch ws(q);
    T* V_sk = ws.alloc<T>(d * n);
    T* sigma_sk = ws.alloc<T>(n);
    T* x0 = ws.alloc<T>(n);
    T* resid = resid_vec ? resid_vec : ws.alloc<T>(iter_lim + 1);
    state = rpc_data_svd_saso(Layout::ColMajor, A, d, nnz, V_sk, sigma_sk, state);
    SapLstsqResult out;
    out.rank = make_right_orthogonalizer(Layout::ColMajor, n, V_sk, sigma_sk, delta, n, q);
    randlapack_require(out.rank >= 1) << "sap_lstsq: the sketch of A has numerical rank 0";
    blas::device_memset(x0, 0, n, q);
    pcg_saddle(A, (const T*)b, (const T*)c, delta, iter_lim, resid, tol, out.rank, (const T*)V_sk, n, (const T*)x0, x, y, &out.iters);
    return out;
}

}  // namespace RandLAPACK
