// Sketched right preconditioners for overdetermined least squares on the device (RandLAPACK/comps/rl_preconditioners.hh): rpc_data_svd
// (:29-86), rpc_data_svd_saso (:135-153) and make_right_orthogonalizer (:193-224).  nystrom_pc_data (:284-315) is not built;
// rpchol_pc_data (:348-361) is in rl_rpchol.hh.
//
// A, V_sk and sigma_sk are DEVICE arrays, column-major: Layout::RowMajor is refused through randlapack_require, as everywhere in the
// C++ layer.  Differences from the reference:
//   - the sketch A_sk = S A is rlhip_saso_apply_* of the library's sparse sign operator (RandBLAS is absent: the random stream is the
//     library's own, the distribution is RandBLAS's short-axis one);
//   - lapack::gesvd(NoVec, OverwriteVec) is the device one-sided Jacobi SVD, rlhip_gesvdj_*, which returns VT in a scratch n x n block;
//     V = VT^T goes into the leading n x n of V_sk (ld n) by rlhip_transpose_* -- what eat_lda_slack + transpose_square leave there;
//   - make_right_orthogonalizer brings sigma down once, runs the reference's threshold loop on the host and scales the first `rank`
//     columns with one rlhip_scal_cols_* call.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_lapackpp.hh"
#include "rl_randblas.hh"
#include "rl_util.hh"
#include "rl_linops.hh"

namespace RandLAPACK {

namespace _precond_impl {
inline void scal_cols(int64_t m, int64_t n, double* A, int64_t lda, const double* s, blas::Queue& q) { blas::check(rlhip_scal_cols_f64(q.ctx(), m, n, A, lda, s), "scal_cols"); }
inline void scal_cols(int64_t m, int64_t n, float* A, int64_t lda, const float* s, blas::Queue& q) { blas::check(rlhip_scal_cols_f32(q.ctx(), m, n, A, lda, s), "scal_cols"); }
// steps 2 and 3 of rpc_data_svd: the SVD of the d x n sketch held in V_sk (ld d); only sigma and VT are wanted
template <typename T>
void svd_of_sketch(int64_t d, int64_t n, T* V_sk, T* sigma_sk, blas::Queue& q) {
    blas::Scratch ws(q);
    T* VT = ws.alloc<T>(n * n);
    lapack::gesvdj(d, n, V_sk, d, sigma_sk, VT, n, q);                                                                              // :70
    util::transposition(n, n, VT, n, V_sk, n, 0, q);                                                                                // :71, 84
    q.sync();                                    // (VT goes back to the arena)
}
}  // namespace _precond_impl

/// V_sk (leading n x n, ld n) <- right singular vectors, sigma_sk (n) <- singular values of the sketch S A.  A: m x n (lda), m >= n;
/// S: a d x m sketching operator of this library (RandBLAS::SparseSkOp: S.dist.n_rows = d >= n); V_sk: at least d * n entries (it holds
/// the sketch first).                                                                                         rl_preconditioners.hh:29-86
template <typename T, typename SKOP>
void rpc_data_svd(Layout layout, int64_t m, int64_t n, const T* A, int64_t lda, SKOP& S, T* V_sk, T* sigma_sk, blas::Queue& q = blas::default_queue()) {
    randlapack_require(layout == Layout::ColMajor) << "rpc_data_svd: only Layout::ColMajor is built";
    int64_t d = S.dist.n_rows;                                                                                                      // :40
    randlapack_require(d >= n) << "sketching dimension d=" << d << " must be >= n=" << n;
    randlapack_require(m >= n) << "Input matrix A must have at least as many rows as columns.";                                     // :43-44
    randlapack_require(lda >= m) << "lda=" << lda << " < m=" << m << " (lda must be >= m)";                                          // :52
    T* A_sk = V_sk;                                                                                                                 // :42
    // step 1: A_sk = S A (beta = 0: A_sk is not read)
    RandBLAS::sketch_general(layout, Op::NoTrans, Op::NoTrans, d, n, m, (T)1.0, S, 0, 0, A, lda, (T)0.0, A_sk, d, q);               // :55-64
    _precond_impl::svd_of_sketch(d, n, A_sk, sigma_sk, q);
}

/// The same for a sparse operator (m x n, m >= n): the sketch S A is the operator's (linops::SparseLinOp::sketch_as_dense: over the nonzeros
/// of A, with the sums of the dense sketch, so that V_sk and sigma_sk are those of the dense copy of A), the SVD is the dense one.
template <typename T, typename SKOP>
void rpc_data_svd(Layout layout, linops::SparseLinOp<T>& A, SKOP& S, T* V_sk, T* sigma_sk) {
    randlapack_require(layout == Layout::ColMajor) << "rpc_data_svd: only Layout::ColMajor is built";
    const int64_t m = A.n_rows, n = A.n_cols, d = S.dist.n_rows;
    randlapack_require(d >= n) << "sketching dimension d=" << d << " must be >= n=" << n;
    randlapack_require(m >= n) << "Input matrix A must have at least as many rows as columns.";
    A.sketch_as_dense(d, S, V_sk);
    _precond_impl::svd_of_sketch(d, n, V_sk, sigma_sk, A.q);
}

/// rpc_data_svd with a sparse sign operator of d rows and k nonzeros per column drawn from `state`; returns the state to use next.
///                                                                                                           rl_preconditioners.hh:135-153
template <typename T, typename RNG>
RandBLAS::RNGState<RNG> rpc_data_svd_saso(Layout layout, int64_t m, int64_t n, int64_t d, int64_t k, const T* A, int64_t lda, T* V_sk, T* sigma_sk,
                                          RandBLAS::RNGState<RNG> state, blas::Queue& q = blas::default_queue()) {
    randlapack_require(layout == Layout::ColMajor) << "rpc_data_svd_saso: only Layout::ColMajor is built";
    RandBLAS::SparseDist D(d, m, k);                                                                                                // :148
    RandBLAS::SparseSkOp<T, RNG> S(D, state, q);                                                                                    // :149-150
    rpc_data_svd(layout, m, n, A, lda, S, V_sk, sigma_sk, q);                                                                       // :151
    return S.next_state;                                                                                                            // :152
}

/// The same for a sparse operator: the sign operator, and therefore the returned state, are those of a dense A of the same shape.
template <typename T, typename RNG>
RandBLAS::RNGState<RNG> rpc_data_svd_saso(Layout layout, linops::SparseLinOp<T>& A, int64_t d, int64_t k, T* V_sk, T* sigma_sk, RandBLAS::RNGState<RNG> state) {
    randlapack_require(layout == Layout::ColMajor) << "rpc_data_svd_saso: only Layout::ColMajor is built";
    RandBLAS::SparseDist D(d, A.n_rows, k);
    RandBLAS::SparseSkOp<T, RNG> S(D, state, A.q);
    rpc_data_svd(layout, A, S, V_sk, sigma_sk);
    return S.next_state;
}

/// V (n x n DEVICE, ld n: right singular vectors of some tall H) and sigma (DEVICE, its singular values) -> the first `rank` columns of V
/// scaled by 1 / sqrt(sigma_i^2 + mu), so that [H; sqrt(mu) I] V[:, :rank] has orthonormal columns.  Returns rank: the columns before the
/// first regularized singular value below sigma_0' cols_V eps.                                                rl_preconditioners.hh:193-224
template <typename T>
int64_t make_right_orthogonalizer(Layout layout, int64_t n, T* V, const T* sigma, T mu, int64_t cols_V = -1, blas::Queue& q = blas::default_queue()) {
    randlapack_require(layout == Layout::ColMajor) << "make_right_orthogonalizer: only Layout::ColMajor is built";
    if (cols_V < 0) cols_V = n;                                                                                                     // :202-204
    randlapack_require(n >= 1 && cols_V >= 1 && cols_V <= n) << "make_right_orthogonalizer needs 1 <= cols_V=" << cols_V << " <= n=" << n;
    std::vector<T> sig((size_t)cols_V), scales((size_t)cols_V);
    blas::copy_to_host(cols_V, sigma, sig.data(), q);
    double sqrtmu = std::sqrt((double)mu);                                                                                          // :205
    auto regularized = [sqrtmu](T s) { return (sqrtmu == 0) ? s : (T)std::hypot((double)s, sqrtmu); };                              // :206-208
    T curr_s = regularized(sig[0]);
    T abstol = curr_s * cols_V * std::numeric_limits<T>::epsilon();                                                                 // :210
    int64_t rank = 0;
    while (rank < cols_V) {                                                                                                         // :215
        curr_s = regularized(sig[(size_t)rank]);
        if (curr_s < abstol) break;
        scales[(size_t)rank] = (T)1.0 / curr_s;                                                                                     // :219
        rank = rank + 1;
    }
    if (rank > 0) {
        blas::Scratch ws(q);
        T* sdev = ws.alloc<T>(rank);
        blas::copy_to_device(rank, scales.data(), sdev, q);
        _precond_impl::scal_cols(n, rank, V, n, sdev, q);                                                                           // :220
        q.sync();                                // (the scales go back to the arena)
    }
    return rank;
}

}  // namespace RandLAPACK
