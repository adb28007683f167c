// Randomly pivoted Cholesky, device flavour (RandLAPACK/comps/rl_rpchol.hh; Algorithm 4 of arXiv:2304.12465) and the preconditioner
// data built on it (rpchol_pc_data, RandLAPACK/comps/rl_preconditioners.hh:348-361).
//
// Deviations from the reference:
//   - A is not a host functor A_stateless(i, j) but any operator with
//         A.q                                                   the blas::Queue the work goes to
//         A.diag(T* d_dev)                                      its n diagonal entries
//         A.columns(nidx, const int64_t* idx_dev, T* out, ldo)  its columns idx_dev[0:nidx)
//     linops::RBFKernelMatrix (rl_pdkernels.hh) and linops::ExplicitSymLinOp (rl_revd2.hh) provide them;
//   - S is a HOST int64_t array as in the reference, F a DEVICE n x k buffer with ld n (as RSVD's outputs);
//   - weights_to_cdf + sample_indices_iid are rlhip_sample_indices_iid_* (include/rlhip.h): prefix sums in double for both precisions, the
//     library's own Philox stream; the state advances by ceil(curr_B / 2) per block;
//   - after a Cholesky breakdown (c_status = info) the solve uses the leading (info - 1) x (info - 1) factor with its true leading dimension
//     (the reference passes the truncated size as ld, rl_rpchol.hh:174);
//   - nothing is printed on an early exit; rlhip_drv_rpchol_* report w_status / c_status instead.
//
// Per block: 1 sampler (one host read: status, unique count, the indices), 2 kernel columns into F(:, ell:ell+cnt), 3 gather F(S', 0:ell) and
// the downdate GEMM F_panel -= F(:, 0:ell) F(S', 0:ell)^T, 4 gather G = F_panel(S', :) and potrf (one host read: info), 5 panel finish
// (trsm F_panel U^-1, d -= row norms^2, d[S'] = 0).  Two host reads per block, and one status-only sampler call after the last block.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_lapackpp.hh"
#include "rl_randblas.hh"
#include "rl_util.hh"
#include "rl_revd2.hh"
#include "rl_pdkernels.hh"

namespace RandLAPACK {

namespace _rpchol_impl {

inline int sample(blas::Queue& q, int64_t n, const double* d, int64_t k, const uint32_t* ctr, const uint32_t* key, uint32_t* next,
                  int64_t* out_dev, int64_t* out_host, int64_t* count, int* status) {
    return rlhip_sample_indices_iid_f64(q.ctx(), n, d, k, 1, ctr, key, next, out_dev, out_host, count, status);
}
inline int sample(blas::Queue& q, int64_t n, const float* d, int64_t k, const uint32_t* ctr, const uint32_t* key, uint32_t* next,
                  int64_t* out_dev, int64_t* out_host, int64_t* count, int* status) {
    return rlhip_sample_indices_iid_f32(q.ctx(), n, d, k, 1, ctr, key, next, out_dev, out_host, count, status);
}
inline int gather_rows(blas::Queue& q, int64_t cnt, const int64_t* idx, int64_t ncols, const double* A, int64_t lda, double* out, int64_t ldo) {
    return rlhip_gather_rows_f64(q.ctx(), cnt, idx, ncols, A, lda, out, ldo);
}
inline int gather_rows(blas::Queue& q, int64_t cnt, const int64_t* idx, int64_t ncols, const float* A, int64_t lda, float* out, int64_t ldo) {
    return rlhip_gather_rows_f32(q.ctx(), cnt, idx, ncols, A, lda, out, ldo);
}
inline int panel_finish(blas::Queue& q, int64_t n, int64_t cols, const double* U, int64_t ldu, double* F, int64_t ldf, double* d, const int64_t* s) {
    return rlhip_rpchol_panel_finish_f64(q.ctx(), n, cols, U, ldu, F, ldf, d, s);
}
inline int panel_finish(blas::Queue& q, int64_t n, int64_t cols, const float* U, int64_t ldu, float* F, int64_t ldf, float* d, const int64_t* s) {
    return rlhip_rpchol_panel_finish_f32(q.ctx(), n, cols, U, ldu, F, ldf, d, s);
}

struct Status {
    int w_status = 0;       // downdate_d_and_cdf's code (rl_rpchol.hh:47-72) after the last block
    int c_status = 0;       // potrf's info of the block that broke down (:168-173)
    bool initial = false;   // the diagonal itself failed weights_to_cdf (the reference throws there, :64)
};

/// rl_rpchol.hh:114-185 with F's leading dimension explicit; k: in = target rank, out = achieved rank
template <typename T, typename KOP, typename STATE>
Status run(int64_t n, KOP& A, int64_t& k, int64_t* S, T* F, int64_t ldf, int64_t b, STATE& state) {
    randlapack_require(n >= 1) << "n=" << n << " must be >= 1";
    randlapack_require(k >= 0 && k <= n) << "k=" << k << " must be in [0, n=" << n << "]";
    randlapack_require(b >= 1 && b <= 4096) << "block size b=" << b << " must be in [1, 4096]";
    randlapack_require(ldf >= n) << "ldf=" << ldf << " < n=" << n;
    blas::Queue& q = A.q;
    Status r;
    blas::Scratch ws(q);
    T* d = ws.alloc<T>(n);
    int64_t* Sp = ws.alloc<int64_t>(b);
    T* W = ws.alloc<T>(b * std::max(k, b));             // F(S', 0:ell) (cnt x ell, ell < k), then G = F_panel(S', :) (cnt x cnt)
    std::vector<int64_t> Sp_host((size_t)b);
    A.diag(d);                                                                                                      // :124-125
    int64_t ell = 0;
    bool first = true;
    while (ell < k && r.w_status == 0 && r.c_status == 0) {
        const int64_t curr_B = std::min(b, k - ell);                                                                // :134
        int64_t cnt = 0;
        int st = 0;
        STATE next = state;
        blas::check(sample(q, n, d, curr_B, state.counter.data(), state.key.data(), next.counter.data(), Sp, Sp_host.data(), &cnt, &st),
                    "sample_indices_iid");                                                                          // :141-144
        if (st) {                        // the status of the previous downdate (or of the diagonal): the reference stops before drawing
            r.w_status = st;
            r.initial = first;
            break;
        }
        first = false;
        state = next;
        T* Fp = F + ell * ldf;
        A.columns(cnt, Sp, Fp, ldf);                                                                                // :158
        if (ell > 0) {
            blas::check(gather_rows(q, cnt, Sp, ell, F, ldf, W, cnt), "gather_rows");                            // :160
            blas::gemm(Layout::ColMajor, Op::NoTrans, Op::Trans, n, cnt, ell, (T)-1, F, ldf, W, cnt, (T)1, Fp, ldf, q);   // :162-165
        }
        blas::check(gather_rows(q, cnt, Sp, cnt, Fp, ldf, W, cnt), "gather_rows");                               // :169
        int64_t ell_incr = cnt;
        const int64_t info = lapack::potrf(Uplo::Upper, cnt, W, cnt, q);                                            // :170
        if (info) {
            r.c_status = (int)info;
            ell_incr = info - 1;                                                                                    // :171-173
        }
        blas::check(panel_finish(q, n, ell_incr, W, cnt, Fp, ldf, d, Sp), "rpchol_panel_finish");                // :174-178, :47-62
        std::copy(Sp_host.begin(), Sp_host.begin() + ell_incr, S + ell);                                            // :183
        ell += ell_incr;
    }
    if (r.w_status == 0 && !first) {     // the last downdate's status (:184), which no later block's sampler reported
        int64_t cnt = 0;
        int st = 0;
        blas::check(sample(q, n, d, 0, state.counter.data(), state.key.data(), nullptr, nullptr, nullptr, &cnt, &st), "sample_indices_iid");
        r.w_status = st;
    }
    k = ell;
    return r;
}

}  // namespace _rpchol_impl

/// Rank-k approximation A ~ F F^T of the n x n PSD operator A, at most b pivots per block.  S (HOST, k entries) receives the pivots, F (DEVICE,
/// n x k, ld n) the factor; k returns the achieved rank.  Returns the advanced state.                                 rl_rpchol.hh:114-187
template <typename T, typename FUNC_T, typename STATE, typename CALLBACK>
STATE rp_cholesky(int64_t n, FUNC_T& A, int64_t& k, int64_t* S, T* F, int64_t b, STATE state, CALLBACK& cb) {
    const _rpchol_impl::Status r = _rpchol_impl::run(n, A, k, S, F, n, b, state);
    if (r.initial)
        throw Error("rp_cholesky: the diagonal is not a valid weight vector (weights_to_cdf status " + std::to_string(r.w_status) + ")");
    cb(k);
    return state;
}

template <typename T, typename FUNC_T, typename STATE>
STATE rp_cholesky(int64_t n, FUNC_T& A, int64_t& k, int64_t* S, T* F, int64_t b, STATE state) {
    auto cb = [](int64_t i) { return i; };
    return rp_cholesky(n, A, k, S, F, b, state, cb);
}

/// rp_cholesky, then V (DEVICE, n x k, ld n) <- the left singular vectors of F and eigvals (DEVICE, k) <- its squared singular values:
/// A ~ V diag(eigvals) V^T.                                                                                       rl_preconditioners.hh:348-361
template <typename T, typename STATE, typename FUNC>
STATE rpchol_pc_data(int64_t n, FUNC& A_stateless, int64_t& k, int64_t b, T* V, T* eigvals, STATE state) {
    std::vector<int64_t> selection((size_t)std::max<int64_t>(k, 1), -1);
    state = rp_cholesky(n, A_stateless, k, selection.data(), V, b, state);
    if (k == 0) return state;
    blas::Queue& q = A_stateless.q;
    blas::Scratch ws(q);
    T* U = ws.alloc<T>(n * k);
    T* VT = ws.alloc<T>(k * k);
    lapack::gesdd(Job::SomeVec, n, k, V, n, eigvals, U, n, VT, k, q);
    lapack::lacpy(MatrixType::General, n, k, U, n, V, n, q);
    std::vector<T> ev((size_t)k);
    blas::copy_to_host(k, eigvals, ev.data(), q);
    for (auto& e : ev) e = e * e;
    blas::copy_to_device(k, ev.data(), eigvals, q);
    q.sync();
    return state;
}

}  // namespace RandLAPACK
