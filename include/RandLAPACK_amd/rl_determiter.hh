// The deterministic iterative solvers on the device (RandLAPACK/comps/rl_determiter.hh): pcg_saddle (:18-134), and block / lockstep
// preconditioned conjugate gradients (:140-526): StatefulFrobeniusNorm, posm_square and pcg.
//
// pcg_saddle: the loop is the reference's, statement by statement (line numbers at the right), with these differences:
//   - every vector (b, c, resid_vec, x0, x, y) and both matrices are DEVICE arrays on q; alpha, beta and delta_1 never leave the device;
//   - one host read per iteration: the sizeof(T) bytes of resid_vec[iter], for the stop test delta_1 > (delta_1^0 tol) tol;
//   - the loop is written once, over an operator with the members matvec and normal_matvec (linops::DenseLinOp, linops::SparseLinOp); the
//     reference's pointer signature wraps its A in a DenseLinOp;
//   - q = A^T (A d) + delta d and d^T q come from the operator's normal_matvec (dense: rlhip_normal_matvec_*, one pass over A for n within
//     its limit; sparse: rlhip_csr_normal_matvec_*), A^T b and y = b - A x from its matvec, M^T r and M (.) from rlhip_gemv_*,
//     the n-length updates from rlhip_pcg_saddle_step_*;
//   - the residual refresh on iter % 25 == 1 runs the normal matvec on x;
//   - resid_vec must hold iter_lim + 1 entries: the reference writes resid_vec[iter] after the loop (:127), one past its documented
//     length (:28) when the limit is reached;
//   - a trailing `int64_t* iters` (optional) returns the number of iterations run.
// pcg_saddle_block (no counterpart in the reference): the same loop for s right-hand sides kept in lockstep over an operator with
// the members matmat and normal_matmat (linops::DenseLinOp): one normal product and two products with M per iteration for all columns,
// per-column scalars and stop flags on the device (rlhip_pcg_saddle_block_step_*), one host read of the s flags per iteration.
//
// pcg:
// Everything n x s and s x s lives in device memory on G.q; the loop is the reference's, statement by statement (line numbers at the right),
// with these differences:
//   - H, X and the block handed to `seminorm` are DEVICE arrays;
//   - posm_square runs the Cholesky attempt in one device kernel (rlhip_posm_square_*) and, when that reports a failed pivot, the reference's
//     eigenvalue fallback on the HOST (rl_determiter_host.hh: the product links no host LAPACK, and s <= 64 in practice).  LHS is not
//     destroyed.  In lockstep mode the kernel applies zero_off_diagonal to both of its operands itself, so RNR and ableft are never
//     rewritten on the device; the values that reach alpha and beta are the same;
//   - X += P alpha, R -= GP alpha and ||R|| are one kernel (rlhip_pcg_update_xr_*), P <- NR + P beta another (rlhip_pcg_update_p_*);
//   - when the seminorm is StatefulFrobeniusNorm<T>, the two norms of an iteration are taken from the squared column norms (sums in double,
//     fixed order) that the update kernel and the preconditioner return, and the beta solve is enqueued BEFORE the stop test so that its status
//     comes back with them: two host reads per iteration (the status of the alpha solve; the two norms + the status of the beta solve), and
//     s x s copies only when a Cholesky attempt fails.  What the speculative work overwrites (RNR, alpha, beta, ableft) is not read after a stop.
//     Any other callable is called as in the reference, after one more read per solve;
//   - a trailing `int64_t* iters` (optional) returns k, the number of iterations started.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <limits>
#include <type_traits>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_lapackpp.hh"
#include "rl_linops.hh"
#include "rl_determiter_host.hh"

namespace RandLAPACK {

namespace _saddle_impl {

inline int gemv(blas::Queue& q, Op t, int64_t m, int64_t n, double al, const double* A, int64_t lda, const double* x, double be, double* y) { return rlhip_gemv_f64(q.ctx(), (char)t, m, n, al, A, lda, x, be, y); }
inline int gemv(blas::Queue& q, Op t, int64_t m, int64_t n, float al, const float* A, int64_t lda, const float* x, float be, float* y) { return rlhip_gemv_f32(q.ctx(), (char)t, m, n, al, A, lda, x, be, y); }
inline int step_xr(blas::Queue& q, int64_t n, const double* d, const double* qv, const double* dq, const double* d1, double* x, double* r) { return rlhip_pcg_saddle_step_xr_f64(q.ctx(), n, d, qv, dq, d1, x, r); }
inline int step_xr(blas::Queue& q, int64_t n, const float* d, const float* qv, const float* dq, const float* d1, float* x, float* r) { return rlhip_pcg_saddle_step_xr_f32(q.ctx(), n, d, qv, dq, d1, x, r); }
inline int step_refresh(blas::Queue& q, int64_t n, const double* b1, const double* qx, double delta, const double* x, double* r) { return rlhip_pcg_saddle_step_refresh_f64(q.ctx(), n, b1, qx, delta, x, r); }
inline int step_refresh(blas::Queue& q, int64_t n, const float* b1, const float* qx, float delta, const float* x, float* r) { return rlhip_pcg_saddle_step_refresh_f32(q.ctx(), n, b1, qx, delta, x, r); }
inline int step_d(blas::Queue& q, int64_t n, const double* r, const double* s, const double* d1o, double* d1n, double* d) { return rlhip_pcg_saddle_step_d_f64(q.ctx(), n, r, s, d1o, d1n, d); }
inline int step_d(blas::Queue& q, int64_t n, const float* r, const float* s, const float* d1o, float* d1n, float* d) { return rlhip_pcg_saddle_step_d_f32(q.ctx(), n, r, s, d1o, d1n, d); }
inline int axpby(blas::Queue& q, int64_t n, double a, const double* x, double b, double* y) { return rlhip_axpby_f64(q.ctx(), n, a, x, b, y); }
inline int axpby(blas::Queue& q, int64_t n, float a, const float* x, float b, float* y) { return rlhip_axpby_f32(q.ctx(), n, a, x, b, y); }
// the same three steps on n x s blocks in lockstep (rlhip_pcg_saddle_block_step_*)
inline int block_step_xr(blas::Queue& q, int64_t n, int64_t s, const double* D, int64_t ldd, const double* Q, int64_t ldq, const double* dq, const double* d1, int64_t ldh, double* X, int64_t ldx, double* R, int64_t ldr, const int* act) { return rlhip_pcg_saddle_block_step_xr_f64(q.ctx(), n, s, D, ldd, Q, ldq, dq, d1, ldh, X, ldx, R, ldr, act); }
inline int block_step_xr(blas::Queue& q, int64_t n, int64_t s, const float* D, int64_t ldd, const float* Q, int64_t ldq, const float* dq, const float* d1, int64_t ldh, float* X, int64_t ldx, float* R, int64_t ldr, const int* act) { return rlhip_pcg_saddle_block_step_xr_f32(q.ctx(), n, s, D, ldd, Q, ldq, dq, d1, ldh, X, ldx, R, ldr, act); }
inline int block_step_refresh(blas::Queue& q, int64_t n, int64_t s, const double* B1, int64_t ldb1, const double* QX, int64_t ldqx, double delta, const double* X, int64_t ldx, double* R, int64_t ldr, const int* act) { return rlhip_pcg_saddle_block_step_refresh_f64(q.ctx(), n, s, B1, ldb1, QX, ldqx, delta, X, ldx, R, ldr, act); }
inline int block_step_refresh(blas::Queue& q, int64_t n, int64_t s, const float* B1, int64_t ldb1, const float* QX, int64_t ldqx, float delta, const float* X, int64_t ldx, float* R, int64_t ldr, const int* act) { return rlhip_pcg_saddle_block_step_refresh_f32(q.ctx(), n, s, B1, ldb1, QX, ldqx, delta, X, ldx, R, ldr, act); }
inline int block_step_d(blas::Queue& q, int64_t n, int64_t s, const double* R, int64_t ldr, const double* S, int64_t lds, const double* d1o, double* d1n, int64_t ldh, double* D, int64_t ldd, double tol, double* rel, int* act) { return rlhip_pcg_saddle_block_step_d_f64(q.ctx(), n, s, R, ldr, S, lds, d1o, d1n, ldh, D, ldd, tol, rel, act); }
inline int block_step_d(blas::Queue& q, int64_t n, int64_t s, const float* R, int64_t ldr, const float* S, int64_t lds, const float* d1o, float* d1n, int64_t ldh, float* D, int64_t ldd, float tol, float* rel, int* act) { return rlhip_pcg_saddle_block_step_d_f32(q.ctx(), n, s, R, ldr, S, lds, d1o, d1n, ldh, D, ldd, tol, rel, act); }

}  // namespace _saddle_impl

/// Solves the saddle point problem (A'A + delta I) x = A'b - c by conjugate gradients preconditioned with M M' (M: n x k, ldm), then
/// y = b - A x.  A: m x n (lda); b, y: m; c, x0, x: n; resid_vec: iter_lim + 1 -- all DEVICE, column-major.  resid_vec[i] receives
/// delta_1 = r' M M' r at the start of iteration i and, after the loop, of the iteration that was not run; iterations stop when
/// delta_1 <= (delta_1^0 tol) tol or after iter_lim.                                                                rl_determiter.hh:18-134
/// The loop is written once, over an operator: A is anything with n_rows, n_cols, the queue q and the two members
/// matvec(trans, alpha, x, beta, y) and normal_matvec(d, delta, q, t, dq) -- linops::DenseLinOp and linops::SparseLinOp (rl_linops.hh).
template <typename T, typename LinOp>
void pcg_saddle(LinOp& A, const T* b, const T* c, T delta, int64_t iter_lim, T* resid_vec, T tol, int64_t k, const T* M, int64_t ldm, const T* x0, T* x,
                T* y, int64_t* iters = nullptr) {
    namespace si = _saddle_impl;
    const int64_t m = A.n_rows, n = A.n_cols;
    blas::Queue& q = A.q;
    randlapack_require(m >= 1 && n >= 1 && k >= 1) << "pcg_saddle needs m=" << m << ", n=" << n << ", k=" << k << " >= 1";
    randlapack_require(iter_lim >= 0) << "iter_lim=" << iter_lim << " must be >= 0";
    if (iters) *iters = 0;

    blas::Scratch ws(q);                                                                                                            // :38-46
    T* allwork = ws.alloc<T>(m + 5 * n + k + 1);
    T* out_a1 = allwork;
    T* out_at1 = out_a1 + m;
    T* r = out_at1 + n;
    T* d = r + n;
    T* b1 = d + n;
    T* out_m1 = b1 + n;
    T* out_mt1 = out_m1 + n;
    T* dq = out_mt1 + k;                                                         // d' q of the current iteration

    //  b1 = A'b - c
    blas::copy(n, c, 1, b1, 1, q);                                                                                                  // :49
    A.matvec(Op::Trans, (T)1.0, b, (T)-1.0, b1);                                                                                    // :50

    // r = b1 - (A'(A x0) + delta x0)
    blas::copy(n, b1, 1, r, 1, q);                                                                                                  // :57
    A.normal_matvec(x0, delta, out_at1, (T*)nullptr, (T*)nullptr);                                                                  // :58-60
    blas::check(si::axpby(q, n, (T)-1.0, out_at1, (T)1.0, r), "axpby");                                                             // :61

    // d = M (M' r)
    blas::check(si::gemv(q, Op::Trans, n, k, (T)1.0, M, ldm, r, (T)0.0, out_mt1), "gemv");                                          // :64
    blas::check(si::gemv(q, Op::NoTrans, n, k, (T)1.0, M, ldm, out_mt1, (T)0.0, d), "gemv");                                        // :65

    blas::copy(n, x0, 1, x, 1, q);                                                                                                  // :68
    blas::check(si::step_d(q, n, r, d, (const T*)nullptr, resid_vec, (T*)nullptr), "pcg_saddle_step_d");   // resid_vec[0] = d' r       :69
    T delta1_new = 0;
    blas::copy_to_host(1, resid_vec, &delta1_new, q);
    T rel_sq_tol = (delta1_new * tol) * tol;                                                                                        // :71

    int64_t iter = 0;
    while (iter < iter_lim && delta1_new > rel_sq_tol) {                                                                            // :76
        // (resid_vec[iter] = delta1_new: written by the step that computed it)                                                     :77
        // q = A'(A d) + delta d, and d' q
        A.normal_matvec(d, delta, out_at1, (T*)nullptr, dq);                                                                        // :81-83, 86
        const bool refresh = iter % 25 == 1;                                                                                        // :92
        // alpha = delta1_new / (d' q); x += alpha d; r -= alpha q unless r is recomputed
        blas::check(si::step_xr(q, n, d, refresh ? (const T*)nullptr : out_at1, dq, resid_vec + iter, x, r), "pcg_saddle_step_xr"); // :86, 89, 106
        if (refresh) {
            // r = b1 - (A'(A x) + delta x)
            A.normal_matvec(x, (T)0.0, out_at1, (T*)nullptr, (T*)nullptr);                                                          // :99-100
            blas::check(si::step_refresh(q, n, b1, out_at1, delta, x, r), "pcg_saddle_step_refresh");                               // :101-103
        }
        // s = M (M' r)
        blas::check(si::gemv(q, Op::Trans, n, k, (T)1.0, M, ldm, r, (T)0.0, out_mt1), "gemv");                                      // :113
        blas::check(si::gemv(q, Op::NoTrans, n, k, (T)1.0, M, ldm, out_mt1, (T)0.0, out_m1), "gemv");                               // :114
        // scalars and update d: resid_vec[iter + 1] = r' s, beta = that / resid_vec[iter], d = beta d + s
        blas::check(si::step_d(q, n, r, out_m1, resid_vec + iter, resid_vec + iter + 1, d), "pcg_saddle_step_d");                   // :117-122
        ++iter;                                                                                                                     // :124
        blas::copy_to_host(1, resid_vec + iter, &delta1_new, q);                 // the iteration's one host read
    }
    // (resid_vec[iter] = delta1_new, :127: already there)
    if (iters) *iters = iter;

    // recover y = b - Ax
    blas::copy(m, b, 1, y, 1, q);                                                                                                   // :130
    A.matvec(Op::NoTrans, (T)-1.0, x, (T)1.0, y);                                                                                   // :131
    q.sync();                                    // (the work space goes back to the arena)
}

/// The same for a dense column-major A (m x n, lda, DEVICE): the reference's signature.
template <typename T>
void pcg_saddle(int64_t m, int64_t n, const T* A, int64_t lda, const T* b, const T* c, T delta, int64_t iter_lim, T* resid_vec, T tol, int64_t k,
                const T* M, int64_t ldm, const T* x0, T* x, T* y, blas::Queue& q = blas::default_queue(), int64_t* iters = nullptr) {
    randlapack_require(m >= 1 && n >= 1 && k >= 1) << "pcg_saddle needs m=" << m << ", n=" << n << ", k=" << k << " >= 1";
    linops::DenseLinOp<T> op(m, n, A, lda, Layout::ColMajor, q);
    pcg_saddle(op, b, c, delta, iter_lim, resid_vec, tol, k, M, ldm, x0, x, y, iters);
}

/// pcg_saddle for s right-hand sides in lockstep: column j runs exactly the recurrence of pcg_saddle on (b_j, c_j, x0_j) --
/// the residual refresh on iter % 25 == 1 and the stop test delta_1j > (delta_1j^0 tol) tol included -- while all columns share each
/// iteration's one normal product (A.normal_matmat: A is read once per chunk of columns on its one-pass route) and its two products with M.
/// B: m x s (ldb); C: n x s (ldc; NULL: zero); resid: (iter_lim + 1) x s (ldr >= iter_lim + 1); M: n x k (ldm); X0: n x s (ldx0; NULL:
/// zero); X: n x s (ldx); Y: m x s (ldy) -- all DEVICE, column-major.  iters: HOST, s entries, may be NULL.
/// The loop runs while iter < iter_lim and some column is active.  A column that has met its stop test is frozen: its x_j, r_j and d_j no
/// longer change, iters[j] is the number of iterations it ran, resid[0 .. iters[j], j] are written and the entries below them are left
/// as they were.  A column whose delta_1j^0 is zero (a zero right-hand side) or NaN never starts: x_j = x0_j, iters[j] = 0.  At the end
/// Y = B - A X for every column.  alpha_j, beta_j, delta_1j, d_j' q_j and rel_sq_tol_j never leave the device; the one host read of an
/// iteration is that of the s flags active_j.
/// A is anything with n_rows, n_cols, q and the two members matmat(trans, s, alpha, X, ldx, beta, Y, ldy) and
/// normal_matmat(s, D, ldd, delta, Q, ldq, T, ldt, dq): linops::DenseLinOp (rl_linops.hh).
template <typename T, typename LinOp>
void pcg_saddle_block(LinOp& A, int64_t s, const T* B, int64_t ldb, const T* C, int64_t ldc, T delta, int64_t iter_lim, T* resid, int64_t ldr, T tol,
                      int64_t k, const T* M, int64_t ldm, const T* X0, int64_t ldx0, T* X, int64_t ldx, T* Y, int64_t ldy, int64_t* iters = nullptr) {
    namespace si = _saddle_impl;
    const int64_t m = A.n_rows, n = A.n_cols;
    blas::Queue& q = A.q;
    const auto gen = lapack::MatrixType::General;
    const auto layout = Layout::ColMajor;
    randlapack_require(m >= 1 && n >= 1 && k >= 1) << "pcg_saddle_block needs m=" << m << ", n=" << n << ", k=" << k << " >= 1";
    randlapack_require(s >= 0 && s <= 65535) << "s=" << s << " must lie in [0, 65535]";
    randlapack_require(iter_lim >= 0) << "iter_lim=" << iter_lim << " must be >= 0";
    randlapack_require(ldb >= m && ldy >= m && ldx >= n && ldm >= n && (!C || ldc >= n) && (!X0 || ldx0 >= n))
        << "pcg_saddle_block: a leading dimension is below its row count";
    randlapack_require(ldr >= iter_lim + 1) << "ldr=" << ldr << " must be >= iter_lim + 1 = " << iter_lim + 1;
    if (s == 0) return;
    std::vector<int64_t> its((size_t)s, 0);
    if (iters) std::copy(its.begin(), its.end(), iters);

    blas::Scratch ws(q);
    T* allwork = ws.alloc<T>(5 * n * s + k * s + 2 * s);
    T* out_at1 = allwork;                        // n x s: the normal product
    T* R = out_at1 + n * s;
    T* D = R + n * s;
    T* B1 = D + n * s;
    T* out_m1 = B1 + n * s;
    T* out_mt1 = out_m1 + n * s;                 // k x s
    T* dq = out_mt1 + k * s;                     // d_j' q_j of the current iteration
    T* rel_sq_tol = dq + s;
    int* active = ws.alloc<int>(s);
    std::vector<int> act((size_t)s, 0);

    // B1 = A'B - C
    if (C) {
        lapack::lacpy(gen, n, s, C, ldc, B1, n, q);
        A.matmat(Op::Trans, s, (T)1.0, B, ldb, (T)-1.0, B1, n);
    } else {
        A.matmat(Op::Trans, s, (T)1.0, B, ldb, (T)0.0, B1, n);
    }
    if (X0) lapack::lacpy(gen, n, s, X0, ldx0, X, ldx, q);
    else lapack::laset(gen, n, s, (T)0.0, (T)0.0, X, ldx, q);
    // R = B1 - (A'(A X0) + delta X0)
    blas::device_copy_vector(n * s, B1, R, q);
    A.normal_matmat(s, X, ldx, delta, out_at1, n, (T*)nullptr, 0, (T*)nullptr);
    blas::check(si::axpby(q, n * s, (T)-1.0, out_at1, (T)1.0, R), "axpby");
    // D = M (M' R)
    blas::gemm(layout, Op::Trans, Op::NoTrans, k, s, n, (T)1.0, M, ldm, R, n, (T)0.0, out_mt1, k, q);
    blas::gemm(layout, Op::NoTrans, Op::NoTrans, n, s, k, (T)1.0, M, ldm, out_mt1, k, (T)0.0, D, n, q);
    // resid[0, j] = d_j' r_j, rel_sq_tol_j and active_j
    blas::check(si::block_step_d(q, n, s, R, n, D, n, (const T*)nullptr, resid, ldr, (T*)nullptr, n, tol, rel_sq_tol, active), "pcg_saddle_block_step_d");
    blas::copy_to_host(s, active, act.data(), q);

    int64_t iter = 0;
    auto any_active = [&] {
        for (int a : act)
            if (a) return true;
        return false;
    };
    while (iter < iter_lim && any_active()) {
        for (int64_t j = 0; j < s; ++j) its[j] += act[j] ? 1 : 0;
        // Q = A'(A D) + delta D, and d_j' q_j
        A.normal_matmat(s, D, n, delta, out_at1, n, (T*)nullptr, 0, dq);
        const bool refresh = iter % 25 == 1;
        blas::check(si::block_step_xr(q, n, s, D, n, refresh ? (const T*)nullptr : out_at1, n, dq, resid + iter, ldr, X, ldx, R, n, active),
                    "pcg_saddle_block_step_xr");
        if (refresh) {
            A.normal_matmat(s, X, ldx, (T)0.0, out_at1, n, (T*)nullptr, 0, (T*)nullptr);
            blas::check(si::block_step_refresh(q, n, s, B1, n, out_at1, n, delta, X, ldx, R, n, active), "pcg_saddle_block_step_refresh");
        }
        // S = M (M' R)
        blas::gemm(layout, Op::Trans, Op::NoTrans, k, s, n, (T)1.0, M, ldm, R, n, (T)0.0, out_mt1, k, q);
        blas::gemm(layout, Op::NoTrans, Op::NoTrans, n, s, k, (T)1.0, M, ldm, out_mt1, k, (T)0.0, out_m1, n, q);
        blas::check(si::block_step_d(q, n, s, R, n, out_m1, n, resid + iter, resid + iter + 1, ldr, D, n, tol, rel_sq_tol, active), "pcg_saddle_block_step_d");
        ++iter;
        blas::copy_to_host(s, active, act.data(), q);                            // the iteration's one host read
    }
    if (iters) std::copy(its.begin(), its.end(), iters);

    // Y = B - A X
    lapack::lacpy(gen, m, s, B, ldb, Y, ldy, q);
    A.matmat(Op::NoTrans, s, (T)-1.0, X, ldx, (T)1.0, Y, ldy);
    q.sync();                                    // (the work space goes back to the arena)
}

/// The same for a dense column-major A (m x n, lda, DEVICE).
template <typename T>
void pcg_saddle_block(int64_t m, int64_t n, const T* A, int64_t lda, int64_t s, const T* B, int64_t ldb, const T* C, int64_t ldc, T delta, int64_t iter_lim,
                      T* resid, int64_t ldr, T tol, int64_t k, const T* M, int64_t ldm, const T* X0, int64_t ldx0, T* X, int64_t ldx, T* Y, int64_t ldy,
                      blas::Queue& q = blas::default_queue(), int64_t* iters = nullptr) {
    randlapack_require(m >= 1 && n >= 1 && k >= 1) << "pcg_saddle_block needs m=" << m << ", n=" << n << ", k=" << k << " >= 1";
    linops::DenseLinOp<T> op(m, n, A, lda, Layout::ColMajor, q);
    pcg_saddle_block(op, s, B, ldb, C, ldc, delta, iter_lim, resid, ldr, tol, k, M, ldm, X0, ldx0, X, ldx, Y, ldy, iters);
}

/// The Frobenius norm of a DEVICE block, every value kept (rl_determiter.hh:139-151).  pcg recognises this type and fills `history` from the
/// sums its kernels return instead of calling it.
template <typename T>
struct StatefulFrobeniusNorm {
    std::vector<T> history;
    blas::Queue* q = nullptr;              // the queue operator() reads through; null: the default queue
    StatefulFrobeniusNorm() : history() {}
    explicit StatefulFrobeniusNorm(blas::Queue& queue) : history(), q(&queue) {}
    StatefulFrobeniusNorm(StatefulFrobeniusNorm<T>&& other) noexcept : history(std::move(other.history)), q(other.q) {}
    inline T operator()(int64_t n, int64_t s, const T* NR) {
        const T nrm = lapack::lange(Norm::Fro, n, s, NR, n > 0 ? n : 1, q ? *q : blas::default_queue());
        this->history.push_back(nrm);
        return nrm;
    }
};

namespace _pcg_impl {

inline int posm_enqueue(blas::Queue& q, int64_t s, const double* L, double* R, int diag_only, int64_t* st) { return rlhip_posm_square_f64(q.ctx(), s, L, R, diag_only, st); }
inline int posm_enqueue(blas::Queue& q, int64_t s, const float* L, float* R, int diag_only, int64_t* st) { return rlhip_posm_square_f32(q.ctx(), s, L, R, diag_only, st); }
inline int update_xr(blas::Queue& q, int64_t n, int64_t s, const double* a, const double* P, const double* GP, double* X, double* R, double* cn) {
    return rlhip_pcg_update_xr_f64(q.ctx(), n, s, a, P, n, GP, n, X, n, R, n, cn);
}
inline int update_xr(blas::Queue& q, int64_t n, int64_t s, const float* a, const float* P, const float* GP, float* X, float* R, double* cn) {
    return rlhip_pcg_update_xr_f32(q.ctx(), n, s, a, P, n, GP, n, X, n, R, n, cn);
}
inline int update_p(blas::Queue& q, int64_t n, int64_t s, const double* b, const double* NR, double* P) { return rlhip_pcg_update_p_f64(q.ctx(), n, s, b, NR, n, P, n); }
inline int update_p(blas::Queue& q, int64_t n, int64_t s, const float* b, const float* NR, float* P) { return rlhip_pcg_update_p_f32(q.ctx(), n, s, b, NR, n, P, n); }
inline int colnorm2(blas::Queue& q, int64_t n, int64_t s, const double* A, double* cn) { return rlhip_pcg_colnorm2_f64(q.ctx(), n, s, A, n, cn); }
inline int colnorm2(blas::Queue& q, int64_t n, int64_t s, const float* A, double* cn) { return rlhip_pcg_colnorm2_f32(q.ctx(), n, s, A, n, cn); }
inline int axpby(blas::Queue& q, int64_t n, double a, const double* x, double b, double* y) { return rlhip_axpby_f64(q.ctx(), n, a, x, b, y); }
inline int axpby(blas::Queue& q, int64_t n, float a, const float* x, float b, float* y) { return rlhip_axpby_f32(q.ctx(), n, a, x, b, y); }

// N(R) -> C with the squared column norms of C: the preconditioner's own fused form when it has one, a pass over C otherwise
template <typename FN, typename T, typename = void>
struct has_apply_norms : std::false_type {};
template <typename FN, typename T>
struct has_apply_norms<FN, T, std::void_t<decltype(std::declval<FN&>().apply(Layout::ColMajor, int64_t(0), T(1), (const T*)nullptr, int64_t(0), T(0), (T*)nullptr,
                                                                            int64_t(0), (double*)nullptr))>> : std::true_type {};
template <typename T, typename FN>
void apply_with_norms(FN& N, blas::Queue& q, int64_t n, int64_t s, T* R, T* C, double* cn) {
    if constexpr (has_apply_norms<FN, T>::value) {
        N.apply(Layout::ColMajor, s, (T)1.0, R, n, (T)0.0, C, n, cn);
    } else {
        N(Layout::ColMajor, s, (T)1.0, R, n, (T)0.0, C, n);
        blas::check(colnorm2(q, n, s, C, cn), "pcg_colnorm2");
    }
}

inline double root_of_sum(const double* cn, int64_t s) {
    double t = 0;
    for (int64_t j = 0; j < s; ++j) t += cn[j];
    return std::sqrt(t);
}

/// what posm_square does once the status of the device attempt is known: s on success; on -1 the s x s pair comes down, the fallback
/// (rl_determiter.hh:258-281) runs on the host and, if it produced a solution, RHS goes back up
template <typename T>
int64_t posm_finish(int64_t s, const T* LHS, T* RHS, bool diag_only, int64_t status, blas::Queue& q) {
    if (status >= 0) return status;
    const int64_t ss = s * s;
    std::vector<T> L((size_t)ss), B((size_t)ss), work((size_t)ss);
    blas::copy_to_host(ss, LHS, L.data(), q);
    blas::copy_to_host(ss, RHS, B.data(), q);
    if (diag_only) {
        zero_off_diagonal(L.data(), s);
        zero_off_diagonal(B.data(), s);
    }
    const int64_t r = posm_square_fallback(s, L.data(), B.data(), work.data());
    if (r >= 0) blas::copy_to_device(ss, B.data(), RHS, q);
    return r;
}

}  // namespace _pcg_impl

/// RHS <- pinv(LHS) RHS for the PSD s x s matrix LHS (DEVICE, ld s, lower triangle read, left as it is; RHS DEVICE, ld s).  `work`: DEVICE,
/// at least s * s entries and at least 8 bytes, 8-byte aligned (its first word receives the kernel's status).  Returns rank(LHS), or
/// -(s + 1) when LHS is not positive semidefinite, -(s + 2) when it is zero up to rounding.                      rl_determiter.hh:231-282
/// diag_only: the lockstep form, zero_off_diagonal applied to both matrices first.
template <typename T>
int64_t posm_square(int64_t s, const T* LHS, T* RHS, T* work, blas::Queue& q = blas::default_queue(), bool diag_only = false) {
    int64_t* st = reinterpret_cast<int64_t*>(work);
    blas::check(_pcg_impl::posm_enqueue(q, s, LHS, RHS, diag_only ? 1 : 0, st), "posm_square");
    int64_t status = 0;
    blas::copy_to_host(1, st, &status, q);
    return _pcg_impl::posm_finish(s, LHS, RHS, diag_only, status, q);
}

/// Solves G_i x_i = h_i, i = 1..s, with preconditioners N_i.  G.num_ops == 1: block PCG with block size s; G.num_ops == s: s single-vector
/// iterations kept in lockstep.  G and N are called as G(Layout::ColMajor, s, alpha, B, ldb, beta, C, ldc) on DEVICE blocks; G.dim, G.num_ops
/// and G.q (the queue everything runs on) are read.  H (in) and X (in: the starting point, out: the solution) are DEVICE dim x s arrays with
/// stride dim.  seminorm(dim, s, R_dev) is called on the residual (even calls) and the preconditioned residual (odd calls); iterations stop
/// when normNR < tol (1 + normNR0) or after max_iters.                                                           rl_determiter.hh:371-493
template <typename T, typename FG, typename FSeminorm, typename FN>
void pcg(FG& G, const T* H, int64_t s, FSeminorm& seminorm, T tol, int64_t max_iters, FN& N, T* X, bool verbose, int64_t* iters = nullptr) {
    constexpr bool fused_norms = std::is_same_v<FSeminorm, StatefulFrobeniusNorm<T>>;
    int64_t n = G.dim;                                                                                                              // :383
    int64_t ns = n * s;
    int64_t ss = s * s;
    bool treat_as_separable = G.num_ops > 1;                                                                                        // :386
    if (treat_as_separable) { randlapack_require(s == G.num_ops) << "with separable treatment, s=" << s << " must equal G.num_ops=" << G.num_ops; }
    randlapack_require(s >= 1 && n >= 1) << "pcg needs s=" << s << " >= 1 and dim=" << n << " >= 1";
    blas::Queue& q = G.q;
    if (iters) *iters = 0;

    // all work space is zero-initialised; only R is overwritten                                                                    :389-403
    blas::Scratch ws(q);
    T* allwork = ws.alloc<T>(4 * ns + 4 * ss);
    blas::device_memset(allwork, 0, 4 * ns + 4 * ss, q);
    T* R = allwork;
    blas::device_copy_vector(ns, H, R, q);
    T* P = R + ns;
    T* GP = P + ns;
    T* NR = GP + ns;
    T* RNR = NR + ns;
    T* alpha = RNR + ss;
    T* beta = alpha + ss;
    T* ableft = beta + ss;                       // (the reference's `scratch` block backs up LHS for its potrf; the kernel leaves LHS alone)
    // what comes back from the device: the status words of the two solves, then the squared column norms of R and of N R
    int64_t* mail = ws.alloc<int64_t>(2 + 2 * s);
    double* cnR = reinterpret_cast<double*>(mail + 2);
    double* cnNR = cnR + s;
    std::vector<int64_t> mail_host((size_t)(2 + 2 * s));
    const double* cnR_host = reinterpret_cast<const double*>(mail_host.data() + 2);
    const double* cnNR_host = cnR_host + s;
    const int diag_only = treat_as_separable ? 1 : 0;

    T normNR = INFINITY;                                                                                                            // :405
    auto layout = Layout::ColMajor;

    G(layout, s, (T)1.0, X, n, (T)0.0, GP, n);                                           // GP <- G X                               :410
    blas::check(_pcg_impl::axpby(q, ns, (T)-1.0, GP, (T)1.0, R), "axpby");               // R <- R - GP                             :412
    if constexpr (fused_norms) {
        blas::check(_pcg_impl::colnorm2(q, n, s, R, cnR), "pcg_colnorm2");
        _pcg_impl::apply_with_norms<T>(N, q, n, s, R, P, cnNR);                          // P <- N R                                :414
    } else {
        N(layout, s, (T)1.0, R, n, (T)0.0, P, n);
    }
    blas::gemm(layout, Op::Trans, Op::NoTrans, s, s, n, (T)1.0, R, n, P, n, (T)0.0, RNR, s, q);   // RNR <- R^T N R                 :416
    // (zero_off_diagonal(RNR), :418: applied by the solve kernel to its operands)
    blas::device_copy_vector(ss, RNR, alpha, q);                                         // alpha <- RNR                            :420

    int64_t k = 0;
    T normR0, normNR0;
    if constexpr (fused_norms) {
        blas::copy_to_host(2 + 2 * s, mail, mail_host.data(), q);
        normR0 = (T)_pcg_impl::root_of_sum(cnR_host, s);                                                                            // :424-425
        normNR0 = (T)_pcg_impl::root_of_sum(cnNR_host, s);
        seminorm.history.push_back(normR0);
        seminorm.history.push_back(normNR0);
    } else {
        normR0 = seminorm(n, s, R);
        normNR0 = seminorm(n, s, P);
    }
    T stop_abstol = tol * ((T)1.0 + normNR0);                                                                                       // :426
    int64_t subspace_dim = 0;
    if (verbose) std::cout << "normNR : " << normNR0 << "\tnormR : " << normR0 << "\tk: 0\tdim : 0\n";
    while (subspace_dim < n && k < max_iters) {                                                                                     // :430
        k++;
        if (iters) *iters = k;
        G(layout, s, (T)1.0, P, n, (T)0.0, GP, n);                                       // GP <- G P                               :436
        blas::gemm(layout, Op::Trans, Op::NoTrans, s, s, n, (T)1.0, P, n, GP, n, (T)0.0, ableft, s, q);   // ableft <- P^T G P      :438
        blas::check(_pcg_impl::posm_enqueue(q, s, ableft, alpha, diag_only, mail), "posm_square");   // alpha <- ableft^-1 alpha    :440-441
        blas::copy_to_host(1, mail, mail_host.data(), q);
        int64_t subspace_incr = _pcg_impl::posm_finish(s, ableft, alpha, treat_as_separable, mail_host[0], q);
        if (treat_as_separable && subspace_incr > 0) subspace_incr = 1;                                                             // :443-444
        if (subspace_incr < -((int64_t)s)) break;                                                                                   // :446-447
        subspace_dim = subspace_dim + subspace_incr;

        T normR;
        if constexpr (fused_norms) {
            blas::check(_pcg_impl::update_xr(q, n, s, alpha, P, GP, X, R, cnR), "pcg_update_xr");   // X += P alpha, R -= GP alpha  :450-453
            _pcg_impl::apply_with_norms<T>(N, q, n, s, R, NR, cnNR);                     // NR <- N R                               :462
            // enqueued ahead of the stop test, so that one read brings the norms and the status of the beta solve
            blas::device_copy_vector(ss, RNR, ableft, q);                                // ableft <- RNR                           :472
            blas::gemm(layout, Op::Trans, Op::NoTrans, s, s, n, (T)1.0, R, n, NR, n, (T)0.0, RNR, s, q);   // RNR <- R^T NR         :474
            blas::device_copy_vector(ss, RNR, alpha, q);                                 // alpha <- RNR                            :477
            blas::device_copy_vector(ss, alpha, beta, q);                                // beta <- alpha                           :479
            blas::check(_pcg_impl::posm_enqueue(q, s, ableft, beta, diag_only, mail + 1), "posm_square");   //                      :481
            blas::copy_to_host(1 + 2 * s, mail + 1, mail_host.data() + 1, q);
            normR = (T)_pcg_impl::root_of_sum(cnR_host, s);                                                                         // :460
            normNR = (T)_pcg_impl::root_of_sum(cnNR_host, s);                                                                       // :464
            seminorm.history.push_back(normR);
            seminorm.history.push_back(normNR);
        } else {
            blas::check(_pcg_impl::update_xr(q, n, s, alpha, P, GP, X, R, (double*)nullptr), "pcg_update_xr");
            normR = seminorm(n, s, R);                                                                                              // :460
            N(layout, s, (T)1.0, R, n, (T)0.0, NR, n);                                                                              // :462
            normNR = seminorm(n, s, NR);                                                                                            // :464
        }
        if (verbose) std::cout << "normNR : " << normNR << "\tnormR : " << normR << "\tk: " << k << "\tdim : " << subspace_dim << '\n';
        if (normNR < stop_abstol) break;                                                                                            // :467-468
        int64_t err;
        if constexpr (fused_norms) {
            err = _pcg_impl::posm_finish(s, ableft, beta, treat_as_separable, mail_host[1], q);   // beta <- ableft^-1 beta         :481
        } else {
            blas::device_copy_vector(ss, RNR, ableft, q);                                                                           // :472
            blas::gemm(layout, Op::Trans, Op::NoTrans, s, s, n, (T)1.0, R, n, NR, n, (T)0.0, RNR, s, q);                            // :474
            blas::device_copy_vector(ss, RNR, alpha, q);                                                                            // :477
            blas::device_copy_vector(ss, alpha, beta, q);                                                                           // :479
            blas::check(_pcg_impl::posm_enqueue(q, s, ableft, beta, diag_only, mail + 1), "posm_square");                           // :481
            blas::copy_to_host(1, mail + 1, mail_host.data() + 1, q);
            err = _pcg_impl::posm_finish(s, ableft, beta, treat_as_separable, mail_host[1], q);
        }
        if (err < -((int64_t)s)) break;                                                                                             // :483-484
        blas::check(_pcg_impl::update_p(q, n, s, beta, NR, P), "pcg_update_p");          // P <- NR + P beta                        :485-488
    }
    q.sync();                                    // (the work space goes back to the arena)
}

/// The reference's std::vector wrapper (:512-526) for HOST vectors: H and X go to the device, the solution comes back into X.
template <typename T, typename FG, typename FN, typename FSeminorm = StatefulFrobeniusNorm<T>>
FSeminorm pcg(FG& G, const std::vector<T>& H, T tol, int64_t max_iters, FN& N, std::vector<T>& X, bool verbose) {
    FSeminorm seminorm{};
    int64_t s = ((int64_t)H.size()) / G.dim;
    blas::Queue& q = G.q;
    blas::Scratch ws(q);
    T* Hd = ws.alloc<T>(G.dim * s);
    T* Xd = ws.alloc<T>(G.dim * s);
    blas::copy_to_device(G.dim * s, H.data(), Hd, q);
    blas::copy_to_device(G.dim * s, X.data(), Xd, q);
    pcg(G, (const T*)Hd, s, seminorm, tol, max_iters, N, Xd, verbose);
    blas::copy_to_host(G.dim * s, Xd, X.data(), q);
    return seminorm;
}

}  // namespace RandLAPACK
