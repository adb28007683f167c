/* rlhip_drivers.h -- C entry points of the driver/comp objects (include/RandLAPACK_amd/), for bindings that
 * cannot instantiate C++ templates (ctypes in tests/bench, or a C caller).  Each function builds the same
 * object graph a RandLAPACK user builds (Stabilization -> RS -> RF -> QB -> RSVD) and invokes
 * call().  All matrices are DEVICE pointers, column-major.
 *
 * state[6] = RNGState: counter[0..3], key[0..1]; advanced in place exactly as the reference threads it
 * (`state = fill_dense(D, buf, state)`, comps/rl_rs.hh:135).
 * stab kinds: 0 = CholQRQ, 1 = HQRQ, 2 = PLUL (comps/rl_orth.hh:26-65,101-141,167-207).
 * Return codes are the reference's (RS 0/1, RF 0/1/2, QB 0/2/3/4/5/6, RSVD 0); -100 = RandLAPACK::Error
 * (bad argument), -101 = device/runtime failure; rlhip_last_error() gives the message.
 */
#ifndef RLHIP_DRIVERS_H
#define RLHIP_DRIVERS_H
#include "rlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* rlhip_last_error(void);

/* Stabilization<double>::call(m, k, A)                                   comps/rl_orth.hh:69-98 */
int rlhip_drv_stab_f64(rlhip_ctx* ctx, int kind, int cond_check, int64_t m, int64_t k, double* A, int* chol_fail);
/* RS<double>::call -> Omega (n x k, caller allocated)                    comps/rl_rs.hh:117-178 */
int rlhip_drv_rs_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t k, int64_t p, int64_t q,
                     int stab_kind, double* Omega, uint32_t state[6]);
/* RF<double>::call -> Q (m x k, caller allocated)                        comps/rl_rf.hh:107-137 */
int rlhip_drv_rf_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t k, int64_t p, int64_t q,
                     int rs_stab, int orth_kind, double* Q, uint32_t state[6]);
/* QB<double>::call; *Q (m x k) and *BT (n x k) are allocated by the callee, free with rlhip_free.
 *                                                                         comps/rl_qb.hh:134-268 */
int rlhip_drv_qb_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t* k, int64_t b_sz, double tol,
                     int64_t p, int64_t q, int rs_stab, int rf_orth, int qb_orth, int orth_check, double** Q,
                     double** BT, uint32_t state[6]);
/* RSVD<double>::call; *U (m x k), *S (k), *V (n x k) allocated by the callee, free with rlhip_free.
 * *qb_ret receives QB's return code.                                      drivers/rl_rsvd.hh:114-154 */
int rlhip_drv_rsvd_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t* k, int64_t b_sz, double tol,
                       int64_t p, int64_t q, int rs_stab, int rf_orth, int qb_orth, int orth_check, double** U,
                       double** S, double** V, uint32_t state[6], int* qb_ret);

/* CQRRPT<double>::call; qrcp {0 hqrrp, 1 bqrrp, 2 geqp3} in the reference's enum order (rl_cqrrpt.hh:41), -1 = default (geqp3); add 16 for
 * CQRRPT::orthogonalization = true (the trailing n - rank columns of A become an orthonormal completion, R is left as R_chol; :347-367).  A (m x n, lda) -> Q; R (n x n, ldr); J (n, device int64).  If A_hat_in
 * is non-NULL it is used as the d x n sketch (ld d) instead of generating a SASO (parity tests share one sketch
 * between this path and the oracle, like test/drivers/test_bqrrp_gpu.cu:91-110); if A_hat_out is non-NULL the
 * sketch that was factored is copied there BEFORE geqp3.  *rank_out = CQRRPT::rank; times_us[8] may be NULL.
 *                                                                         drivers/rl_cqrrpt.hh:147-391 */
int rlhip_drv_cqrrpt_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* R, int64_t ldr,
                         int64_t* J, double d_factor, int64_t nnz, double eps, uint32_t state[6],
                         const double* A_hat_in, double* A_hat_out, int64_t* rank_out, long* times_us, int qrcp);

/* hqrrp (drivers/rl_hqrrp.hh:812): GEQP3-format Householder QR with randomized pivoting.  qr_type 0 Householder panel
 * (pivoted inside the panel when panel_pivoting != 0), 1 geqrf, 2 CholQR (2 needs panel_pivoting == 0, as in the
 * reference's dispatch :587-591).  G_out (may be NULL): receives the (nb_alg+pp) x m Uniform(-1,1) sketching matrix.
 * Returns 0, or 1 if a CholQR panel broke down. */
int rlhip_drv_hqrrp_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, int64_t* jpvt, double* tau, int64_t nb_alg,
                        int64_t pp, int64_t panel_pivoting, int64_t qr_type, uint32_t state[6], double* G_out);
/* the same call with the reference's `T** timing` argument armed (rl_hqrrp.hh:815, :1144-1164): times27 receives the 27 entries the
 * reference's HQRRP_runtime_breakdown benchmark prints, in microseconds (layout: include/RandLAPACK_amd/rl_hqrrp.hh) */
int rlhip_drv_hqrrp_timed_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, int64_t* jpvt, double* tau, int64_t nb_alg,
                              int64_t pp, int64_t panel_pivoting, int64_t qr_type, uint32_t state[6], double times27[27]);

/* BQRRP<double>::call.  qrcp_wide {0 luqr, 1 geqp3}, qr_tall {0 geqrt, 1 cholqr, 2 geqrf}, apply_trans_q {0 ormqr, 1 gemqrt}
 * follow the reference's enum order (rl_bqrrp.hh:45-49); -1 keeps the object's default = the reference's {luqr, geqrf, ormqr}
 * (rl_bqrrp.hh:74-76).  The fastest triple on the device is {0, 1, 1} = {luqr, cholqr, gemqrt} (BQRRP::use_fast_subroutines()).
 * DIVERGENCE from the reference, qr_tall = cholqr only: when the panel's Cholesky factorization breaks down, or diag(R_chol) is
 * graded beyond eps^(1/4) (the preconditioned panel is not well conditioned, so Cholesky QR cannot deliver an orthonormal Q), the
 * panel is re-factored with Householder reflectors (BQRRP::cholqr_fallback, default on; environment RLHIP_BQRRP_CHOLQR_FALLBACK=0
 * restores the reference's behaviour, which carries on with the half-factored Gram matrix, rl_bqrrp.hh:461).  Pivots, rank and
 * well-conditioned panels are unaffected.
 * Row-sharded context (rlhip_comm_*): m and A are this rank's rows, tau needs min(global rows, n) entries; every qr_tall runs sharded
 * (cholqr: one b x b Gram all-reduce per panel; geqrf / geqrt: TSQR, the ranks' b x b triangles stacked by one all-reduce);
 * qr_tall + 16 (16 + 3 for the object's default qr_tall) selects the BLOCK-CYCLIC layout (global row blocks of b_sz rows dealt round-robin,
 * block g on rank g % P, stacked in increasing order in A) instead of one contiguous row block per rank.  A (m x n, lda) -> GEQP3
 * format, tau (min(m,n)), J (n) all on the device.  A_sk_in / A_sk_out: shared-sketch hooks as for CQRRPT (d x n,
 * ld d, d = (int64)(d_factor * b_sz)).  times_us[9] may be NULL.              drivers/rl_bqrrp.hh:155-665 */
int rlhip_drv_bqrrp_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double d_factor, int64_t b_sz,
                        int64_t internal_nb, double tol, double* tau, int64_t* J, uint32_t state[6],
                        const double* A_sk_in, double* A_sk_out, int64_t* rank_out, long* times_us, int qrcp_wide, int qr_tall,
                        int apply_trans_q);

/* BQRRP_GPU<T>::call (drivers/rl_bqrrp_gpu.hh:120-129, body :152-934): the reference's device class -- the d x n sketch A_sk (ld d,
 * DEVICE, overwritten) is an INPUT, d >= b_sz is free (not tied to a d_factor).  qr_tall in the reference's enum order
 * (BQRRPGPUSubroutines::QRTall, :44-46): 0 cholqr, 1 geqrf, -1 = the object's default (geqrf, :84).  tol <= 0 keeps eps.
 * A (m x n, lda) -> GEQP3 format, tau (n), J (n), all DEVICE.  times15 (may be NULL) receives BQRRP_GPU::times, the 15 entries of
 * rl_bqrrp_gpu.hh:829-834 in microseconds: {preallocation, qrcp_main, copy_A_sk, qrcp_piv, copy_A, piv_A, copy_J, updating_J,
 * preconditioning, qr_tall, q_reconstruction, apply_transq, sample_update, rest, total}. */
int rlhip_drv_bqrrp_gpu_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* A_sk, int64_t d, int64_t b_sz, int qr_tall,
                            double tol, double* tau, int64_t* J, int64_t* rank_out, long* times15);
int rlhip_drv_bqrrp_gpu_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* A_sk, int64_t d, int64_t b_sz, int qr_tall,
                            float tol, float* tau, int64_t* J, int64_t* rank_out, long* times15);
/* CQRRPT_GPU<T>::call (drivers/rl_cqrrpt_gpu.hh:117-127, body :149-390): HOST matrices in and out as in the reference (A m x n lda -> Q,
 * R n x n ldr, J n); every stage runs on the device, the class owns the two transfers.  nnz <= 0 keeps the object's default (2);
 * no_hqrrp: 1 geqp3 (default, :75), 0 hqrrp, -1 default.  A_hat_out_host (may be NULL): HOST buffer receiving the d x n sketch that
 * was factored (d = (int64)(d_factor * n)) -- the shared-sketch hook of the parity tests.  times8 (may be NULL): CQRRPT_GPU::times
 * {saso, qrcp, rank_reveal, cholqr, a_mod_piv, a_mod_trsm, rest, total} in microseconds (:371).  Returns 0 or 1. */
int rlhip_drv_cqrrpt_gpu_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A_host, int64_t lda, double* R_host, int64_t ldr, int64_t* J_host,
                             double d_factor, int64_t nnz, double eps, int no_hqrrp, uint32_t state[6], double* A_hat_out_host,
                             int64_t* rank_out, long* times8);
int rlhip_drv_cqrrpt_gpu_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A_host, int64_t lda, float* R_host, int64_t ldr, int64_t* J_host,
                             float d_factor, int64_t nnz, float eps, int no_hqrrp, uint32_t state[6], float* A_hat_out_host,
                             int64_t* rank_out, long* times8);

/* ABRIK<double>::call(m, n, A, lda, k, U, V, Sigma, state), the dense-pointer overload (drivers/rl_abrik.hh:122-143).  A (m x n, lda) is not
 * modified.  *U (m x triplets), *Sigma (triplets), *V (n x triplets) are allocated by the callee (rlhip_malloc), freed by the caller.
 * max_krylov_iters <= 0 keeps the object's default (INT_MAX). */
int rlhip_drv_abrik_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, int64_t k, double tol, int64_t max_krylov_iters,
                        double** U, double** Sigma, double** V, uint32_t state[6], int64_t* triplets, int64_t* iters, double* norm_R_end,
                        int qr_exp /* 0 geqrf_ungqr, 1 cqrrt, -1 default (geqrf_ungqr); both run on a row-sharded context */);

/* CQRRT<double>::call (drivers/rl_cqrrt.hh:124): unpivoted CQRRPT.  A (m x n, lda) -> Q; upper triangle of R (n x n, ldr).
 * A_hat_in / A_hat_out: shared-sketch hooks as for CQRRPT (d x n, ld d, d = (int64)(d_factor * n)).  Returns 0 or 1. */
int rlhip_drv_cqrrt_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* R, int64_t ldr, double d_factor, int64_t nnz,
                        double eps, uint32_t state[6], const double* A_hat_in, double* A_hat_out);

/* fp32 instantiations (same contracts; tol / eps / d_factor are float) */
int rlhip_drv_stab_f32(rlhip_ctx* ctx, int kind, int cond_check, int64_t m, int64_t k, float* A, int* chol_fail);
int rlhip_drv_rsvd_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t* k, int64_t b_sz, float tol,
                       int64_t p, int64_t q, int rs_stab, int rf_orth, int qb_orth, int orth_check, float** U,
                       float** S, float** V, uint32_t state[6], int* qb_ret);
int rlhip_drv_cqrrpt_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* R, int64_t ldr,
                         int64_t* J, float d_factor, int64_t nnz, float eps, uint32_t state[6],
                         const float* A_hat_in, float* A_hat_out, int64_t* rank_out, long* times_us, int qrcp);
int rlhip_drv_hqrrp_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, int64_t* jpvt, float* tau, int64_t nb_alg,
                        int64_t pp, int64_t panel_pivoting, int64_t qr_type, uint32_t state[6], float* G_out);
int rlhip_drv_bqrrp_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float d_factor, int64_t b_sz,
                        int64_t internal_nb, float tol, float* tau, int64_t* J, uint32_t state[6],
                        const float* A_sk_in, float* A_sk_out, int64_t* rank_out, long* times_us, int qrcp_wide, int qr_tall,
                        int apply_trans_q);

/* ---- drivers over abstract linear operators (include/RandLAPACK_amd/rl_linops.hh, rl_qr_linops.hh).
 * An operator is described by plain arrays: kind 0 = dense column-major (dense, ld); kind 1 = CSR with int64 indices
 * (rowptr, colidx, vals; nnz entries); kind 2 = CSC (RandBLAS::sparse_data::CSCMatrix: the `rowptr` field carries colptr (cols + 1), the `colidx`
 * field the ROW indices); kind 3 = COO (COOMatrix: `rowptr` carries the nnz row indices, `colidx` the nnz column indices; any order, duplicates
 * are summed).  All arrays are DEVICE pointers.  `right` == NULL: the operator is `left`;
 * otherwise it is the implicit product left * right (linops::CompositeOperator, rl_composite_linop.hh:43). */
typedef struct rlhip_linop_desc {
    int kind;
    int64_t rows, cols;
    const void* dense;
    int64_t ld;
    int64_t nnz;
    const int64_t* rowptr;
    const int64_t* colidx;
    const void* vals;
} rlhip_linop_desc;

/* alg: 0 CholQR_linops (rl_cholqr_linops.hh:60), 1 sCholQR3_linops (rl_scholqr3_linops.hh:182), 2 sCholQR3_linops_basic (:600),
 *      3 CQRRT_linops (rl_cqrrt_linops.hh:144).  R (n x n, ldr) receives the upper-triangular factor.  block_size as the classes'
 *      member.  Q_out != NULL turns test_mode on and receives a library-owned copy of Q (m x n; free with rlhip_free).
 *      d_factor, nnz, use_dense_sketch, state, A_hat_in/out (d x n sketch injection / export): CQRRT_linops only.
 *      Returns the class's return value (0 ok, >0 Cholesky breakdown index), negative on argument / device errors. */
int rlhip_drv_qr_linops_f64(rlhip_ctx* ctx, int alg, const rlhip_linop_desc* left, const rlhip_linop_desc* right, double* R, int64_t ldr,
                            int64_t block_size, double** Q_out, double d_factor, int64_t nnz, int use_dense_sketch, uint32_t state[6],
                            const double* A_hat_in, double* A_hat_out);
int rlhip_drv_qr_linops_f32(rlhip_ctx* ctx, int alg, const rlhip_linop_desc* left, const rlhip_linop_desc* right, float* R, int64_t ldr,
                            int64_t block_size, float** Q_out, float d_factor, int64_t nnz, int use_dense_sketch, uint32_t state[6],
                            const float* A_hat_in, float* A_hat_out);
/* ABRIK<double>::call on an operator given by descriptor(s) (rl_abrik.hh:166; sparse / composite operators as in
 * benchmark/bench_ABRIK/ABRIK_speed_comparisons_sparse.cc).  Outputs as rlhip_drv_abrik_f64. */
int rlhip_drv_abrik_linop_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right /* must be NULL */, int64_t k, double tol,
                              int64_t max_krylov_iters, double** U, double** Sigma, double** V, uint32_t state[6], int64_t* triplets,
                              int64_t* iters, double* norm_R_end, int qr_exp);
/* The same call with ABRIK's subroutine timers armed (ABRIK(verbose, time_subroutines = true, tol), rl_abrik.hh:64; the 13 entries of
 * ABRIK::times, rl_abrik.hh:733-734, in microseconds: allocation, get_factors, ungqr, reorth, qr, gemm_A, main_loop, sketching, r_cpy,
 * s_cpy, norm, rest, total).  Every lap drains the stream, so a timed call is slower than an untimed one. */
int rlhip_drv_abrik_linop_timed_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, int64_t k, double tol, int64_t max_krylov_iters, double** U,
                                    double** Sigma, double** V, uint32_t state[6], int64_t* triplets, int64_t* iters, double* norm_R_end,
                                    int qr_exp, long times[13]);
/* C (m x n, ldc) = alpha * op(A) * B + beta * C for an operator given by descriptor(s): the raw operator call, for tests and for
 * callers that only want the SpMM / composite product.  side 'L' or 'R', trans 'N' or 'T', column-major B and C. */
int rlhip_linop_apply_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, char side, char trans, int64_t m,
                          int64_t n, int64_t k, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);

/* The same product with a BLOCK VIEW of the operator (rl_dense_linop.hh:295-330, rl_sparse_linop.hh:393-465, rl_composite_linop.hh:505-530):
 * how 0 = row_block(view[0], view[2]), 1 = col_block(view[1], view[3]), 2 = submatrix(view[0], view[1], view[2], view[3]);
 * view = {row_start, col_start, row_count, col_count}; m, n, k describe the product with the VIEW. */
int rlhip_linop_apply_view_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, int how, const int64_t view[4], char side,
                               char trans, int64_t m, int64_t n, int64_t k, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* linops::RegExplicitSymLinOp (rl_sym_linops.hh:134-233): C (dim x n) = alpha * (A + mu_i I) * B + beta * C with A given by its UPPER triangle
 * (dim x dim, lda, DEVICE; the strictly lower triangle is never read); regs_host[num_ops] on the HOST; eval_includes_reg as
 * set_eval_includes_reg; with num_ops > 1 column i takes regs[i] and n must equal num_ops. */
int rlhip_regsym_apply_f64(rlhip_ctx* ctx, int64_t dim, const double* A, int64_t lda, const double* regs_host, int64_t num_ops, int eval_includes_reg,
                           int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);

/* gen::mat_gen (RandLAPACK/testing/rl_gen.hh:712-772) in HBM.  type: 0 polynomial, 1 exponential, 2 gaussian, 3 step, 4 spiked,
 * 5 adverserial, 6 bad_cholqr, 7 kahan (the enum order of rl_gen.hh:22-31).  A: m x n DEVICE (rank x rank, ld rank, when diag != 0).
 * Fields as mat_gen_info; rank_out (may be NULL) receives info.rank after the call (changed only by check_true_rank). */
int rlhip_drv_mat_gen_f64(rlhip_ctx* ctx, int type, int64_t m, int64_t n, int64_t rank, double cond_num, double scaling, double exponent,
                          int diag, double theta, double perturb, double frac_spectrum_one, int check_true_rank, double* A,
                          uint32_t state[6], int64_t* rank_out);
int rlhip_drv_mat_gen_f32(rlhip_ctx* ctx, int type, int64_t m, int64_t n, int64_t rank, float cond_num, float scaling, float exponent,
                          int diag, float theta, float perturb, float frac_spectrum_one, int check_true_rank, float* A,
                          uint32_t state[6], int64_t* rank_out);

/* REVD2<SYRF<SYPS, Stabilization>>::call (drivers/rl_revd2.hh:96-243; comps/rl_syrf.hh, rl_syps.hh): A ~ V diag(eigvals) V^T for a
 * symmetric PSD A given by its `uplo` triangle (m x m, ld m, DEVICE; the other triangle is never read).  *k: in = starting rank,
 * out = rank used.  *V (m x k) and *eigvals (k) are library-allocated DEVICE buffers (rlhip_free).  orth_kind: 0 CholQRQ, 1 HQRQ,
 * 2 PLUL (the reference's tests use HQRQ).  err_out (may be NULL): the final power-method error estimate. */
int rlhip_drv_revd2_f64(rlhip_ctx* ctx, char uplo, int64_t m, const double* A, int64_t* k, double tol, int64_t syps_passes,
                        int64_t passes_per_stab, int error_est_p, int orth_kind, double** V, double** eigvals, uint32_t state[6],
                        double* err_out);
/* SYRF::call alone (comps/rl_syrf.hh:44-92): Q (m x k, DEVICE, caller-allocated) <- orth(A * SYPS sketch). */
int rlhip_drv_syrf_f64(rlhip_ctx* ctx, char uplo, int64_t m, const double* A, int64_t k, int64_t syps_passes, int64_t passes_per_stab,
                       int orth_kind, double* Q, uint32_t state[6]);

/* rp_cholesky (comps/rl_rpchol.hh:114-187; include/RandLAPACK_amd/rl_rpchol.hh) on a squared-exponential kernel matrix (RBF): the n points are
 * the columns of X (rows_x x n, ldx, DEVICE), K(i,j) = exp(-|x_i - x_j|^2 / (2 bandwidth^2)) + reg [i == j].  *k: in = target rank, out =
 * achieved rank.  S_host (k entries) receives the pivots in the order chosen, F (n x k, ldf, DEVICE, caller-allocated) the factor with
 * K ~ F F^T.  status[0] = w_status (downdate_d_and_cdf's 0 / 1 / 2 after the last block), status[1] = c_status (potrf's info of the block
 * that broke down, 0 if none).  A diagonal that is no valid weight vector (e.g. all zero) returns 0 with *k = 0 and status[0] = 1 or 2;
 * the C++ rp_cholesky throws there, as the reference's weights_to_cdf does.  b in [1, 4096]. */
int rlhip_drv_rpchol_rbf_f64(rlhip_ctx* ctx, const double* X, int64_t ldx, int64_t rows_x, int64_t n, double bandwidth, double reg, int64_t* k,
                             int64_t b, int64_t* S_host, double* F, int64_t ldf, uint32_t state[6], int status[2]);
int rlhip_drv_rpchol_rbf_f32(rlhip_ctx* ctx, const float* X, int64_t ldx, int64_t rows_x, int64_t n, float bandwidth, float reg, int64_t* k,
                             int64_t b, int64_t* S_host, float* F, int64_t ldf, uint32_t state[6], int status[2]);
/* the same on a full symmetric PSD matrix A (n x n, lda, DEVICE; its upper triangle is symmetrised into a scratch copy, linops::ExplicitSymLinOp),
 * which is what the reference's own tests feed it (test/comps/test_rpchol.cc) */
int rlhip_drv_rpchol_dense_f64(rlhip_ctx* ctx, int64_t n, const double* A, int64_t lda, int64_t* k, int64_t b, int64_t* S_host, double* F,
                               int64_t ldf, uint32_t state[6], int status[2]);
int rlhip_drv_rpchol_dense_f32(rlhip_ctx* ctx, int64_t n, const float* A, int64_t lda, int64_t* k, int64_t b, int64_t* S_host, float* F,
                               int64_t ldf, uint32_t state[6], int status[2]);
/* rpchol_pc_data (comps/rl_preconditioners.hh:348-361) on the RBF matrix above: V (n x k, ld n, DEVICE) <- left singular vectors of the RPCholesky
 * factor, eigvals (k, DEVICE) <- its squared singular values, so K ~ V diag(eigvals) V^T.  *k: achieved rank.  -100 if the diagonal fails. */
int rlhip_drv_rpchol_pc_data_rbf_f64(rlhip_ctx* ctx, const double* X, int64_t ldx, int64_t rows_x, int64_t n, double bandwidth, double reg,
                                     int64_t* k, int64_t b, double* V, double* eigvals, uint32_t state[6]);
int rlhip_drv_rpchol_pc_data_rbf_f32(rlhip_ctx* ctx, const float* X, int64_t ldx, int64_t rows_x, int64_t n, float bandwidth, float reg,
                                     int64_t* k, int64_t b, float* V, float* eigvals, uint32_t state[6]);

/* pcg (comps/rl_determiter.hh:371-493; include/RandLAPACK_amd/rl_determiter.hh) on (A + mu_i I) x_i = h_i with the spectral preconditioner
 * (linops/rl_sym_linops.hh:204-379) built from V (n x dim_pre, ldv, DEVICE) and eigvals (dim_pre, DEVICE, positive and decreasing) with
 * A ~ V diag(eigvals) V^T.  A: linops::RegExplicitSymLinOp over the UPPER triangle of a DEVICE n x n matrix (lda).  regs_host: num_ops
 * regularization parameters on the HOST; num_ops == 1 is block PCG with block size s, num_ops == s keeps s single-vector iterations in lockstep,
 * anything else is refused (-100).  H (n x s, ld n, DEVICE) holds the right-hand sides, X (n x s, ld n, DEVICE) the starting point on entry and
 * the solution on return.  Iterations stop when ||N R||_F < tol (1 + ||N R_0||_F) or after max_iters.  *iters = iterations started;
 * hist (HOST, 2 (max_iters + 1) entries) receives ||R||_F and ||N R||_F per iteration, iteration 0 first: hist[2 i], hist[2 i + 1]; the entries
 * of iterations not run stay as they were. */
int rlhip_drv_pcg_dense_f64(rlhip_ctx* ctx, int64_t n, const double* A, int64_t lda, const double* regs_host, int64_t num_ops, const double* V,
                            int64_t ldv, const double* eigvals, int64_t dim_pre, const double* H, double* X, int64_t s, double tol, int64_t max_iters,
                            int64_t* iters, double* hist);
int rlhip_drv_pcg_dense_f32(rlhip_ctx* ctx, int64_t n, const float* A, int64_t lda, const float* regs_host, int64_t num_ops, const float* V,
                            int64_t ldv, const float* eigvals, int64_t dim_pre, const float* H, float* X, int64_t s, float tol, int64_t max_iters,
                            int64_t* iters, float* hist);
/* the same over linops::RBFKernelMatrix: the n points are the columns of X_pts (rows_x x n, ldx, DEVICE), K(i,j) = exp(-|x_i - x_j|^2 / (2 bandwidth^2)) */
int rlhip_drv_pcg_rbf_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, double bandwidth, const double* regs_host,
                          int64_t num_ops, const double* V, int64_t ldv, const double* eigvals, int64_t dim_pre, const double* H, double* X, int64_t s,
                          double tol, int64_t max_iters, int64_t* iters, double* hist);
int rlhip_drv_pcg_rbf_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, float bandwidth, const float* regs_host,
                          int64_t num_ops, const float* V, int64_t ldv, const float* eigvals, int64_t dim_pre, const float* H, float* X, int64_t s,
                          float tol, int64_t max_iters, int64_t* iters, float* hist);
/* krill_full_rpchol (drivers/rl_krill.hh:20-55; include/RandLAPACK_amd/rl_krill.hh) on the RBF matrix above: rpchol_pc_data of the unregularized
 * kernel with rank *k (in: target, < 0: sqrt(n); out: achieved) and block size b (< 0: min(64, n / 4)), then pcg as above with s right-hand sides.
 * state[6] is advanced as rlhip_drv_rpchol_pc_data_rbf_* advances it. */
int rlhip_drv_krill_full_rpchol_rbf_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, double bandwidth,
                                        const double* regs_host, int64_t num_ops, const double* H, double* X, int64_t s, double tol, int64_t max_iters,
                                        int64_t* k, int64_t b, uint32_t state[6], int64_t* iters, double* hist);
int rlhip_drv_krill_full_rpchol_rbf_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, float bandwidth,
                                        const float* regs_host, int64_t num_ops, const float* H, float* X, int64_t s, float tol, int64_t max_iters,
                                        int64_t* k, int64_t b, uint32_t state[6], int64_t* iters, float* hist);
/* krr_predict (include/RandLAPACK_amd/rl_krill.hh) over linops::RBFCrossKernel: Y (mz x s, ldy) = K(Z, X_pts) * coeffs (n x s, ldcoef); Z is
 * rows_x x mz (ldz), X_pts rows_x x n (ldx), all DEVICE. */
int rlhip_drv_krr_predict_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n, const double* X_pts, int64_t ldx,
                              double bandwidth, int64_t s, const double* coeffs, int64_t ldcoef, double* Y, int64_t ldy);
int rlhip_drv_krr_predict_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n, const float* X_pts, int64_t ldx,
                              float bandwidth, int64_t s, const float* coeffs, int64_t ldcoef, float* Y, int64_t ldy);
/* linops::RBFKernelMatrix::operator() through the object, with set_eval_includes_reg(eval_includes_reg) and set_matrix_free(matrix_free):
 * C (dim x n) = alpha * (K [+ regs]) * B + beta * C, the arguments of rlhip_rbf_apply_*. */
int rlhip_drv_rbf_kernel_apply_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t dim, double bandwidth,
                                   const double* regs_host, int64_t num_ops, int eval_includes_reg, int matrix_free, int64_t n, double alpha,
                                   const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
int rlhip_drv_rbf_kernel_apply_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t dim, float bandwidth,
                                   const float* regs_host, int64_t num_ops, int eval_includes_reg, int matrix_free, int64_t n, float alpha,
                                   const float* B, int64_t ldb, float beta, float* C, int64_t ldc);
/* The four RBF drivers above with the kernel function as an argument (RLHIP_PDK_*, include/rlhip.h): `int kernel` in front of the bandwidth, passed
 * to the object by set_kernel; everything behind the object -- rp_cholesky, rpchol_pc_data, pcg, krr_predict -- is the same code.  An unknown kind
 * returns -(position of kernel): -6, -6, -9, -6. */
int rlhip_drv_rpchol_pdk_f64(rlhip_ctx* ctx, const double* X, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth, double reg,
                             int64_t* k, int64_t b, int64_t* S_host, double* F, int64_t ldf, uint32_t state[6], int status[2]);
int rlhip_drv_rpchol_pdk_f32(rlhip_ctx* ctx, const float* X, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth, float reg,
                             int64_t* k, int64_t b, int64_t* S_host, float* F, int64_t ldf, uint32_t state[6], int status[2]);
int rlhip_drv_krill_full_rpchol_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                        const double* regs_host, int64_t num_ops, const double* H, double* X, int64_t s, double tol, int64_t max_iters,
                                        int64_t* k, int64_t b, uint32_t state[6], int64_t* iters, double* hist);
int rlhip_drv_krill_full_rpchol_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                        const float* regs_host, int64_t num_ops, const float* H, float* X, int64_t s, float tol, int64_t max_iters,
                                        int64_t* k, int64_t b, uint32_t state[6], int64_t* iters, float* hist);
int rlhip_drv_krr_predict_pdk_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n, const double* X_pts, int64_t ldx,
                                  int kernel, double bandwidth, int64_t s, const double* coeffs, int64_t ldcoef, double* Y, int64_t ldy);
int rlhip_drv_krr_predict_pdk_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n, const float* X_pts, int64_t ldx,
                                  int kernel, float bandwidth, int64_t s, const float* coeffs, int64_t ldcoef, float* Y, int64_t ldy);
int rlhip_drv_pdk_kernel_apply_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t dim, int kernel, double bandwidth,
                                   const double* regs_host, int64_t num_ops, int eval_includes_reg, int matrix_free, int64_t n, double alpha,
                                   const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
int rlhip_drv_pdk_kernel_apply_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t dim, int kernel, float bandwidth,
                                   const float* regs_host, int64_t num_ops, int eval_includes_reg, int matrix_free, int64_t n, float alpha,
                                   const float* B, int64_t ldb, float beta, float* C, int64_t ldc);
/* Restricted kernel ridge regression (include/RandLAPACK_amd/rl_krill.hh) over linops::RBFKernelMatrix with the kernel function
 * `kernel` (RLHIP_PDK_*): the k centres are points of X_pts, the model is k coefficients per right-hand side.  H: n x s (ldh), alpha: k x s
 * (ldalpha), both DEVICE; regs_host: num_ops (1 or s) regularization parameters >= 0 on the HOST.  An unknown kind returns -(position of
 * kernel): -6, -6, -9; a refused argument -100 with rlhip_last_error().
 * krill_restricted_rpchol: the centres are the pivots of rp_cholesky.  *k in: centres asked for (< 0: sqrt(n)), out: the achieved rank; b: block
 * size (< 0: min(64, n / 4)); S_host (k_in entries) receives the centres in selection order, -1 behind the achieved rank, where the rows of
 * alpha are zero; status[2] = {w_status, c_status} as rlhip_drv_rpchol_* report them; state[6] advances as theirs. */
int rlhip_drv_krill_restricted_rpchol_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                              const double* regs_host, int64_t num_ops, const double* H, int64_t ldh, int64_t s, int64_t* k, int64_t b,
                                              int64_t* S_host, double* alpha, int64_t ldalpha, uint32_t state[6], int status[2]);
int rlhip_drv_krill_restricted_rpchol_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                              const float* regs_host, int64_t num_ops, const float* H, int64_t ldh, int64_t s, int64_t* k, int64_t b,
                                              int64_t* S_host, float* alpha, int64_t ldalpha, uint32_t state[6], int status[2]);
/* krill_restricted: the same fit with the k distinct centres S_host given.  *info = potrf's info of K(S,S): 0, or the 1-based position of the
 * first centre that depends on the ones before it; then alpha is untouched. */
int rlhip_drv_krill_restricted_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                       const double* regs_host, int64_t num_ops, const double* H, int64_t ldh, int64_t s, int64_t k, const int64_t* S_host,
                                       double* alpha, int64_t ldalpha, int64_t* info);
int rlhip_drv_krill_restricted_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                       const float* regs_host, int64_t num_ops, const float* H, int64_t ldh, int64_t s, int64_t k, const int64_t* S_host,
                                       float* alpha, int64_t ldalpha, int64_t* info);
/* krill_restricted_rpchol_cv and krill_restricted_cv: the two fits above with the regularization of every column chosen from the
 * HOST grid mu_grid_host[g] (g >= 1, every value >= 0) in place of regs_host.  criterion: 0 leave-one-out, 1 generalized cross-validation
 * n rss / (n - dof)^2; per column the smallest finite value wins, the lower index on a tie.  HOST outputs, each may be NULL: loo_host and
 * rss_host (g x s, stride g: the sums over the n points of the squared leave-one-out residuals and of the squared residuals), dof_host (g),
 * best_host (s indices into the grid), best_mu_host (s).  alpha is the fit with best_mu_host.  An empty grid, a negative grid value, an
 * unknown criterion, a NULL buffer or a column without a finite criterion return -100 with rlhip_last_error().  With *info != 0
 * krill_restricted_cv leaves alpha and the HOST outputs untouched. */
int rlhip_drv_krill_restricted_rpchol_cv_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                                 const double* mu_grid_host, int64_t g, int criterion, const double* H, int64_t ldh, int64_t s, int64_t* k,
                                                 int64_t b, int64_t* S_host, double* alpha, int64_t ldalpha, uint32_t state[6], int status[2],
                                                 double* loo_host, double* rss_host, double* dof_host, int64_t* best_host, double* best_mu_host);
int rlhip_drv_krill_restricted_rpchol_cv_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                                 const float* mu_grid_host, int64_t g, int criterion, const float* H, int64_t ldh, int64_t s, int64_t* k,
                                                 int64_t b, int64_t* S_host, float* alpha, int64_t ldalpha, uint32_t state[6], int status[2],
                                                 double* loo_host, double* rss_host, double* dof_host, int64_t* best_host, double* best_mu_host);
int rlhip_drv_krill_restricted_cv_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                          const double* mu_grid_host, int64_t g, int criterion, const double* H, int64_t ldh, int64_t s, int64_t k,
                                          const int64_t* S_host, double* alpha, int64_t ldalpha, int64_t* info, double* loo_host, double* rss_host,
                                          double* dof_host, int64_t* best_host, double* best_mu_host);
int rlhip_drv_krill_restricted_cv_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                          const float* mu_grid_host, int64_t g, int criterion, const float* H, int64_t ldh, int64_t s, int64_t k,
                                          const int64_t* S_host, float* alpha, int64_t ldalpha, int64_t* info, double* loo_host, double* rss_host,
                                          double* dof_host, int64_t* best_host, double* best_mu_host);
/* krr_predict_restricted: Y (mz x s, ldy) = K(Z, X_pts(:, S)) alpha -- the k centre columns are gathered and krr_predict runs on them: mz x k
 * kernel evaluations.  Z is rows_x x mz (ldz), X_pts rows_x x n (ldx); k <= 65535. */
int rlhip_drv_krr_predict_restricted_pdk_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n, const double* X_pts,
                                             int64_t ldx, int kernel, double bandwidth, int64_t k, const int64_t* S_host, int64_t s, const double* alpha,
                                             int64_t ldalpha, double* Y, int64_t ldy);
int rlhip_drv_krr_predict_restricted_pdk_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n, const float* X_pts,
                                             int64_t ldx, int kernel, float bandwidth, int64_t k, const int64_t* S_host, int64_t s, const float* alpha,
                                             int64_t ldalpha, float* Y, int64_t ldy);
/* Gradients of the fitted functions with respect to the evaluation point: krr_predict_grad and krr_predict_restricted_grad,
 * the arguments of rlhip_drv_krr_predict_pdk_* and rlhip_drv_krr_predict_restricted_pdk_* with G (DEVICE, rows_x x (mz s), ldg >= rows_x)
 * in the place of Y: column c * mz + i is the gradient at Z(:, i) of the function of the c-th regularization, laid out like Z. */
int rlhip_drv_krr_predict_grad_pdk_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n, const double* X_pts,
                                       int64_t ldx, int kernel, double bandwidth, int64_t s, const double* coeffs, int64_t ldcoef, double* G, int64_t ldg);
int rlhip_drv_krr_predict_grad_pdk_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n, const float* X_pts,
                                       int64_t ldx, int kernel, float bandwidth, int64_t s, const float* coeffs, int64_t ldcoef, float* G, int64_t ldg);
int rlhip_drv_krr_predict_restricted_grad_pdk_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n,
                                                  const double* X_pts, int64_t ldx, int kernel, double bandwidth, int64_t k, const int64_t* S_host,
                                                  int64_t s, const double* alpha, int64_t ldalpha, double* Grad, int64_t ldgrad);
int rlhip_drv_krr_predict_restricted_grad_pdk_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n,
                                                  const float* X_pts, int64_t ldx, int kernel, float bandwidth, int64_t k, const int64_t* S_host,
                                                  int64_t s, const float* alpha, int64_t ldalpha, float* Grad, int64_t ldgrad);
/* The predictive variance of a restricted fit.  rlhip_drv_krill_restricted_rpchol_gp_pdk_* and rlhip_drv_krill_restricted_gp_pdk_*
 * are the two fits above with three more arguments: G_out (DEVICE, k_in x k_in, ldg >= k_in) and sigma_out (DEVICE, k_in) receive the fit's
 * basis (RandLAPACK::KrillRestrictedBasis), zero behind the achieved rank; alpha, S_host, state and status are bit for bit those of the fit
 * without them; with *info != 0 the basis is untouched, as alpha is.
 * rlhip_drv_krr_predict_restricted_var_pdk_*: V (DEVICE, mz x s, ldv) = the variance of the latent function at the mz points Z for the
 * regularizations mus_host (HOST, num_mus = 1 or s values >= 0), from the k centres S_host and the basis (G_basis, ldg, sigma) of their
 * fit: RandLAPACK::krr_predict_restricted_var, one call of rlhip_pdk_cross_var_*; fused_kernel != 0 asks for its fused kernel
 * (rlhip_pdk_var_set_fused for the length of the call).  An unknown kind returns -9. */
int rlhip_drv_krill_restricted_rpchol_gp_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                                 const double* regs_host, int64_t num_ops, const double* H, int64_t ldh, int64_t s, int64_t* k, int64_t b,
                                                 int64_t* S_host, double* alpha, int64_t ldalpha, uint32_t state[6], int status[2], double* G_out,
                                                 int64_t ldg, double* sigma_out);
int rlhip_drv_krill_restricted_rpchol_gp_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                                 const float* regs_host, int64_t num_ops, const float* H, int64_t ldh, int64_t s, int64_t* k, int64_t b,
                                                 int64_t* S_host, float* alpha, int64_t ldalpha, uint32_t state[6], int status[2], float* G_out,
                                                 int64_t ldg, float* sigma_out);
int rlhip_drv_krill_restricted_gp_pdk_f64(rlhip_ctx* ctx, const double* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, double bandwidth,
                                          const double* regs_host, int64_t num_ops, const double* H, int64_t ldh, int64_t s, int64_t k,
                                          const int64_t* S_host, double* alpha, int64_t ldalpha, int64_t* info, double* G_out, int64_t ldg,
                                          double* sigma_out);
int rlhip_drv_krill_restricted_gp_pdk_f32(rlhip_ctx* ctx, const float* X_pts, int64_t ldx, int64_t rows_x, int64_t n, int kernel, float bandwidth,
                                          const float* regs_host, int64_t num_ops, const float* H, int64_t ldh, int64_t s, int64_t k,
                                          const int64_t* S_host, float* alpha, int64_t ldalpha, int64_t* info, float* G_out, int64_t ldg,
                                          float* sigma_out);
int rlhip_drv_krr_predict_restricted_var_pdk_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t n, const double* X_pts,
                                                 int64_t ldx, int kernel, double bandwidth, int64_t k, const int64_t* S_host, const double* G_basis,
                                                 int64_t ldg, const double* sigma, int64_t s, const double* mus_host, int64_t num_mus, double* V,
                                                 int64_t ldv, int fused_kernel);
int rlhip_drv_krr_predict_restricted_var_pdk_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t n, const float* X_pts,
                                                 int64_t ldx, int kernel, float bandwidth, int64_t k, const int64_t* S_host, const float* G_basis,
                                                 int64_t ldg, const float* sigma, int64_t s, const float* mus_host, int64_t num_mus, float* V,
                                                 int64_t ldv, int fused_kernel);
/* posm_square (comps/rl_determiter.hh:231-282) as the C++ layer runs it: rlhip_posm_square_* and, after a failed pivot, the eigenvalue fallback on
 * the host.  LHS, RHS: s x s DEVICE, ld s.  *code = rank(LHS), -(s + 1) not positive semidefinite, -(s + 2) zero up to rounding. */
int rlhip_drv_posm_square_f64(rlhip_ctx* ctx, int64_t s, const double* LHS, double* RHS, int diag_only, int64_t* code);
int rlhip_drv_posm_square_f32(rlhip_ctx* ctx, int64_t s, const float* LHS, float* RHS, int diag_only, int64_t* code);

/* pcg_saddle (comps/rl_determiter.hh:18-134; include/RandLAPACK_amd/rl_determiter.hh): (A'A + delta I) x = A'b - c by conjugate gradients
 * preconditioned with M M', then y = b - A x.  A: m x n (lda); M: n x k (ldm); b, y: m; c, x0, x: n; resid_vec: iter_lim + 1 -- all DEVICE.
 * *iters (may be NULL) = iterations run; resid_vec[0 .. *iters] are written.  -100 with rlhip_last_error() on a refused argument. */
int rlhip_drv_pcg_saddle_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, const double* b, const double* c, double delta,
                             int64_t iter_lim, double* resid_vec, double tol, int64_t k, const double* M, int64_t ldm, const double* x0, double* x,
                             double* y, int64_t* iters);
int rlhip_drv_pcg_saddle_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, const float* b, const float* c, float delta,
                             int64_t iter_lim, float* resid_vec, float tol, int64_t k, const float* M, int64_t ldm, const float* x0, float* x,
                             float* y, int64_t* iters);
/* rpc_data_svd_saso (comps/rl_preconditioners.hh:135-153; include/RandLAPACK_amd/rl_preconditioners.hh): V_sk (DEVICE, at least d * n entries;
 * on return its leading n x n, ld n, holds the right singular vectors) and sigma_sk (DEVICE, n) from the SVD of a d x m sparse sign sketch
 * (nnz nonzeros per column) of A (m x n, lda, DEVICE).  state[6] (counter, key) in, the next state out. */
int rlhip_drv_rpc_data_svd_saso_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t d, int64_t nnz, const double* A, int64_t lda, double* V_sk,
                                    double* sigma_sk, uint32_t state[6]);
int rlhip_drv_rpc_data_svd_saso_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t d, int64_t nnz, const float* A, int64_t lda, float* V_sk,
                                    float* sigma_sk, uint32_t state[6]);
/* make_right_orthogonalizer (comps/rl_preconditioners.hh:193-224): scales the first *rank columns of V (n x n, ld n, DEVICE) by
 * 1 / sqrt(sigma_i^2 + mu); sigma: DEVICE; cols_V < 0 means n.  *rank receives the number of columns that define the orthogonalizer. */
int rlhip_drv_make_right_orthogonalizer_f64(rlhip_ctx* ctx, int64_t n, double* V, const double* sigma, double mu, int64_t cols_V, int64_t* rank);
int rlhip_drv_make_right_orthogonalizer_f32(rlhip_ctx* ctx, int64_t n, float* V, const float* sigma, float mu, int64_t cols_V, int64_t* rank);
/* sap_lstsq (include/RandLAPACK_amd/rl_lstsq.hh; no reference counterpart): the two calls above with d = ceil(d_factor n) and mu = delta, then
 * pcg_saddle from x0 = 0.  x (n), y (m), resid_vec (iter_lim + 1, may be NULL): DEVICE.  state[6] is advanced as rlhip_drv_rpc_data_svd_saso_*
 * advances it.  *rank and *iters (each may be NULL) receive the orthogonalizer's column count and the iterations run. */
int rlhip_drv_sap_lstsq_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, const double* b, const double* c, double delta,
                            double d_factor, int64_t nnz, double tol, int64_t iter_lim, double* x, double* y, double* resid_vec, uint32_t state[6],
                            int64_t* rank, int64_t* iters);
int rlhip_drv_sap_lstsq_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, const float* b, const float* c, float delta,
                            float d_factor, int64_t nnz, float tol, int64_t iter_lim, float* x, float* y, float* resid_vec, uint32_t state[6],
                            int64_t* rank, int64_t* iters);
/* pcg_saddle_block and the sap_lstsq overload with s right-hand sides (include/RandLAPACK_amd/rl_determiter.hh, rl_lstsq.hh; no
 * reference counterpart): column j runs pcg_saddle's recurrence on (B_j, C_j, X0_j) while all columns share each iteration's one normal product
 * (rlhip_normal_matmat_*).  B, Y: m x s (ldb, ldy); C: n x s (ldc; NULL: zero); X0: n x s (ldx0; NULL: zero); X: n x s (ldx); resid:
 * (iter_lim + 1) x s with stride ldr >= iter_lim + 1 (sap_lstsq_block: stride iter_lim + 1, may be NULL) -- all DEVICE.  iters (HOST, s entries,
 * may be NULL): iterations each column ran; resid[0 .. iters[j], j] are written, the entries below them are left as they were.  s == 0
 * returns 0 and writes nothing (sap_lstsq_block still advances state[6]).  sap_lstsq_block builds ONE preconditioner for all columns and
 * advances state[6] as rlhip_drv_sap_lstsq_* does.  -100 with rlhip_last_error() on a refused argument, a row-sharded context included. */
int rlhip_drv_pcg_saddle_block_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, int64_t s, const double* B, int64_t ldb,
                                   const double* C, int64_t ldc, double delta, int64_t iter_lim, double* resid, int64_t ldr, double tol, int64_t k,
                                   const double* M, int64_t ldm, const double* X0, int64_t ldx0, double* X, int64_t ldx, double* Y, int64_t ldy,
                                   int64_t* iters);
int rlhip_drv_pcg_saddle_block_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, int64_t s, const float* B, int64_t ldb,
                                   const float* C, int64_t ldc, float delta, int64_t iter_lim, float* resid, int64_t ldr, float tol, int64_t k,
                                   const float* M, int64_t ldm, const float* X0, int64_t ldx0, float* X, int64_t ldx, float* Y, int64_t ldy,
                                   int64_t* iters);
int rlhip_drv_sap_lstsq_block_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, int64_t s, const double* B, int64_t ldb,
                                  const double* C, int64_t ldc, double delta, double d_factor, int64_t nnz, double tol, int64_t iter_lim, double* X,
                                  int64_t ldx, double* Y, int64_t ldy, double* resid, uint32_t state[6], int64_t* rank, int64_t* iters);
int rlhip_drv_sap_lstsq_block_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, int64_t s, const float* B, int64_t ldb,
                                  const float* C, int64_t ldc, float delta, float d_factor, int64_t nnz, float tol, int64_t iter_lim, float* X,
                                  int64_t ldx, float* Y, int64_t ldy, float* resid, uint32_t state[6], int64_t* rank, int64_t* iters);
/* The three entries above over an operator descriptor (rlhip_linop_desc, above) in place of (A, lda); m = left->rows, n = left->cols.  Kind 0
 * runs the dense entry; kinds 1, 2, 3 (CSR, CSC, COO) a linops::SparseLinOp: the sketch is the operator's scatter over its nonzeros, every product
 * of the iteration a sparse matrix-vector product (rlhip_csr_spmv_*, rlhip_csr_normal_matvec_*), and A is never densified.  The sign operator, and
 * so state[6] afterwards, are those of a dense A of the same shape.  right must be NULL: a composite operator is refused (-100 and a message), and
 * so is a row-sharded one. */
int rlhip_drv_pcg_saddle_linop_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, const double* b, const double* c,
                                   double delta, int64_t iter_lim, double* resid_vec, double tol, int64_t k, const double* M, int64_t ldm,
                                   const double* x0, double* x, double* y, int64_t* iters);
int rlhip_drv_pcg_saddle_linop_f32(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, const float* b, const float* c,
                                   float delta, int64_t iter_lim, float* resid_vec, float tol, int64_t k, const float* M, int64_t ldm, const float* x0,
                                   float* x, float* y, int64_t* iters);
int rlhip_drv_rpc_data_svd_saso_linop_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, int64_t d, int64_t nnz,
                                          double* V_sk, double* sigma_sk, uint32_t state[6]);
int rlhip_drv_rpc_data_svd_saso_linop_f32(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, int64_t d, int64_t nnz,
                                          float* V_sk, float* sigma_sk, uint32_t state[6]);
int rlhip_drv_sap_lstsq_linop_f64(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, const double* b, const double* c,
                                  double delta, double d_factor, int64_t nnz, double tol, int64_t iter_lim, double* x, double* y, double* resid_vec,
                                  uint32_t state[6], int64_t* rank, int64_t* iters);
int rlhip_drv_sap_lstsq_linop_f32(rlhip_ctx* ctx, const rlhip_linop_desc* left, const rlhip_linop_desc* right, const float* b, const float* c,
                                  float delta, float d_factor, int64_t nnz, float tol, int64_t iter_lim, float* x, float* y, float* resid_vec,
                                  uint32_t state[6], int64_t* rank, int64_t* iters);

#ifdef __cplusplus
}
#endif
#endif
