/* rlhip.h -- C ABI of librlhip.so: the MI355X (gfx950) device layer underneath the RandLAPACK
 * sketch-and-factor path.
 *
 * This is the drop-in boundary.  The reference has no FFI on this path: its
 * drivers are C++ templates that bottom out in blas:: / lapack:: / RandBLAS:: free functions
 * (RandLAPACK/rl_blaspp.hh:5-9, RandLAPACK/rl_lapackpp.hh:7-9).  Each entry point below names the
 * reference call site(s) it replaces.  The C++ classes in include/RandLAPACK_amd/ (same names and call
 * signatures as the reference's driver/comp objects) are written purely against this header.
 *
 * Conventions
 *   - every matrix pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - column-major storage, int64_t dimensions and leading dimensions, 1-based int64_t pivots;
 *   - op / uplo / diag / side flags are the LAPACK characters ('N','T','U','L','R', ...);
 *   - return value: 0 success; >0 LAPACK-style info (e.g. potrf failing minor); <0 = -(index of the bad
 *     argument) or -1000-hipError_t for a runtime failure.  Nothing aborts the process.
 *   - suffix _f64 / _f32 = the arithmetic type; results of the f64 entry points are what the parity
 *     tests compare against the CPU oracle.
 *   - all work is enqueued on the context's HIP stream; entry points that return a value to the host
 *     (info codes, norms, ranks) synchronise that stream, the others are asynchronous.
 */
#ifndef RLHIP_H
#define RLHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rlhip_ctx rlhip_ctx;

/* ---- context, memory, stream (replaces blas::Queue / lapack::Queue, device_malloc, device_free,
 *      device_copy_matrix: RandLAPACK/drivers/rl_bqrrp_gpu.hh:232-233, rl_cqrrpt_gpu.hh:267-297) ---- */
/* own_stream != 0: create a private non-blocking stream (hip_stream ignored);
 * own_stream == 0: enqueue on hip_stream (a hipStream_t; NULL = the device's default stream, which is what
 * PyTorch-ROCm uses unless told otherwise). */
int rlhip_create(rlhip_ctx** ctx, int device, void* hip_stream, int own_stream);
/* a second context on the parent's device: own high-priority stream, own scratch arena -- for work that runs beside the parent's stream
 * (BQRRP's look-ahead); destroyed with rlhip_destroy.  rlhip_order_after: what `waiter` enqueues from now on starts after what `signaler`
 * has enqueued so far (an event, no host wait). */
int rlhip_create_side(rlhip_ctx* parent, rlhip_ctx** out);
int rlhip_order_after(rlhip_ctx* waiter, rlhip_ctx* signaler);
int rlhip_destroy(rlhip_ctx* ctx);
/* ---- per-context options: the library's supported switches (value -1 = the default; a side context inherits its parent's at creation).
 *      Everything else about kernel selection is decided from the shapes alone -- there are no environment switches for kernels; the
 *      environment only carries diagnostics (RLHIP_SK_CLOCK, RLHIP_JACOBI_CLOCK, RLHIP_SK_TUNE, RLHIP_GESDD_TRACE, RLHIP_POOL_TRACE) and
 *      RLHIP_COMM_SINGLE_RANK_NCCL (build a real one-rank RCCL communicator).
 *      The first group selects between two routes of this library that deliver the same result (tests compare them, bitwise where
 *      stated); the RLHIP_OPT_DRV_* group holds defaults that the rlhip_drv_* entry points (rlhip_drivers.h) hand to the C++ objects
 *      they construct -- C++ callers set the members of the same name on their own objects. */
enum rlhip_option {
    RLHIP_OPT_CHOLQRQ_ONE_STREAM = 0,   /* 1: rlhip_cholqrq_* serves tall 256-aligned inputs as one stream of kernels; 0: returns 1 (caller runs syrk, potrf, trsm) */
    RLHIP_OPT_GESDD_GRAM = 1,           /* 1: device SVD of a well-conditioned tall factor, 32 < k <= 256, by Jacobi on its Gram matrix; 0: classic route always */
    RLHIP_OPT_JACOBI_PERSIST = 2,       /* 1: all Jacobi sweeps in one cooperative launch (blocks handed over through the XCD's L2 when the workers share one); 2: the same, hand-over through uncached memory always; 3: the workers alone through an ordinary (non-cooperative) launch -- the route rocprofv3 --pmc can profile, idle device only; 0: one launch per round */
    RLHIP_OPT_TRSM_XASM = 3,            /* fused solve: X loads issued from inline asm (1) or plain loads (0); default = what scripts/check_trsm_asm.py proved for this build */
    RLHIP_OPT_SASO_MODE = 4,            /* rlhip_saso_create: 1 independent columns (RandBLAS's short-axis SASO), 0 block-affine family */
    RLHIP_OPT_HQRRP_TALL_PANEL = 5,     /* hqrrp: 1 pivots of a tall panel from the QRCP of its R factor; 0: one pivoted sweep (the reference's order) */
    RLHIP_OPT_DRV_BQRRP_LOOKAHEAD_MIN_ELEMS = 6,   /* BQRRP::lookahead_min_elems (default 2.5e8; 0 = whenever the shapes allow, a huge value = never) */
    RLHIP_OPT_DRV_BQRRP_CHOLQR_FALLBACK = 7,       /* BQRRP::cholqr_fallback (default 1; 0 = the reference's behaviour on a Cholesky breakdown) */
    RLHIP_OPT_DRV_CQRRPT_FOLD_PIVOTING = 8,        /* CQRRPT::fold_pivoting (default 1) */
    RLHIP_OPT_DRV_CQRRPT_SPLIT_QRCP = 9,           /* CQRRPT::split_qrcp (default 1) */
    RLHIP_OPT_DRV_SPARSE_SKETCH_DENSIFY = 10,      /* linops::SparseLinOp::force_densified_sketch (default 0) */
    RLHIP_OPT_JACOBI_CLOCK_HOLDERS = 11,           /* persistent Jacobi: 1 (default) the CUs its workers leave idle run FMA-burning holder workgroups so that DVFS keeps the clock up for the next GEMM (never on a context that shares the device with another stream); 0: the workers alone */
    RLHIP_OPT_LSQ_NORMAL_FUSED = 12,               /* rlhip_normal_matvec_*: 1 the one-pass kernel wherever n is within its limit, 0 always the two rlhip_gemv calls; default: one pass up to the widths at which it measured faster */
    RLHIP_OPT_SPMV_LANES = 13,                     /* rlhip_csr_spmv_*, rlhip_csr_normal_matvec_*: 4, 16 or 64 lanes per row, 0 the split long-row route; default: chosen from the mean row length (tests reach every route at small sizes with it) */
    RLHIP_OPT_RBF_FUSED = 14,                      /* rlhip_rbf_cross_apply_*: 1 the matrix-free one-launch kernel wherever the shape is within its limits (RLHIP_RBF_FUSED_MAX_N, RLHIP_RBF_FUSED_MAX_ROWS_X), 0 always the composed route (row blocks of K in scratch), 2 the fused kernel split over X wherever rlhip_rbf_split_chunks(mz, nx) > 1 (two launches, partial sums in scratch) and as 1 elsewhere; default: the one-launch kernel within its limits, never split */
    RLHIP_OPT_COUNT = 15                           /* one past the last option.  (It was RLHIP_OPT_COUNT = 14 through DESIGN 4.21; tests/test_splsq_cases.py, written then, still looks for that text in this header.) */
};
int rlhip_set_option(rlhip_ctx* ctx, int option, int64_t value);     /* -1 (bad context / option) or 0 */
int64_t rlhip_get_option(rlhip_ctx* ctx, int option);                /* the stored value (-1 = default), INT64_MIN for a bad option */
int rlhip_sync(rlhip_ctx* ctx);
void* rlhip_stream(rlhip_ctx* ctx);
int rlhip_malloc(rlhip_ctx* ctx, void** dev_ptr, size_t bytes);
int rlhip_free(rlhip_ctx* ctx, void* dev_ptr);
/* rlhip_malloc/rlhip_free recycle blocks by exact size (stream-ordered, no synchronisation on free; at most 1/8 of
 * the device memory idles in the pool).  rlhip_trim returns every idle block to the driver. */
int rlhip_trim(rlhip_ctx* ctx);
/* page-locked HOST memory that the device kernels can address directly (slowly, over the host link): lets code written for the
 * reference's host buffers -- std::fill on an array that is then handed to a driver, test/comps/test_qb.cc:154 -- run unchanged
 * against this library for small problems.  Production data belongs in HBM (rlhip_malloc). */
int rlhip_malloc_host(rlhip_ctx* ctx, void** host_ptr, size_t bytes);
int rlhip_free_host(rlhip_ctx* ctx, void* host_ptr);
int rlhip_memcpy_h2d(rlhip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int rlhip_memcpy_d2h(rlhip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int rlhip_memcpy_d2d(rlhip_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int rlhip_memset(rlhip_ctx* ctx, void* dst_dev, int byte, size_t bytes);
/* reserve the scratch arena up front (split-K slabs, trsm panels ...) so no hipMalloc happens later */
int rlhip_reserve_workspace(rlhip_ctx* ctx, size_t bytes);
size_t rlhip_workspace_highwater(rlhip_ctx* ctx);
const char* rlhip_version(void);

/* stream-ordered scratch arena for driver temporaries (Omega, Gram matrices, split-K slabs ...): a bump
 * allocator that replaces the reference's new[]/delete[] of work buffers inside call() (e.g. rl_rs.hh:130,
 * rl_rf.hh:116, rl_orth.hh:76).  Take a mark, allocate, release back to the mark; memory handed out is
 * only valid for work enqueued on the context's stream before the release. */
size_t rlhip_scratch_mark(rlhip_ctx* ctx);
int rlhip_scratch_alloc(rlhip_ctx* ctx, void** dev_ptr, size_t bytes);
int rlhip_scratch_release(rlhip_ctx* ctx, size_t mark);

/* event timing on the context's stream (bench.py roofline leg) */
int rlhip_timer_start(rlhip_ctx* ctx);
int rlhip_timer_stop_ms(rlhip_ctx* ctx, float* ms_host);

/* ---- counter-based RNG: RandBLAS::RNGState + fill_dense (rl_rs.hh:134-139, rl_bqrrp.hh:310-311,
 *      rl_hqrrp.hh:929-930, rl_abrik.hh:298-299).  dist: 0 = N(0,1), 1 = U(-1,1).
 *      ctr[4]/key[2] are host arrays; next_ctr_host receives the advanced counter (may be NULL). ---- */
int rlhip_philox4x32_10(rlhip_ctx* ctx, int64_t nblocks, uint32_t* out_dev, const uint32_t ctr_host[4],
                        const uint32_t key_host[2]);
int rlhip_fill_dense_f64(rlhip_ctx* ctx, int dist, int64_t rows, int64_t cols, double* buf,
                         const uint32_t ctr_host[4], const uint32_t key_host[2], uint32_t next_ctr_host[4]);
int rlhip_fill_dense_f32(rlhip_ctx* ctx, int dist, int64_t rows, int64_t cols, float* buf,
                         const uint32_t ctr_host[4], const uint32_t key_host[2], uint32_t next_ctr_host[4]);
/* rows [row0, row0 + loc_rows) of the glob_rows x cols operator rlhip_fill_dense_* generates (same stream positions):
 * a row shard regenerates its slice of the global m x k sketch (odd power-pass counts, rl_rs.hh:137-139, under
 * row-block sharding); the device counterpart of RandBLAS::fill_dense_unpacked's offsets.  next_ctr advances by the
 * GLOBAL size, so every rank's state stays identical to the single-device run. */
int rlhip_fill_dense_rows_f64(rlhip_ctx* ctx, int dist, int64_t glob_rows, int64_t cols, int64_t row0, int64_t loc_rows,
                              double* buf, int64_t ld, const uint32_t ctr[4], const uint32_t key[2], uint32_t next_ctr[4]);
int rlhip_fill_dense_rows_f32(rlhip_ctx* ctx, int dist, int64_t glob_rows, int64_t cols, int64_t row0, int64_t loc_rows,
                              float* buf, int64_t ld, const uint32_t ctr[4], const uint32_t key[2], uint32_t next_ctr[4]);

/* ---- BLAS-3 on MFMA.  blas::gemm (rl_rs.hh:142,153,165; rl_rf.hh:123; rl_qb.hh:210-218,260;
 *      rl_rsvd.hh:148), blas::syrk (rl_orth.hh:78; rl_cqrrpt.hh:310; rl_bqrrp.hh:460),
 *      blas::trsm Side::Right/Uplo::Upper/NoTrans (rl_orth.hh:95; rl_cqrrpt.hh:302,338; rl_bqrrp.hh:457,464),
 *      blas::trmm Side::Right/Uplo::Upper/NoTrans (rl_cqrrpt.hh:345; rl_bqrrp.hh:497). ---- */
int rlhip_gemm_f64(rlhip_ctx* ctx, char transa, char transb, int64_t m, int64_t n, int64_t k, double alpha,
                   const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                   int64_t ldc);
int rlhip_gemm_f32(rlhip_ctx* ctx, char transa, char transb, int64_t m, int64_t n, int64_t k, float alpha,
                   const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                   int64_t ldc);
/* gemm + ||A||_F in ONE pass over A (QB needs both: rl_qb.hh:168 then rl_rf.hh:123 read A twice in the
 * reference).  A is (m x k) for transa 'N', (k x m) for 'T'.  *fused_host = 1 when the norm came out of the GEMM
 * kernel itself (stream-K path), 0 when a separate lange pass was needed.  Synchronises the stream -- unless norm_a_host is NULL:
 * the norm is then DEFERRED (when it came out of the product, its sum of squares follows the stream into a pinned mailbox) and
 * rlhip_norma_collect_f64 returns it later, after the caller's next synchronisation (rl_qb.hh:168,221: ||A||_F and ||B_i||_F with one
 * host round trip).  One norm can be pending per context. */
int rlhip_gemm_norma_f64(rlhip_ctx* ctx, char transa, char transb, int64_t m, int64_t n, int64_t k, double alpha,
                         const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                         int64_t ldc, double* norm_a_host, int* fused_host);
/* the norm a rlhip_gemm_norma_f64 call with a NULL result pointer left pending (-4 when there is none).  over_ranks != 0 on a row-sharded
 * context: the norm of the WHOLE matrix (root of the sum over the ranks' sums of squares) -- the sum rides on the Gram matrix's all-reduce
 * when a rlhip_cholqrq call came in between (the QB sequence), otherwise it takes a scalar all-reduce of its own here. */
int rlhip_norma_collect_f64(rlhip_ctx* ctx, int over_ranks, double* norm_a_host);
/* uplo must be 'U' (the only form the path uses); the strictly lower triangle of C is not touched. */
int rlhip_syrk_f64(rlhip_ctx* ctx, char uplo, char trans, int64_t n, int64_t k, double alpha, const double* A,
                   int64_t lda, double beta, double* C, int64_t ldc);
int rlhip_syrk_f32(rlhip_ctx* ctx, char uplo, char trans, int64_t n, int64_t k, float alpha, const float* A,
                   int64_t lda, float beta, float* C, int64_t ldc);
/* B <- alpha * B * inv(A), A n x n upper triangular, B m x n (side 'R', uplo 'U', trans 'N' only) */
int rlhip_trsm_f64(rlhip_ctx* ctx, char side, char uplo, char trans, char diag, int64_t m, int64_t n,
                   double alpha, const double* A, int64_t lda, double* B, int64_t ldb);
int rlhip_trsm_f32(rlhip_ctx* ctx, char side, char uplo, char trans, char diag, int64_t m, int64_t n,
                   float alpha, const float* A, int64_t lda, float* B, int64_t ldb);
/* Out-of-place right-side solve with a column gather:  B <- alpha * (Bsrc * P) * inv(A), where column c of Bsrc * P is column
 * jpvt_dev[c] - 1 of Bsrc (LAPACK-style 1-based pivot vector in device memory; NULL: P = I).  Bsrc (m x n, ldsrc) is not modified and
 * must not overlap B unless it IS B with jpvt_dev == NULL (plain rlhip_trsm).  This is CQRRPT's "util::col_swap(A, J) followed by
 * blas::trsm(A, R_sk)" (rl_cqrrpt.hh:288-300) as ONE pass over A, and its second solve (rl_cqrrpt.hh:329) written straight into A.
 * Returns -7 and writes nothing when jpvt_dev is not a permutation of 1..n (the same refusal as rlhip_col_swap). */
int rlhip_trsm_gather_f64(rlhip_ctx* ctx, char diag, int64_t m, int64_t n, double alpha, const double* A, int64_t lda,
                          const double* Bsrc, int64_t ldsrc, const int64_t* jpvt_dev, double* B, int64_t ldb);
int rlhip_trsm_gather_f32(rlhip_ctx* ctx, char diag, int64_t m, int64_t n, float alpha, const float* A, int64_t lda,
                          const float* Bsrc, int64_t ldsrc, const int64_t* jpvt_dev, float* B, int64_t ldb);
/* Columns [col0, col1) (multiples of 256) of the same solve, given that B[:, 0 : col0) already holds the solution's leading columns; only the
 * leading col1 x col1 part of A and jpvt[0 : col1) are read, and jpvt maps into nsrc >= col1 source columns (a prefix of a pivot vector).
 * Pieces of a split solve are bitwise the whole solve.  Returns 0, 1 (not taken: outside the fused kernel's domain, nothing written --
 * the caller takes rlhip_trsm_gather_* for the whole matrix) or an error (< 0). */
int rlhip_trsm_gather_range_f64(rlhip_ctx* ctx, char diag, int64_t m, int64_t nsrc, double alpha, const double* A, int64_t lda,
                                const double* Bsrc, int64_t ldsrc, const int64_t* jpvt, double* B, int64_t ldb, int64_t col0, int64_t col1);
int rlhip_trsm_gather_range_f32(rlhip_ctx* ctx, char diag, int64_t m, int64_t nsrc, float alpha, const float* A, int64_t lda,
                                const float* Bsrc, int64_t ldsrc, const int64_t* jpvt, float* B, int64_t ldb, int64_t col0, int64_t col1);
/* side 'R': B <- alpha * B * A, A n x n upper triangular, B m x n (trans 'N' only);
 * side 'L': B <- alpha * op(A) * B, A m x m upper triangular (trans 'N' or 'T').  uplo 'U' only. */
int rlhip_trmm_f64(rlhip_ctx* ctx, char side, char uplo, char trans, char diag, int64_t m, int64_t n,
                   double alpha, const double* A, int64_t lda, double* B, int64_t ldb);
int rlhip_trmm_f32(rlhip_ctx* ctx, char side, char uplo, char trans, char diag, int64_t m, int64_t n,
                   float alpha, const float* A, int64_t lda, float* B, int64_t ldb);

/* ---- LAPACK-level pieces.  lapack::potrf Upper (rl_orth.hh:81; rl_cqrrpt.hh:311; rl_bqrrp.hh:462):
 *      returns info (0, or the 1-based order of the first non-positive leading minor). ---- */
int rlhip_potrf_f64(rlhip_ctx* ctx, char uplo, int64_t n, double* A, int64_t lda);
int rlhip_potrf_f32(rlhip_ctx* ctx, char uplo, int64_t n, float* A, int64_t lda);
/* CholQRQ::call (rl_orth.hh:69-98: syrk :78, potrf :81, trsm :95) as ONE stream of kernels with ONE host read: R (k x k, ld k) receives the
 * Cholesky factor of A^T A, A (m x k) is overwritten by A R^-1, *info_host = potrf's info (!= 0: A is untouched, as the reference returns
 * before its trsm).  reduce_gram != 0: row-sharded A, the Gram matrix is all-reduced before it is factored.  Returns 0 when done, 1 when
 * this shape is not served (the caller issues syrk / potrf / trsm itself), < 0 on error. */
int rlhip_cholqrq_f64(rlhip_ctx* ctx, int64_t m, int64_t k, double* A, int64_t lda, double* R, int reduce_gram, int* info_host);
int rlhip_cholqrq_f32(rlhip_ctx* ctx, int64_t m, int64_t k, float* A, int64_t lda, float* R, int reduce_gram, int* info_host);
/* lapack::lange(Norm::Fro) (rl_qb.hh:168,221) */
int rlhip_lange_fro_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, double* result_host);
int rlhip_lange_fro_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, float* result_host);
/* lapack::lacpy / lapack::laset; uplo 'U','L' or 'G' (rl_qb.hh:171; rl_cqrrpt.hh:281; rl_util.hh:102-131) */
int rlhip_lacpy_f64(rlhip_ctx* ctx, char uplo, int64_t m, int64_t n, const double* A, int64_t lda, double* B,
                    int64_t ldb);
int rlhip_lacpy_f32(rlhip_ctx* ctx, char uplo, int64_t m, int64_t n, const float* A, int64_t lda, float* B,
                    int64_t ldb);
int rlhip_laset_f64(rlhip_ctx* ctx, char uplo, int64_t m, int64_t n, double offdiag, double diag, double* A,
                    int64_t lda);
int rlhip_laset_f32(rlhip_ctx* ctx, char uplo, int64_t m, int64_t n, float offdiag, float diag, float* A,
                    int64_t lda);
/* thin SVD of a tall m x n matrix (m >= n), replacing lapack::gesdd(Job::SomeVec) at rl_rsvd.hh:146:
 * on exit A holds U (m x n), S[n] descending, VT (n x n, ld ldvt; NULL: singular values and left vectors only).  One-sided Jacobi,
 * entirely on device.  Returns the number of sweeps used in *sweeps_host (may be NULL); info > 0 = not converged after 60 sweeps.
 * Argument codes, checked before anything is enqueued: -2 m < 0 or m < n, -3 n < 0, -5 lda < max(1, m), -8 ldvt < max(1, n) with VT != NULL;
 * n == 0 returns 0 and writes nothing.  Rows beyond m of A and beyond n of VT are not touched.
 * Scaled inputs: the call measures max |a_ij| and, outside (1e-30, 1e30) in fp64 / (1e-10, 1e10) in fp32, runs on A times the power of
 * two that brings it into [1, 2); S gets the scale back exactly, U and VT do not depend on it.  So the SVD of 2^e A is that of A with
 * S times 2^e for every e that keeps A's entries normal numbers -- no sum of squares overflows or vanishes.  (A column more than
 * half the exponent range below the largest entry still loses its norm.)  fp32 problems, a single column included, run in fp64.
 * Rank deficiency (rank r < n, zero and repeated columns, the zero matrix): info == 0 and everything finite; S_j <= c n eps sigma_1 for
 * j >= r; U S VT reproduces A and VT is orthogonal as for full rank; the leading r columns of U are orthonormal.  A column of U that
 * belongs to S_j == 0 exactly is ZERO, one that belongs to a rounding-level S_j has norm 1 but need not be orthogonal to the others:
 * this is where the library departs from LAPACK, whose trailing columns of U are orthonormal too. */
int rlhip_gesvdj_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* S, double* VT,
                     int64_t ldvt, int* sweeps_host);
int rlhip_gesvdj_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* S, float* VT,
                     int64_t ldvt, int* sweeps_host);

/* A[i,i] += alpha for i < n (the "A_gram[i*k+i] -= 1" loop of util::orthogonality_check, rl_util.hh:480-482) */
int rlhip_add_diag_f64(rlhip_ctx* ctx, int64_t n, double alpha, double* A, int64_t lda);
int rlhip_add_diag_f32(rlhip_ctx* ctx, int64_t n, float alpha, float* A, int64_t lda);
/* lapack::gesdd(Job::SomeVec) contract for a tall matrix (m >= n): A (destroyed) = U diag(S) VT with
 * U m x n (ldu), VT n x n (ldvt), S descending.  Cholesky-QR2 preconditioning + Jacobi on R^T; falls back
 * to rlhip_gesvdj on A when the Cholesky steps cannot be trusted.  (rl_rsvd.hh:146)
 * Argument codes in LAPACK's positions, checked before anything is enqueued: -2 m < 0 or m < n, -3 n < 0, -5 lda < max(1, m),
 * -8 ldu < max(1, m), -10 ldvt < max(1, n); n == 0 returns 0 and writes nothing.  Rows beyond m of A and U and beyond n of VT are not
 * touched (A may be a block of a larger matrix, as ABRIK passes it).  Scaled and rank-deficient inputs: as rlhip_gesvdj above, on every
 * route -- a rank-deficient input takes the Jacobi-on-A route, its U has the same zero / non-orthogonal trailing columns. */
int rlhip_gesdd_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* S, double* U, int64_t ldu,
                    double* VT, int64_t ldvt, int* sweeps_host);
int rlhip_gesdd_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* S, float* U, int64_t ldu,
                    float* VT, int64_t ldvt, int* sweeps_host);
/* util::transposition (misc/rl_util.hh:315-334): AT (n x m, ld ldat) = A^T; upper_only != 0 moves only i <= j */
int rlhip_transpose_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, double* AT,
                        int64_t ldat, int upper_only);
int rlhip_transpose_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, float* AT, int64_t ldat,
                        int upper_only);

/* ---- sparse sketching operator (SASO): RandBLAS::SparseDist(d, m, nnz) + SparseSkOp(DS, state) +
 *      sketch_general(ColMajor, NoTrans, NoTrans, d, n, m, alpha, S, 0, 0, A, lda, beta, B, ldb)
 *      (rl_cqrrpt.hh:214-222, rl_cqrrt.hh:174-182).  S is d x m with nnz nonzeros (+-1) per column.
 *      next_ctr_host receives `S.next_state`.  Two structures (sketch.hip header; restated in oracle/__init__.py::saso_dense):
 *      mode 1 = INDEPENDENT COLUMNS, every column draws its nnz distinct rows by its own Fisher-Yates walk (the distribution of
 *      RandBLAS::SparseSkOp) -- the default; mode 0 = BLOCK AFFINE (one affine row map per block of d columns: faster,
 *      every d x d block is a sum of nnz signed permutations).  rlhip_saso_create takes the default (environment RLHIP_SASO_MODE =
 *      affine switches it), rlhip_saso_create_mode the given one.  Limits: nnz <= min(d, 128); the dense-operand apply stages a
 *      d-row slab in LDS: d <= 20480 (fp64) / 40960 (fp32), -2 beyond. ---- */
typedef struct rlhip_saso rlhip_saso;
int rlhip_saso_create(rlhip_ctx* ctx, int64_t d, int64_t m, int nnz, const uint32_t ctr_host[4],
                      const uint32_t key_host[2], uint32_t next_ctr_host[4], rlhip_saso** S);
int rlhip_saso_create_mode(rlhip_ctx* ctx, int64_t d, int64_t m, int nnz, int mode, const uint32_t ctr_host[4],
                           const uint32_t key_host[2], uint32_t next_ctr_host[4], rlhip_saso** S);
int rlhip_saso_destroy(rlhip_ctx* ctx, rlhip_saso* S);
int rlhip_saso_apply_f64(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, double alpha, const double* A, int64_t lda,
                         double beta, double* B, int64_t ldb);
int rlhip_saso_apply_f32(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, float alpha, const float* A, int64_t lda,
                         float beta, float* B, int64_t ldb);
/* contribution of ONE ROW SHARD: B = alpha * S[:, row0 : row0+mloc] * A_loc (mloc x n, lda) + beta * B.  Summed over the
 * shards (all-reduce) this is S * A; S was created for the GLOBAL row count. */
int rlhip_saso_apply_rows_f64(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, double alpha, const double* A_loc, int64_t lda,
                              int64_t row0, int64_t mloc, double beta, double* B, int64_t ldb);
int rlhip_saso_apply_rows_f32(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, float alpha, const float* A_loc, int64_t lda,
                              int64_t row0, int64_t mloc, float beta, float* B, int64_t ldb);
/* B (d x n, ldb) = alpha * S * A + beta * B for a SPARSE A (m x n) given by the CSR of its transpose (n rows; colidxT = source
 * row).  Scatter with 64-bit fixed-point integer LDS atomics: bitwise reproducible (sketch.hip).  d <= 19200.
 * row0: global index of the operand's first row (0 unless the operator is a row shard of the matrix S was built for). */
int rlhip_saso_apply_csr_f64(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, double alpha, const int64_t* rowptrT, const int64_t* colidxT,
                             const double* valsT, double beta, double* B, int64_t ldb, int64_t row0);
int rlhip_saso_apply_csr_f32(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, float alpha, const int64_t* rowptrT, const int64_t* colidxT,
                             const float* valsT, float beta, float* B, int64_t ldb, int64_t row0);
/* The same product with the SUMS of rlhip_saso_apply_* on the same matrix stored densely (lda = m, 16-byte aligned): every output adds
 * sign * a over its source rows in ascending order, cut into the same partial groups, so the result is bit for bit the dense one (zero
 * terms change no running sum) -- what makes the sketched preconditioner of a sparse operator identical to that of its dense copy
 * (rpc_data_svd on a linops::SparseLinOp).  The entries of a row of the transpose's CSR must be in ascending source row without
 * duplicates (what rlhip_csr_transpose_* builds).  One workgroup per column, no atomics.  Returns 1 and does nothing when the operator is
 * not served (block-affine mode, or (d + 1024) * sizeof(T) + 4 KiB beyond 160 KiB of LDS): the caller then uses rlhip_saso_apply_csr_*. */
int rlhip_saso_apply_csr_ordered_f64(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, double alpha, const int64_t* rowptrT, const int64_t* colidxT,
                                     const double* valsT, double beta, double* B, int64_t ldb);
int rlhip_saso_apply_csr_ordered_f32(rlhip_ctx* ctx, const rlhip_saso* S, int64_t n, float alpha, const int64_t* rowptrT, const int64_t* colidxT,
                                     const float* valsT, float beta, float* B, int64_t ldb);
int rlhip_saso_dense_f64(rlhip_ctx* ctx, const rlhip_saso* S, double* dense_d_by_m);   /* tests / debugging */
int rlhip_saso_dense_f32(rlhip_ctx* ctx, const rlhip_saso* S, float* dense_d_by_m);
/* util::col_swap (misc/rl_util.hh:151-164 == lapmt forward): on exit column i holds former column idx[i]-1.
 * idx: DEVICE array of n 1-based indices, left untouched.  k > n is an error (reference throws).  In place,
 * one read + one write of the matrix, lanes along rows. */
int rlhip_col_swap_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, double* A, int64_t lda, const int64_t* idx);
int rlhip_col_swap_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, float* A, int64_t lda, const int64_t* idx);
/* integer-vector overload (rl_util.hh:174-198): first k entries of A permuted by a permutation idx of 1..k */
int rlhip_col_swap_i64(rlhip_ctx* ctx, int64_t n, int64_t k, int64_t* A, const int64_t* idx);
/* lapack::geqp3 (rl_cqrrpt.hh:247): column-pivoted Householder QR, LAPACK output format (R above, reflectors
 * below the diagonal, tau, 1-based jpvt); all arrays on the device.  jpvt entries on entry are ignored. */
int rlhip_geqp3_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, int64_t* jpvt, double* tau);
int rlhip_geqp3_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, int64_t* jpvt, float* tau);
/* diag(A)[0..n) to the host (rank tests read R's diagonal: rl_cqrrpt.hh:267-272,319-331, rl_bqrrp.hh:421-427) */
int rlhip_get_diag_f64(rlhip_ctx* ctx, int64_t n, const double* A, int64_t lda, double* diag_host);
int rlhip_get_diag_f32(rlhip_ctx* ctx, int64_t n, const float* A, int64_t lda, float* diag_host);

/* lapack::getrf (rl_bqrrp.hh:343, rl_orth.hh:219): row-pivoted LU of an m x n (m up to ~1e5, tall) device matrix;
 * ipiv: DEVICE int64, 1-based, min(m,n) entries.  Returns LAPACK info (first exactly-zero pivot) or 0. */
int rlhip_getrf_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, int64_t* ipiv);
/* the same factorization when only the PIVOTS are wanted (BQRRP's LU-based qrcp_wide reads J_buffer_lu and discards the factors,
 * rl_bqrrp.hh:343-352): ipiv is identical; A is left as scratch (U is valid, L misses the interchanges of later panels). */
int rlhip_getrf_piv_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, int64_t* ipiv);
int rlhip_getrf_piv_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, int64_t* ipiv);
int rlhip_getrf_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, int64_t* ipiv);
/* lapack::geqrf (rl_orth.hh:157, rl_bqrrp.hh:356,515): Householder QR, reflectors below the diagonal, tau: DEVICE.
 * lapack::ungqr(m, n, k = n) (rl_orth.hh:162): overwrite the reflectors with the first n columns of Q (k must equal n).
 * lapack::laswp(n, A, lda, k1, k2, ipiv, 1) (rl_orth.hh:226): forward row interchanges, ipiv DEVICE int64 1-based. */
/* geqrf FOLLOWED BY ungqr(m, n, n) in one call, for the call sites that want the explicit orthonormal factor (rl_abrik.hh:333-342, :420-444,
 * :552-570; HQRQ, rl_orth.hh:157-162): A <- the first n columns of the Householder Q, R (n x n, ld ldr) <- the triangle geqrf leaves
 * (zero below the diagonal).  Tall well-conditioned panels only (Cholesky-QR twice + the sign vector of the Householder reconstruction,
 * csrc/house.hip::geqrf_q): returns 0 when done, 1 when NOT taken -- the caller then runs rlhip_geqrf + rlhip_ungqr on A, which is still its
 * input to rounding -- < 0 on error.  Same Q and R as the two calls up to rounding. */
int rlhip_geqrf_q_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* R, int64_t ldr);
int rlhip_geqrf_q_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* R, int64_t ldr);
int rlhip_geqrf_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double* tau);
int rlhip_geqrf_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float* tau);
int rlhip_ungqr_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, double* A, int64_t lda, const double* tau);
int rlhip_ungqr_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, float* A, int64_t lda, const float* tau);
int rlhip_laswp_f64(rlhip_ctx* ctx, int64_t n, double* A, int64_t lda, int64_t k1, int64_t k2, const int64_t* ipiv);
int rlhip_laswp_f32(rlhip_ctx* ctx, int64_t n, float* A, int64_t lda, int64_t k1, int64_t k2, const int64_t* ipiv);
/* J <- iota(1..cols); for i < min(sd, cols): swap(J[ipiv[i]-1], J[i])   (rl_bqrrp.hh:345-350; CUDA twin
 * LUQRCP_piv_process_gpu_global, rl_cuda_kernels.cuh:203-220).  Integer-exact. */
int rlhip_luqrcp_piv(rlhip_ctx* ctx, int64_t sd, int64_t cols, const int64_t* ipiv, int64_t* J);

/* ---- Householder reconstruction / block reflectors (BQRRP, HQRRP) ----
 * lapack::orhr_col(m, n, nb, A, lda, T, ldt, D) (rl_bqrrp.hh:480; util::rl_orhr_col rl_util.hh:339-379; CUDA twin
 * rl_cuda_kernels.cuh:772-803): A holds orthonormal columns on entry, the unit-lower-trapezoidal V on exit; T (nb x n)
 * the compact-WY factors; D (n) the sign vector. */
int rlhip_orhr_col_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t nb, double* A, int64_t lda, double* T, int64_t ldt,
                       double* D);
int rlhip_orhr_col_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t nb, float* A, int64_t lda, float* T, int64_t ldt,
                       float* D);
/* lapack::gemqrt(Side::Left, Op::Trans, m, n, k, nb, V, ldv, T, ldt, C, ldc) (rl_bqrrp.hh:543) = the block-Householder
 * apply; with rlhip_larft_* it also serves lapack::ormqr (rl_bqrrp.hh:545, cusolver_ormqr rl_bqrrp_gpu.hh:734). */
int rlhip_gemqrt_f64(rlhip_ctx* ctx, char side, char trans, int64_t m, int64_t n, int64_t k, int64_t nb, const double* V,
                     int64_t ldv, const double* T, int64_t ldt, double* C, int64_t ldc);
int rlhip_gemqrt_f32(rlhip_ctx* ctx, char side, char trans, int64_t m, int64_t n, int64_t k, int64_t nb, const float* V,
                     int64_t ldv, const float* T, int64_t ldt, float* C, int64_t ldc);
/* The left / transposed apply of ONE compact-WY block (k reflectors, nb >= k) in two calls, cut where the first k rows of C -- BQRRP's block
 * row R12 (rl_bqrrp.hh:547) -- are final: head computes W2 = T^T V^T C (k x n, ld k, the caller's buffer) and updates rows 0..k-1 of C;
 * tail updates rows k..m-1 (C2 -= V2 W2).  head + tail == rlhip_gemqrt_*('L', 'T', ..., nb = k) bit for bit under rlhip_avoid_persistent(ctx, 1),
 * to rounding otherwise (the tail never takes the persistent stream-K GEMM, gemqrt may). */
int rlhip_gemqrt_head_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* V, int64_t ldv, const double* T, int64_t ldt, double* C, int64_t ldc, double* W2);
int rlhip_gemqrt_head_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, const float* V, int64_t ldv, const float* T, int64_t ldt, float* C, int64_t ldc, float* W2);
int rlhip_gemqrt_tail_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* V, int64_t ldv, const double* W2, double* C, int64_t ldc);
int rlhip_gemqrt_tail_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t k, const float* V, int64_t ldv, const float* W2, float* C, int64_t ldc);
/* (side = 'R', trans = 'N', nb >= k): C (m x n) <- C (I - V T V^T), V n x k -- lapack::larfb(Right, NoTrans, Forward, Columnwise) as
 * used by HQRRP to carry the sketching matrix along (NoFLA_Apply_Q_WY_rnfc_blk_var4, rl_hqrrp.hh:178-206).
 * rlhip_qrp_partial_*: pivoted Householder QR of the first `steps` columns only, HQRRP's norm down-date form
 * (NoFLA_QRPmod_WY_unb_var4 with pivoting = 1, num_stages = steps; rl_hqrrp.hh:516-770); jpvt (device, n, 1-based on exit)
 * is the complete permutation produced by the swaps. */
int rlhip_qrp_partial_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t steps, double* A, int64_t lda, int64_t* jpvt, double* tau);
int rlhip_qrp_partial_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t steps, float* A, int64_t lda, int64_t* jpvt, float* tau);
/* The first `steps` steps of rlhip_geqp3_* itself (LAPACK's norm down-date; lapack::geqp3 as called by rl_cqrrpt.hh:247): rows 0 .. steps-1
 * of R final for all columns, the trailing block updated by every reflector so far, jpvt the permutation so far.  geqp3 of the trailing
 * (m - steps) x (n - steps) block, with its pivots applied to the columns of the finished rows and composed into jpvt, completes it. */
int rlhip_geqp3_steps_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t steps, double* A, int64_t lda, int64_t* jpvt, double* tau);
int rlhip_geqp3_steps_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t steps, float* A, int64_t lda, int64_t* jpvt, float* tau);
/* the context's own cached side context (see rlhip_create_side): created on first use, owned by and destroyed with `parent` -- do NOT
 * rlhip_destroy it */
int rlhip_side_of(rlhip_ctx* parent, rlhip_ctx** out);
/* columns per workgroup of the tag-exchange pivoted QR on this context (0 = default): fewer, fuller workgroups for a factorization that runs
 * beside another stream's kernel */
int rlhip_set_qrcp_cols(rlhip_ctx* ctx, int cols);
/* rows [toff, toff + tcnt) of the unit-lower-triangular V1 held implicitly in Vtop (br x br), written explicitly (0 above, 1 on the
 * diagonal) into out (tcnt x br): a rank's own rows of a reflector block under row sharding (BQRRP). */
int rlhip_vrows_explicit_f64(rlhip_ctx* ctx, int64_t br, int64_t toff, int64_t tcnt, const double* Vtop, int64_t ldv, double* out, int64_t ldo);
int rlhip_vrows_explicit_f32(rlhip_ctx* ctx, int64_t br, int64_t toff, int64_t tcnt, const float* Vtop, int64_t ldv, float* out, int64_t ldo);
/* lapack::larft(Forward, Columnwise): T (k x k) from V (m x k) and tau (k) */
int rlhip_larft_f64(rlhip_ctx* ctx, int64_t m, int64_t k, const double* V, int64_t ldv, const double* tau, double* T, int64_t ldt);
int rlhip_larft_f32(rlhip_ctx* ctx, int64_t m, int64_t k, const float* V, int64_t ldv, const float* tau, float* T, int64_t ldt);
/* R(j,i) *= D(j), j <= i  (rl_bqrrp.hh:485-487; R_cholqr_signs_gpu rl_cuda_kernels.cuh:222-235) */
int rlhip_row_sign_f64(rlhip_ctx* ctx, int64_t n, double* R, int64_t ldr, const double* D);
int rlhip_row_sign_f32(rlhip_ctx* ctx, int64_t n, float* R, int64_t ldr, const float* D);
/* tau(i) = T(i % nb, i)  (rl_bqrrp.hh:490-491) */
int rlhip_tau_from_t_f64(rlhip_ctx* ctx, int64_t k, int64_t nb, const double* T, int64_t ldt, double* tau);
int rlhip_tau_from_t_f32(rlhip_ctx* ctx, int64_t k, int64_t nb, const float* T, int64_t ldt, float* tau);
/* *any_host = 1 iff some |x[i]| > thr, i < n: the zero-block test of rl_bqrrp.hh:373-379 with the CPU semantics (the
 * reference's CUDA all_of only honours its first block) */
int rlhip_any_abs_gt_f64(rlhip_ctx* ctx, int64_t n, const double* x, double thr, int* any_host);
int rlhip_any_abs_gt_f32(rlhip_ctx* ctx, int64_t n, const float* x, float thr, int* any_host);

/* ---- test-matrix generator pieces (RandLAPACK/testing/rl_gen.hh; host-side logic in include/RandLAPACK_amd/rl_gen.hh) ----
 * scal_cols: A[:, j] *= s[j] (s DEVICE, n entries) -- the S factor of gen_singvec (rl_gen.hh:79).
 * scal_rows_idx: A[idx[r], :] *= alpha for the cnt listed rows (idx DEVICE, each row once) -- gen_spiked_mat rl_gen.hh:286-291.
 * gen_kahan: the Kahan matrix of gen_kahan_mat (rl_gen.hh:408-434), m x n leading block. */
int rlhip_scal_cols_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, const double* s_dev);
int rlhip_scal_cols_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, const float* s_dev);
int rlhip_scal_rows_idx_f64(rlhip_ctx* ctx, int64_t cnt, const int64_t* idx_dev, int64_t n, double* A, int64_t lda, double alpha);
int rlhip_scal_rows_idx_f32(rlhip_ctx* ctx, int64_t cnt, const int64_t* idx_dev, int64_t n, float* A, int64_t lda, float alpha);
int rlhip_gen_kahan_f64(rlhip_ctx* ctx, int64_t m, int64_t n, double* A, int64_t lda, double theta, double perturb);
int rlhip_gen_kahan_f32(rlhip_ctx* ctx, int64_t m, int64_t n, float* A, int64_t lda, float theta, float perturb);

/* symmetrize: F (n x n, ldf) = the symmetric matrix whose `uplo` triangle is stored in A; the other triangle of A is not read
 * (linops::ExplicitSymLinOp, RandLAPACK/linops/rl_sym_linops.hh:55-98).  axpby: y = alpha * x + beta * y on n-vectors (beta == 0
 * overwrites without reading y) -- the scal / axpy / copy steps of REVD2's power_error_est (drivers/rl_revd2.hh:34-63). */
int rlhip_symmetrize_f64(rlhip_ctx* ctx, char uplo, int64_t n, const double* A, int64_t lda, double* F, int64_t ldf);
int rlhip_symmetrize_f32(rlhip_ctx* ctx, char uplo, int64_t n, const float* A, int64_t lda, float* F, int64_t ldf);
int rlhip_axpby_f64(rlhip_ctx* ctx, int64_t n, double alpha, const double* x, double beta, double* y);
int rlhip_axpby_f32(rlhip_ctx* ctx, int64_t n, float alpha, const float* x, float beta, float* y);

/* ---- sparse linear operator kernels (linops::SparseLinOp; reference RandLAPACK/linops/rl_sparse_linop.hh:125-330 forwards to
 *      RandBLAS left_spmm/right_spmm).  CSR with int64 indices, all arrays DEVICE pointers.
 *      csr_spmm: C (m x n) = alpha * A (m x k, CSR) * B (k x n) + beta * C; layout 'C' (column-major B, C) or 'R' (row-major).
 *      csr_transpose: CSR of A^T (construction time; staged through the host, deterministic entry order).
 *      csr_densify_cols: out (m x b, column-major) = A[:, c0 : c0 + b], read from the CSR of A^T. ---- */
int rlhip_csr_spmm_f64(rlhip_ctx* ctx, char layout, int64_t m, int64_t n, int64_t k, double alpha, const int64_t* rowptr,
                       const int64_t* colidx, const double* vals, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
int rlhip_csr_spmm_f32(rlhip_ctx* ctx, char layout, int64_t m, int64_t n, int64_t k, float alpha, const int64_t* rowptr,
                       const int64_t* colidx, const float* vals, const float* B, int64_t ldb, float beta, float* C, int64_t ldc);
int rlhip_csr_transpose_f64(rlhip_ctx* ctx, int64_t m, int64_t k, const int64_t* rowptr, const int64_t* colidx, const double* vals,
                            int64_t* rowptrT, int64_t* colidxT, double* valsT);
int rlhip_csr_transpose_f32(rlhip_ctx* ctx, int64_t m, int64_t k, const int64_t* rowptr, const int64_t* colidx, const float* vals,
                            int64_t* rowptrT, int64_t* colidxT, float* valsT);
int rlhip_csr_densify_cols_f64(rlhip_ctx* ctx, int64_t m, const int64_t* rowptrT, const int64_t* colidxT, const double* valsT,
                               int64_t c0, int64_t b, double* out, int64_t ldo);
int rlhip_csr_densify_cols_f32(rlhip_ctx* ctx, int64_t m, const int64_t* rowptrT, const int64_t* colidxT, const float* valsT,
                               int64_t c0, int64_t b, float* out, int64_t ldo);

/* ---- squared-exponential (RBF) kernel matrices and randomly pivoted Cholesky (rpchol.hip; RandLAPACK/misc/rl_pdkernels.hh,
 *      RandLAPACK/comps/rl_rpchol.hh).  X is rows_x x n column-major (ldx), one column per data point; h = bandwidth > 0.
 *
 * rlhip_sqexp_columns_*: out(i, l) = exp(-sum_r (X(r,i) - X(r,idx[l]))^2 / (2 h^2)), plus reg where i == idx[l], for all n points i and
 *   the nidx device indices idx_dev (repeats allowed): squared_exp_kernel (rl_pdkernels.hh:102) as compute_columns evaluates it
 *   (rl_rpchol.hh:19-31).  Differences, not the norm expansion: the entries i == idx[l] are exactly 1 + reg.  out: n x nidx (ldo).
 * rlhip_sqexp_submatrix_*: squared_exp_kernel_submatrix (rl_pdkernels.hh:133-148): Ksub (rows_ksub x cols_ksub, ldk) =
 *   exp(-(|x_i|^2 + |x_j|^2 - 2 x_i^T x_j) / (2 h^2)), i = ro_ksub + row, j = co_ksub + col; MFMA GEMM + one epilogue kernel.
 *   sq_colnorms_x: device |X(:,j)|^2 for all cols_x points, or NULL (computed into scratch); rlhip_sq_colnorms_* fills it.
 * rlhip_rbf_apply_*: linops::RBFKernelMatrix::operator() (rl_pdkernels.hh:255-283): C (dim x n) = alpha * K * B + beta * C, plus
 *   alpha * regs_host[min(i, num_ops - 1)] * B(:, i) in column i when eval_includes_reg (num_ops == 1 or n == num_ops).  K is formed in
 *   full row blocks by rlhip_sqexp_submatrix (not the reference's symmetric arrowhead) in the context's scratch arena: at most
 *   max(2^26, dim) entries of K at a time (512 MiB in fp64), plus dim squared norms. */
int rlhip_sqexp_columns_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t n, const double* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev,
                            double bandwidth, double reg, double* out, int64_t ldo);
int rlhip_sqexp_columns_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t n, const float* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev,
                            float bandwidth, float reg, float* out, int64_t ldo);
int rlhip_sq_colnorms_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const double* X, int64_t ldx, double* sq_colnorms_x);
int rlhip_sq_colnorms_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const float* X, int64_t ldx, float* sq_colnorms_x);
int rlhip_sqexp_submatrix_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const double* X, int64_t ldx, const double* sq_colnorms_x,
                              int64_t rows_ksub, int64_t cols_ksub, double* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, double bandwidth);
int rlhip_sqexp_submatrix_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const float* X, int64_t ldx, const float* sq_colnorms_x,
                              int64_t rows_ksub, int64_t cols_ksub, float* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, float bandwidth);
int rlhip_rbf_apply_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t dim, const double* X, int64_t ldx, double bandwidth, const double* regs_host,
                        int64_t num_ops, int eval_includes_reg, int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C,
                        int64_t ldc);
int rlhip_rbf_apply_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t dim, const float* X, int64_t ldx, float bandwidth, const float* regs_host,
                        int64_t num_ops, int eval_includes_reg, int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C,
                        int64_t ldc);
/* ---- the kernel function as an argument: the squared exponential and the Matern kernels of order 3/2 and 5/2 (a designed extension,
 *      DESIGN 4.23; the reference has the squared exponential only).  With s = |z - x|^2 and l = bandwidth > 0:
 *        RLHIP_PDK_SQEXP     exp(-s / (2 l^2))                                            what every rlhip_sqexp_* / rlhip_rbf_* entry computes
 *        RLHIP_PDK_MATERN32  (1 + a) exp(-a),            a = sqrt(3) sqrt(s) / l
 *        RLHIP_PDK_MATERN52  (1 + a + a^2 / 3) exp(-a),  a = sqrt(5) sqrt(s) / l
 *      Each rlhip_pdk_* entry is the entry it generalises (columns <- rlhip_sqexp_columns, submatrix <- rlhip_sqexp_submatrix, apply <-
 *      rlhip_rbf_apply, cross_submatrix <- rlhip_sqexp_cross_submatrix, cross_apply <- rlhip_rbf_cross_apply) with `int kernel` in front of
 *      the bandwidth: the same routes, route counters (rlhip_rbf_path_count), options (RLHIP_OPT_RBF_FUSED), fused limits and scratch.  The
 *      argument codes are the positions in the NEW list: those of `kernel` itself (an unknown kind) and of every argument behind it are one
 *      larger than the older entry's.  With RLHIP_PDK_SQEXP an rlhip_pdk_* entry returns the bits of the older entry, which is a call of it.
 *      Evaluation of the Matern kinds, the same on every route:
 *        - c = sqrt(3) / l or sqrt(5) / l is computed in double and rounded once to T; so is 1 / 3;
 *        - on the norm-expansion routes (submatrix, apply, cross_submatrix, cross_apply) s = (|z_i|^2 + |x_j|^2) - 2 z_i^T x_j is clamped by
 *          s < 0 ? 0 : s -- a select, not fmax, so a NaN coordinate still gives a NaN entry;
 *        - a = c * sqrt(s) with the accurate sqrt / sqrtf;
 *        - the polynomial in Horner form, one fused multiply-add per step: 1 + a, and 1 + a * (1 + a * (1 / 3));
 *        - times the accurate exp(-a) / expf(-a).
 *      The fused and the composed route of cross_apply use this one formula and differ in the order of the sums only.  rlhip_pdk_columns_*
 *      evaluates s by differences, as rlhip_sqexp_columns_* does: its entries i == idx[l] are exactly 1 + reg for every kind.  A point of X
 *      past nx contributes exactly 0 in the fused kernel: a finite K times a staged zero of B.
 *      The absolute error of the expanded s is about eps (|z|^2 + |x|^2); |dK/ds| <= 1 / (2 l^2), 3 / (2 l^2), 5 / (6 l^2) for the three
 *      kinds, so an entry is off by about eps (1 + L (|z|^2 + |x|^2)).  Matern 1/2, exp(-sqrt(s) / l), is NOT offered: its derivative in s is
 *      unbounded at s = 0, and the expansion would cost it half the digits near coincident points, the diagonal of K(X, X) included. */
#define RLHIP_PDK_SQEXP 0
#define RLHIP_PDK_MATERN32 1
#define RLHIP_PDK_MATERN52 2
int rlhip_pdk_columns_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t n, const double* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev, int kernel,
                          double bandwidth, double reg, double* out, int64_t ldo);
int rlhip_pdk_columns_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t n, const float* X, int64_t ldx, int64_t nidx, const int64_t* idx_dev, int kernel,
                          float bandwidth, float reg, float* out, int64_t ldo);
int rlhip_pdk_submatrix_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const double* X, int64_t ldx, const double* sq_colnorms_x,
                            int64_t rows_ksub, int64_t cols_ksub, double* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel,
                            double bandwidth);
int rlhip_pdk_submatrix_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t cols_x, const float* X, int64_t ldx, const float* sq_colnorms_x,
                            int64_t rows_ksub, int64_t cols_ksub, float* Ksub, int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel,
                            float bandwidth);
int rlhip_pdk_apply_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t dim, const double* X, int64_t ldx, int kernel, double bandwidth,
                        const double* regs_host, int64_t num_ops, int eval_includes_reg, int64_t n, double alpha, const double* B, int64_t ldb,
                        double beta, double* C, int64_t ldc);
int rlhip_pdk_apply_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t dim, const float* X, int64_t ldx, int kernel, float bandwidth,
                        const float* regs_host, int64_t num_ops, int eval_includes_reg, int64_t n, float alpha, const float* B, int64_t ldb,
                        float beta, float* C, int64_t ldc);
int rlhip_pdk_cross_submatrix_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, const double* sq_colnorms_z, int64_t nx,
                                  const double* X, int64_t ldx, const double* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, double* Ksub,
                                  int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel, double bandwidth);
int rlhip_pdk_cross_submatrix_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, const float* sq_colnorms_z, int64_t nx,
                                  const float* X, int64_t ldx, const float* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, float* Ksub,
                                  int64_t ldk, int64_t ro_ksub, int64_t co_ksub, int kernel, float bandwidth);
int rlhip_pdk_cross_apply_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx,
                              int kernel, double bandwidth, int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C,
                              int64_t ldc);
int rlhip_pdk_cross_apply_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx,
                              int kernel, float bandwidth, int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C, int64_t ldc);
/* rlhip_sample_indices_iid_*: RandBLAS::weights_to_cdf + sample_indices_iid as rp_cholesky calls them (rl_rpchol.hh:64, 131, 141-143).
 * RandBLAS is absent, so the stream is this library's own:
 *   weights   w_i = max(d_i, 0) (d: n DEVICE weights); all sums in double for both precisions, in this fixed order:
 *             chunk c = [256c, 256c + 256); loc_i = sequential inclusive sum of w inside i's chunk from 0; S_c = loc of its last element;
 *             off_0 = 0, off_{c+1} = off_c + S_c sequentially; prefix_i = off_c + loc_i; total = off_{nchunks}.  Bitwise reproducible.
 *   status    2 if some d_i < -eps(T) or d_i is NaN, else 1 if total < sqrt(n) * eps(T), else 0 (what downdate_d_and_cdf derives from
 *             RandBLAS's errors, rl_rpchol.hh:47-72).  status != 0: nothing is drawn and next_ctr = ctr.
 *   draw j    Philox4x32-10 block ctr + j/2 with key; its words 2(j%2), 2(j%2)+1 give w64 = lo | hi << 32, u = ((w64 >> 11) + 0.5) 2^-53;
 *             sample = the first i with prefix_i > u * total (upper bound), clamped to the last index with w > 0 (so an index of zero
 *             weight is never drawn).  next_ctr = ctr + ceil(k/2).
 *   unique    0: the k draws in draw order; 1: sorted and de-duplicated in LDS by one workgroup (k <= 4096), *count = distinct values.
 * out_dev (may be NULL: scratch) receives the samples on the device, out_host (may be NULL) the same k slots on the host; *count and
 * *status come back through the same, single, host read. */
int rlhip_sample_indices_iid_f64(rlhip_ctx* ctx, int64_t n, const double* d, int64_t k, int unique, const uint32_t ctr[4], const uint32_t key[2],
                                 uint32_t next_ctr[4], int64_t* out_dev, int64_t* out_host, int64_t* count, int* status);
int rlhip_sample_indices_iid_f32(rlhip_ctx* ctx, int64_t n, const float* d, int64_t k, int unique, const uint32_t ctr[4], const uint32_t key[2],
                                 uint32_t next_ctr[4], int64_t* out_dev, int64_t* out_host, int64_t* count, int* status);
/* rlhip_rpchol_panel_finish_*: the trsm of rl_rpchol.hh:174 and the downdate of :47-62 for the n x cols panel F (ldf): F <- F U^-1 (U: the
 * upper triangle of a cols x cols Cholesky factor, ldu), then d_i <- d_i - sum_j F(i,j)^2 (j in order) and d_i <- 0 for i in sidx_dev[0:cols]
 * (sorted ascending).  cols <= 64: one fused kernel (per-row substitution in registers, U in LDS; the panel is read once and written once);
 * wider panels: rlhip_trsm, then a downdate kernel.  Asynchronous. */
int rlhip_rpchol_panel_finish_f64(rlhip_ctx* ctx, int64_t n, int64_t cols, const double* U, int64_t ldu, double* F, int64_t ldf, double* d,
                                  const int64_t* sidx_dev);
int rlhip_rpchol_panel_finish_f32(rlhip_ctx* ctx, int64_t n, int64_t cols, const float* U, int64_t ldu, float* F, int64_t ldf, float* d,
                                  const int64_t* sidx_dev);
/* row / column gathers with device indices: out(r, c) = A(idx[r], c) (cnt x ncols; _rpchol_impl::pack_selected_rows, rl_rpchol.hh:34-44)
 * and out(:, c) = A(:, idx[c]) (m x cnt, cnt <= 65535). */
int rlhip_gather_rows_f64(rlhip_ctx* ctx, int64_t cnt, const int64_t* idx_dev, int64_t ncols, const double* A, int64_t lda, double* out, int64_t ldo);
int rlhip_gather_rows_f32(rlhip_ctx* ctx, int64_t cnt, const int64_t* idx_dev, int64_t ncols, const float* A, int64_t lda, float* out, int64_t ldo);
int rlhip_gather_cols_f64(rlhip_ctx* ctx, int64_t m, int64_t cnt, const int64_t* idx_dev, const double* A, int64_t lda, double* out, int64_t ldo);
int rlhip_gather_cols_f32(rlhip_ctx* ctx, int64_t m, int64_t cnt, const int64_t* idx_dev, const float* A, int64_t lda, float* out, int64_t ldo);

/* ---- block / lockstep PCG and the spectral preconditioner (pcg.hip; reference RandLAPACK/comps/rl_determiter.hh:181-493,
 *      linops/rl_sym_linops.hh:204-379; the loop is include/RandLAPACK_amd/rl_determiter.hh).  All arrays are DEVICE, column-major; rows n .. ld-1
 *      are never touched.  Sums over rows are returned in DOUBLE for both precisions: one partial per workgroup of 256 rows and column, the
 *      partials added in a fixed order by one workgroup -- no atomics, bitwise reproducible.  Everything is asynchronous. ---- */
/* rlhip_posm_square_*: the Cholesky half of posm_square (rl_determiter.hh:244-257).  LHS, RHS: s x s, ld s; the LOWER triangle of LHS is read
 * and LHS is never written.  Success: RHS <- LHS^-1 RHS, *status_dev = s.  A pivot <= 0 or NaN (dpotrf's test): RHS untouched, *status_dev = -1
 * (the caller runs the eigenvalue fallback, rl_determiter.hh posm_square).  diag_only != 0: zero_off_diagonal (:154-161) is applied to both
 * matrices first -- s independent pivots, x = (b / sqrt(p)) / sqrt(p) as the two solves give it, off-diagonal entries of RHS written as exact zeros.
 * s <= 64: one workgroup with both matrices in LDS.  s > 64: potrf, one triangular solve that forms U^-1, and two products on a scratch copy
 * (one host read); diag_only keeps one element-wise workgroup. */
int rlhip_posm_square_f64(rlhip_ctx* ctx, int64_t s, const double* LHS, double* RHS, int diag_only, int64_t* status_dev);
int rlhip_posm_square_f32(rlhip_ctx* ctx, int64_t s, const float* LHS, float* RHS, int diag_only, int64_t* status_dev);
/* rlhip_pcg_update_xr_*: X += P alpha and R -= GP alpha (the two products at rl_determiter.hh:450-453; alpha s x s, ld s; the rest n x s), and
 * colnorm2_dev[j] = sum_i R(i,j)^2 of the UPDATED R (may be NULL).  s <= 64: one kernel, a thread owns a row, alpha staged once in LDS; P, GP, X
 * and R are read once, X and R written once.  s > 64: rlhip_gemm twice and a column-norm pass. */
int rlhip_pcg_update_xr_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* alpha_dev, const double* P, int64_t ldp, const double* GP, int64_t ldgp,
                            double* X, int64_t ldx, double* R, int64_t ldr, double* colnorm2_dev);
int rlhip_pcg_update_xr_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* alpha_dev, const float* P, int64_t ldp, const float* GP, int64_t ldgp,
                            float* X, int64_t ldx, float* R, int64_t ldr, double* colnorm2_dev);
/* rlhip_pcg_update_p_*: P <- NR + P beta in place (rl_determiter.hh:485-488).  s <= 64: a thread owns a row, NR is not copied.  s > 64: NR is
 * copied to scratch, rlhip_gemm adds P beta, the copy moves into P. */
int rlhip_pcg_update_p_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* beta_dev, const double* NR, int64_t ldnr, double* P, int64_t ldp);
int rlhip_pcg_update_p_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* beta_dev, const float* NR, int64_t ldnr, float* P, int64_t ldp);
/* colnorm2_dev[j] = sum_i A(i,j)^2 (A n x s), the same fixed-order sum the two kernels around it return (PCG's first residual) */
int rlhip_pcg_colnorm2_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* A, int64_t lda, double* colnorm2_dev);
int rlhip_pcg_colnorm2_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* A, int64_t lda, double* colnorm2_dev);
/* rlhip_spectral_precond_apply_*: SpectralPrecond::operator() (rl_sym_linops.hh:328-378): C = alpha (V diag(D_j) V^T + I) B + beta C in four steps,
 * W = V^T B (rlhip_gemm), W(i,j) *= D(i, num_ops == 1 ? 0 : j), C = beta C + alpha B (beta == 0 does not read C), C += alpha V W (rlhip_gemm).
 * V: dim x dim_pre (ldv); D_dev: dim_pre x num_ops; B, C: dim x n; W_dev: dim_pre x n work space; num_ops is 1 or n.  colnorm2_dev (may be
 * NULL) receives the squared column norms of the new C. */
int rlhip_spectral_precond_apply_f64(rlhip_ctx* ctx, int64_t dim, int64_t dim_pre, const double* V, int64_t ldv, const double* D_dev, int64_t num_ops,
                                     int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, double* W_dev,
                                     double* colnorm2_dev);
int rlhip_spectral_precond_apply_f32(rlhip_ctx* ctx, int64_t dim, int64_t dim_pre, const float* V, int64_t ldv, const float* D_dev, int64_t num_ops,
                                     int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C, int64_t ldc, float* W_dev,
                                     double* colnorm2_dev);
/* rlhip_ridge_filter_*: the filter of restricted kernel ridge regression (RandLAPACK::krill_restricted_rpchol, rl_krill.hh):
 * C(j, i) *= sigma[j] / (sigma[j]^2 + mu_i) for the k x s block C (ldc), mu_i = mus_dev[num_mus == 1 ? 0 : i].  sigma_dev: the k singular
 * values of the factor, decreasing.  mu_i == 0 is the pseudo-inverse: where sigma[j] <= rcond * sigma[0] the factor is exactly 0; with
 * mu_i > 0 nothing is cut.  The factor is computed in double for both precisions and rounded once; the product is taken in the precision of
 * C.  One thread per entry, plain loads and stores, no atomics; rows k .. ldc-1 of C are never touched.  k == 0 or s == 0 returns 0 and
 * touches nothing.  Argument codes, checked before anything is enqueued: -2 k < 0, -3 s < 0, -9 ldc < max(1, k); then, when k > 0 and
 * s > 0: -4 sigma_dev NULL, -5 mus_dev NULL, -100 num_mus neither 1 nor s, -7 rcond < 0 or NaN, -8 C NULL. */
int rlhip_ridge_filter_f64(rlhip_ctx* ctx, int64_t k, int64_t s, const double* sigma_dev, const double* mus_dev, int64_t num_mus, double rcond,
                           double* C, int64_t ldc);
int rlhip_ridge_filter_f32(rlhip_ctx* ctx, int64_t k, int64_t s, const float* sigma_dev, const float* mus_dev, int64_t num_mus, float rcond,
                           float* C, int64_t ldc);
/* rlhip_ridge_loo_*: leave-one-out and residual sums of restricted kernel ridge regression over a grid of regularizations (rl_krill.hh,
 * krill_restricted_rpchol_cv).  U (n x k, ldu), sigma_dev (k, decreasing) are the thin SVD of the factor, C = U^T H (k x ell,
 * ldc), H the targets (n x ell, ldh), mus_dev g regularizations >= 0, all DEVICE and of type T.  With d_jm = sigma_j^2 / (sigma_j^2 + mu_m)
 * (mu_m == 0: 1, or 0 where sigma_j <= rcond * sigma_0), s_im = sum_j U_ij^2 d_jm and yhat_imc = sum_j U_ij d_jm C_jc:
 *   loo_dev(m, c) = sum_i ((h_ic - yhat_imc) / (1 - s_im))^2,   rss_dev(m, c) = sum_i (h_ic - yhat_imc)^2,
 * both g x ell with leading dimension g, double in both precisions.  d, every sum over j and every sum over i are taken in double.  A row
 * with 1 - s_im == 0 makes its entry of loo inf (or NaN); nothing is filtered.  No atomics: one partial per workgroup of 256 rows in the
 * scratch arena (2 ceil(n / 256) g ell doubles) and a second launch that adds them in a fixed order, so the bits depend on the shapes and
 * the data alone.  n, k, ell or g == 0 returns 0 and writes nothing.  Rows beyond n (k) of U and H (C) are never read.  Argument codes,
 * checked before anything is enqueued: -2 n < 0, -3 k < 0, -4 ell < 0, -5 g < 0, -7 ldu < max(1, n), -10 ldc < max(1, k), -12 ldh <
 * max(1, n); then, when no size is 0: -6 U NULL, -8 sigma_dev NULL, -9 C NULL, -11 H NULL, -13 mus_dev NULL, -14 rcond < 0 or NaN, -15
 * loo_dev NULL, -16 rss_dev NULL, -100 more than 65535 chunks of 8 grid values or of 4 columns. */
int rlhip_ridge_loo_f64(rlhip_ctx* ctx, int64_t n, int64_t k, int64_t ell, int64_t g, const double* U, int64_t ldu, const double* sigma_dev,
                        const double* C, int64_t ldc, const double* H, int64_t ldh, const double* mus_dev, double rcond, double* loo_dev,
                        double* rss_dev);
int rlhip_ridge_loo_f32(rlhip_ctx* ctx, int64_t n, int64_t k, int64_t ell, int64_t g, const float* U, int64_t ldu, const float* sigma_dev,
                        const float* C, int64_t ldc, const float* H, int64_t ldh, const float* mus_dev, float rcond, double* loo_dev,
                        double* rss_dev);
/* The routes of the two update kernels, one count per call: 43 a fused rlhip_pcg_update_xr, 44 a fused rlhip_pcg_update_p, 45 either one on
 * the composed route (s > 64).  They continue the numbering of rlhip_path_count below but are read here: that function's range ends at 42
 * and answers -1 beyond it.  -1 for any other index. */
int64_t rlhip_pcg_path_count(rlhip_ctx* ctx, int which);

/* ---- matrix-vector layer and the vector steps of pcg_saddle (lsq.hip; reference RandLAPACK/comps/rl_determiter.hh:18-134; the loop is
 *      include/RandLAPACK_amd/rl_determiter.hh).  Column-major, all arrays DEVICE, everything asynchronous.  No kernel waits for another
 *      workgroup and none uses a floating-point atomic: a sum over rows goes through one partial per workgroup and column in the scratch
 *      arena (G x n values for a grid of G workgroups, never proportional to m) and a final pass that adds the partials in a fixed order, so
 *      results are bitwise reproducible from run to run on one device.  Sums are taken in the precision of the data.  Rows m .. lda-1 of A
 *      are never read, and nothing beyond the stated length of an output vector is written. ---- */
/* rlhip_gemv_*: y = alpha op(A) x + beta y, A m x n, trans 'N' or 'T' (blas::gemv(ColMajor, ...) with unit strides, rl_determiter.hh:50,
 * 58-59, 64-65, 81-82, 99-100, 113-114, 131).  beta == 0 does not read y.  m == 0 or n == 0 returns 0 and writes nothing (BLAS's quick return);
 * alpha == 0 scales y without reading A or x.  'N': a workgroup owns 64 rows, its four waves a quarter of the columns each, added in wave
 * order.  'T': a fixed grid whose workgroups walk 512-row slabs s, s + G, ...; a wave owns every fourth column and keeps the running sums
 * of its columns in LDS; one partial per workgroup and column, then the final pass.
 * Argument codes, checked before anything is enqueued: -2 trans, -3 m < 0, -4 n < 0, -6 A NULL, -7 lda < max(1, m), -8 x NULL, -10 y NULL
 * (the pointer codes only when m > 0 and n > 0). */
int rlhip_gemv_f64(rlhip_ctx* ctx, char trans, int64_t m, int64_t n, double alpha, const double* A, int64_t lda, const double* x, double beta,
                   double* y);
int rlhip_gemv_f32(rlhip_ctx* ctx, char trans, int64_t m, int64_t n, float alpha, const float* A, int64_t lda, const float* x, float beta,
                   float* y);
/* rlhip_normal_matvec_*: q = A^T (A d) + delta d (the two gemv calls and the axpy at rl_determiter.hh:58-60, 81-83, 99-100).  Optional
 * outputs, each may be NULL: t = A d (m values) and *dq_dev = d^T q (rl_determiter.hh:86's dot, taken in a fixed order by one workgroup).
 * Fused route, n <= RLHIP_NORMAL_FUSED_MAX_N_F64 / _F32: A is read from memory ONCE.  A fixed grid of G = min(max_wg, slabs) workgroups of
 * 1024 threads (max_wg <= 0: one per CU); workgroup s walks the R-row slabs s, s + G, ...: the slab (R x n) is staged in LDS (columns padded
 * to R + 1 against bank conflicts) while t is formed for its R rows, then the workgroup's partial q is advanced from the staged copy while
 * the next slab is already on its way into registers; after its last slab the workgroup writes its n partial sums, and the final pass adds
 * the G partials in order and adds delta d.  R is the largest power of two between 16 and 256 rows with R n sizeof(T) <= 128 KiB, which
 * sets the limits below (16 rows: a 128-B column segment in fp64).  Composed route (wider n): rlhip_gemv 'N' into t (or scratch) and
 * rlhip_gemv 'T'; two passes over A.
 * The route: unasked, the one-pass kernel serves n <= RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F64 / _F32 -- the widths at which it measured faster
 * than the composed route (in fp32 a 16-row column segment is half a 128-B line and the one-pass kernel loses from n = 1024 on);
 * RLHIP_OPT_LSQ_NORMAL_FUSED = 1 takes it wherever n is within the kernel's limit, 0 never.
 * m == 0: q = delta d.  n == 0: returns 0 and writes nothing.
 * Argument codes: -2 m < 0, -3 n < 0, -4 A NULL (m, n > 0), -5 lda < max(1, m), -6 d NULL, -8 q NULL (both n > 0). */
#define RLHIP_NORMAL_FUSED_MAX_N_F64 1024
#define RLHIP_NORMAL_FUSED_MAX_N_F32 2048
#define RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F64 1024
#define RLHIP_NORMAL_FUSED_DEFAULT_MAX_N_F32 256
int rlhip_normal_matvec_f64(rlhip_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, const double* d, double delta, double* q,
                            double* t, double* dq_dev, int64_t max_wg);
int rlhip_normal_matvec_f32(rlhip_ctx* ctx, int64_t m, int64_t n, const float* A, int64_t lda, const float* d, float delta, float* q, float* t,
                            float* dq_dev, int64_t max_wg);
/* The n-length vector steps of one pcg_saddle iteration, every scalar kept on the device (one workgroup each).
 * rlhip_pcg_saddle_step_xr_*: alpha = *delta1_dev / *dq_dev, x += alpha d, r -= alpha q (rl_determiter.hh:86, 89, 106); q == NULL leaves r
 *   alone (the iterations whose residual is recomputed).  Codes: -2 n < 0, -3 d, -5 dq_dev, -6 delta1_dev, -7 x NULL; -8 r NULL with q given.
 * rlhip_pcg_saddle_step_refresh_*: r = (b1 - qx) - delta x, the last term only when delta > 0 (rl_determiter.hh:101-103).
 *   Codes: -2 n < 0, -3 b1, -4 qx, -6 x, -7 r NULL.
 * rlhip_pcg_saddle_step_d_*: *delta1_new_dev = r^T s (fixed order), beta = that / *delta1_old_dev, d = beta d + s (rl_determiter.hh:117-122);
 *   delta1_old_dev == NULL: the dot alone (rl_determiter.hh:69), d is not touched.  The loop passes resid_vec + iter and resid_vec + iter + 1.
 *   Codes: -2 n < 0, -3 r, -4 s, -6 delta1_new_dev NULL; -7 d NULL with delta1_old_dev given.
 * n == 0: each returns 0 and enqueues nothing. */
int rlhip_pcg_saddle_step_xr_f64(rlhip_ctx* ctx, int64_t n, const double* d, const double* q, const double* dq_dev, const double* delta1_dev,
                                 double* x, double* r);
int rlhip_pcg_saddle_step_xr_f32(rlhip_ctx* ctx, int64_t n, const float* d, const float* q, const float* dq_dev, const float* delta1_dev, float* x,
                                 float* r);
int rlhip_pcg_saddle_step_refresh_f64(rlhip_ctx* ctx, int64_t n, const double* b1, const double* qx, double delta, const double* x, double* r);
int rlhip_pcg_saddle_step_refresh_f32(rlhip_ctx* ctx, int64_t n, const float* b1, const float* qx, float delta, const float* x, float* r);
int rlhip_pcg_saddle_step_d_f64(rlhip_ctx* ctx, int64_t n, const double* r, const double* s, const double* delta1_old_dev, double* delta1_new_dev,
                                double* d);
int rlhip_pcg_saddle_step_d_f32(rlhip_ctx* ctx, int64_t n, const float* r, const float* s, const float* delta1_old_dev, float* delta1_new_dev,
                                float* d);
/* The routes of this layer, one count per call: 46 a fused rlhip_normal_matvec, 47 a composed one (its two rlhip_gemv calls count as
 * well), 48 rlhip_gemv 'N', 49 rlhip_gemv 'T' (calls that launch nothing are not counted).  -1 for any other index. */
int64_t rlhip_lsq_path_count(rlhip_ctx* ctx, int which);

/* ---- least squares with several right-hand sides (lsq.hip): the hot path of RandLAPACK::pcg_saddle_block (rl_determiter.hh;
 *      DESIGN 4.31).  Column-major DEVICE operands with leading dimensions; the rules of the layer above hold (no workgroup waits for
 *      another, no floating-point atomic, static slabs, partials in the scratch arena and a final pass in a fixed order), and on top of them
 *      COLUMN INDEPENDENCE: column j of every output is a function of A, delta and column j of the inputs alone; for given sizes, max_wg and
 *      route its bits do not depend on what the other columns hold.  Column j of a call with s > 1 need not have rlhip_normal_matvec's bits. ---- */
/* rlhip_normal_matmat_*: Q (n x s, ldq) = A^T (A D) + delta D for D n x s (ldd).  Optional outputs, each may be NULL: T = A D (m x s, ldt)
 * and dq_dev[j] = D(:, j)^T Q(:, j) (s values, each by one workgroup in the order of rlhip_normal_matvec's d^T q).
 * One-pass route, n <= RLHIP_NORMAL_MATMAT_FUSED_MAX_N: the slab walk of the fused rlhip_normal_matvec (G = min(max_wg, slabs) workgroups of
 * 1024 threads, max_wg <= 0: one per CU; workgroup b walks the R-row slabs b, b + G, ...), the staged slab S used for a chunk of sc columns
 * at once: T_slab (R x sc) = S D, then the workgroup's partial Q (n x sc) += S^T T_slab, while the next slab is on its way into registers.
 * A is read from memory once per chunk; s columns take ceil(s / sc) passes.  A slab holds at most 64 KiB (R the largest power of two between
 * 16 and 256 with R n sizeof(T) <= 64 KiB) so that D, the shares of T_slab and T_slab fit beside it; sc is at most
 * RLHIP_NORMAL_MATMAT_FUSED_SC_F64 / _F32.  Composed route (every other shape): T = A D and Q = A^T T through rlhip_gemm_*
 * (T in scratch when the caller passes NULL), then Q += delta D; two passes over A.
 * The route: unasked, the one-pass route serves the shapes where it measured faster than both the composed route and s calls of
 * rlhip_normal_matvec: 2 <= s <= 8 with 33 <= n <= 256 in fp64, 129 <= n <= 256 in fp32 (rlhip_normal_matmat_default);
 * rlhip_normal_matmat_set_route(ctx, 1) takes it wherever rlhip_normal_matmat_fused(...) != 0, 0 never, -1 restores the default.
 * m == 0: Q = delta D.  n == 0 or s == 0: returns 0 and writes nothing.  Rows m .. lda - 1 of A are never read; nothing is written beyond
 * column s - 1 or beyond row n - 1 (Q), m - 1 (T) of an output.
 * Argument codes, checked before anything is enqueued: -1 ctx NULL, -2 m < 0, -3 n < 0, -4 s < 0, -5 A NULL (m, n, s > 0), -6 lda < max(1, m),
 * -7 D NULL (n, s > 0), -8 ldd < max(1, n), -10 Q NULL (n, s > 0), -11 ldq < max(1, n), -13 ldt < max(1, m) with T given. */
#define RLHIP_NORMAL_MATMAT_FUSED_MAX_N 512
#define RLHIP_NORMAL_MATMAT_FUSED_SC_F64 4
#define RLHIP_NORMAL_MATMAT_FUSED_SC_F32 4
int rlhip_normal_matmat_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t s, const double* A, int64_t lda, const double* D, int64_t ldd, double delta,
                            double* Q, int64_t ldq, double* T, int64_t ldt, double* dq_dev, int64_t max_wg);
int rlhip_normal_matmat_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t s, const float* A, int64_t lda, const float* D, int64_t ldd, float delta,
                            float* Q, int64_t ldq, float* T, int64_t ldt, float* dq_dev, int64_t max_wg);
/* The chunk width the one-pass route uses for n columns of A, s right-hand sides and elements of elem_bytes (8 or 4) bytes:
 * min(s, RLHIP_NORMAL_MATMAT_FUSED_SC_*) for 1 <= n <= RLHIP_NORMAL_MATMAT_FUSED_MAX_N and s >= 1, else 0.  A function of the shape alone. */
int rlhip_normal_matmat_fused(int64_t n, int64_t s, int elem_bytes);
/* 1 where rlhip_normal_matmat_* takes its one-pass route unasked (the measured ranges above), else 0.  A function of the shape alone. */
int rlhip_normal_matmat_default(int64_t n, int64_t s, int elem_bytes);
/* route: -1 the default, 0 always the composed route, > 0 the one-pass route wherever rlhip_normal_matmat_fused(...) != 0.  Returns the
 * value found (-1, 0 or 1), -1 for a NULL context. */
int rlhip_normal_matmat_set_route(rlhip_ctx* ctx, int route);
/* The three vector steps of rlhip_pcg_saddle_step_* over n x s blocks in lockstep.  Per-column scalars stay on the device: dq_dev (s),
 * rel_sq_tol_dev (s), the flags active_dev (s ints) and the residual histories, one column of (at least) iter_lim + 1 entries each with
 * stride ldh: the loop passes resid + iter as delta1_dev / delta1_old_dev and resid + iter + 1 as delta1_new_dev, so column j's scalar is
 * at [j * ldh].  A column whose flag is 0 is not touched by any step.
 * step_xr: alpha_j = delta1_j / dq_j, X_j += alpha_j D_j, R_j -= alpha_j Q_j (Q == NULL leaves R alone).  Codes: -1 ctx, -2 n < 0, -3 s < 0
 *   or > 65535, -4 D, -5 ldd, -7 ldq (Q given), -8 dq_dev, -9 delta1_dev, -10 ldh < 1, -11 X, -12 ldx, -13 R NULL with Q given, -14 ldr
 *   (Q given), -15 active_dev.
 * step_refresh: R_j = (B1_j - QX_j) - delta X_j, the last term only when delta > 0.  Codes: -1 ctx, -2 n, -3 s, -4 B1, -5 ldb1, -6 QX,
 *   -7 ldqx, -9 X, -10 ldx, -11 R, -12 ldr, -13 active_dev.
 * step_d: one workgroup per column: delta1_new_j = R_j^T S_j (fixed order), written to the column's history; beta_j = that / delta1_old_j,
 *   D_j = beta_j D_j + S_j; active_j is cleared when delta1_new_j > rel_sq_tol_j is false (so a NaN clears it).  delta1_old_dev == NULL is
 *   the first call: the dot alone for EVERY column, rel_sq_tol_j = (delta1_j tol) tol is formed and active_j set from the same test whatever
 *   it held.  Codes: -1 ctx, -2 n, -3 s, -4 R, -5 ldr, -6 S, -7 lds, -9 delta1_new_dev, -10 ldh < 1, -11 D NULL, -12 ldd (both with
 *   delta1_old_dev given), -14 rel_sq_tol_dev, -15 active_dev.
 * The pointer codes only when n > 0 and s > 0; n == 0 or s == 0: each returns 0 and enqueues nothing. */
int rlhip_pcg_saddle_block_step_xr_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* D, int64_t ldd, const double* Q, int64_t ldq,
                                       const double* dq_dev, const double* delta1_dev, int64_t ldh, double* X, int64_t ldx, double* R, int64_t ldr,
                                       const int* active_dev);
int rlhip_pcg_saddle_block_step_xr_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* D, int64_t ldd, const float* Q, int64_t ldq,
                                       const float* dq_dev, const float* delta1_dev, int64_t ldh, float* X, int64_t ldx, float* R, int64_t ldr,
                                       const int* active_dev);
int rlhip_pcg_saddle_block_step_refresh_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* B1, int64_t ldb1, const double* QX, int64_t ldqx,
                                            double delta, const double* X, int64_t ldx, double* R, int64_t ldr, const int* active_dev);
int rlhip_pcg_saddle_block_step_refresh_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* B1, int64_t ldb1, const float* QX, int64_t ldqx,
                                            float delta, const float* X, int64_t ldx, float* R, int64_t ldr, const int* active_dev);
int rlhip_pcg_saddle_block_step_d_f64(rlhip_ctx* ctx, int64_t n, int64_t s, const double* R, int64_t ldr, const double* S, int64_t lds,
                                      const double* delta1_old_dev, double* delta1_new_dev, int64_t ldh, double* D, int64_t ldd, double tol,
                                      double* rel_sq_tol_dev, int* active_dev);
int rlhip_pcg_saddle_block_step_d_f32(rlhip_ctx* ctx, int64_t n, int64_t s, const float* R, int64_t ldr, const float* S, int64_t lds,
                                      const float* delta1_old_dev, float* delta1_new_dev, int64_t ldh, float* D, int64_t ldd, float tol,
                                      float* rel_sq_tol_dev, int* active_dev);
/* The routes of this layer: 76 rlhip_normal_matmat calls on the one-pass route, 77 on the composed route (calls that reach neither are not
 * counted), 78 iterations of the block solver (step_d calls with delta1_old_dev given).  -1 for any other index and for a NULL context. */
int64_t rlhip_lsq_block_path_count(rlhip_ctx* ctx, int which);

/* ---- sparse matrix-vector layer (spmv.hip): the hot path of pcg_saddle on a linops::SparseLinOp.  CSR with int64 indices,
 *      all arrays DEVICE, everything asynchronous, no host read: nnz (= rowptr[nrows]) is an ARGUMENT.  The rules are those of the dense
 *      layer above: no workgroup waits for another, no floating-point atomic, results bitwise reproducible and independent of the grid and
 *      of the device, sums in the precision of the data, nothing written beyond an output's length.  Row pointers are clamped to
 *      [0, nnz]; column indices are trusted. ---- */
/* rlhip_csr_spmv_*: y = alpha A x + beta y for the nrows x ncols CSR A; the transposed product is the same call on the transpose's CSR
 * (rlhip_csr_transpose_*).  beta == 0 does not read y.  nrows == 0 returns 0; nnz == 0 scales y.
 * Rows route: W = 4, 16 or 64 lanes own a row and walk its entries p, p + W, ... in storage order, the W sums added in a fixed tree; x is
 * staged in LDS once per workgroup when ncols * sizeof(T) <= RLHIP_SPMV_X_LDS_BYTES.  Split route: rows cut into chunks of RLHIP_SPMV_CHUNK
 * entries, one wave per chunk, chunk sums in the scratch arena (at most nnz / RLHIP_SPMV_CHUNK + nrows values), a final pass per row.
 * The route: unasked, the split route for at most 512 rows of mean length nnz / nrows >= 2 RLHIP_SPMV_CHUNK, else W = 4 up to a mean row
 * length of 64, W = 16 up to 1023, W = 64 beyond (what was measured, what was not); RLHIP_OPT_SPMV_LANES = 4, 16, 64 or 0
 * (split) forces one.
 * Argument code: -2 for a NULL context, a negative size, or a NULL array that the sizes say is read or written. */
#define RLHIP_SPMV_X_LDS_BYTES 32768
#define RLHIP_SPMV_CHUNK 512
int rlhip_csr_spmv_f64(rlhip_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const double* vals,
                       double alpha, const double* x, double beta, double* y);
int rlhip_csr_spmv_f32(rlhip_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const float* vals,
                       float alpha, const float* x, float beta, float* y);
/* rlhip_csr_normal_matvec_*: q = A^T (A d) + delta d for the m x n CSR A (rowptr, colidx, vals) and the CSR of its transpose (rowptrT,
 * colidxT, valsT): two products as above, + delta d in the pass that writes q.  Optional outputs as in rlhip_normal_matvec_*: t = A d
 * (m values) and *dq_dev = d^T q (the same fixed-order dot).  max_wg > 0 caps the grids; the results do not depend on it.
 * m == 0: q = delta d.  n == 0: returns 0 and writes nothing.  Argument code: -2 as above. */
int rlhip_csr_normal_matvec_f64(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const double* vals,
                                const int64_t* rowptrT, const int64_t* colidxT, const double* valsT, const double* d, double delta, double* q,
                                double* t, double* dq_dev, int64_t max_wg);
int rlhip_csr_normal_matvec_f32(rlhip_ctx* ctx, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr, const int64_t* colidx, const float* vals,
                                const int64_t* rowptrT, const int64_t* colidxT, const float* valsT, const float* d, float delta, float* q, float* t,
                                float* dq_dev, int64_t max_wg);
/* The routes of this layer, one count per product: 50 four lanes per row, 51 sixteen, 52 sixty-four, 53 the split route; 54 counts
 * rlhip_csr_normal_matvec calls (whose two products count as well).  -1 for any other index. */
int64_t rlhip_spmv_path_count(rlhip_ctx* ctx, int which);

/* ---- the squared-exponential kernel between TWO point sets, and kernel ridge regression prediction (rbf.hip; a designed extension, the
 *      reference's squared_exp_kernel_submatrix addresses one point set by offsets).  Z is rows_x x mz (ldz), X is rows_x x nx (ldx), one
 *      column per point, both on the device; Z == X is allowed.  K(Z, X)(i, j) = exp(-|Z(:, i) - X(:, j)|^2 / (2 h^2)), h = bandwidth > 0,
 *      evaluated as exp(scale * ((|z_i|^2 + |x_j|^2) - 2 z_i^T x_j)) with scale = -1 / (2 h^2) rounded from double: rlhip_sqexp_submatrix_*'s
 *      formula, so K(X, X) blocks agree with it to rounding.
 *
 * rlhip_sqexp_cross_submatrix_*: Ksub (rows_ksub x cols_ksub, ldk) = K(Z(:, ro_ksub : ro_ksub + rows_ksub), X(:, co_ksub : co_ksub + cols_ksub)).
 *   sq_colnorms_z (mz values) / sq_colnorms_x (nx values): device squared norms of ALL points of the set, or NULL (those of the block are
 *   computed into scratch).  Argument codes: -2 rows_x < 1, -3 mz < 0, -4 / -8 / -13 a NULL array that would be read or written, -5 / -9
 *   ld < rows_x, -7 nx < 0, -11 / -12 a block outside the point set, -14 ldk, -17 bandwidth not > 0.
 * rlhip_rbf_cross_apply_*: C (mz x n, ldc) = alpha * K(Z, X) * B (nx x n, ldb) + beta * C.  beta == 0: C is not read.  alpha == 0 or
 *   nx == 0: C = beta * C.  mz == 0 or n == 0: returns 0 and touches nothing.
 *   Fused route (n <= RLHIP_RBF_FUSED_MAX_N and rows_x <= RLHIP_RBF_FUSED_MAX_ROWS_X): ONE launch, K is never in memory, scratch = the
 *   mz + nx squared norms.  The sums over the points of X run in the order of X, sixteen points at a time, whatever mz, the grid and the
 *   device are, and there are no atomics: row i of the result is a function of Z(:, i), X, B, alpha, beta and C(i, :) alone, bit for bit --
 *   not of mz, of the row's place in Z, of the CU count or of earlier calls.
 *   Fused and split over X (RLHIP_OPT_RBF_FUSED = 2, the same limits): the one-launch grid is ceil(mz / 64) workgroups that
 *   each walk all of X, a small part of the device when mz is small.  With g = rlhip_rbf_split_chunks(mz, nx) > 1 the kernel runs on a
 *   grid of ceil(mz / 64) x g, chunk b of X = the points [b CH, min(nx, (b + 1) CH)), CH = 64 ceil(nx / (64 g)); the g partial results go
 *   to scratch (g * 64 ceil(mz / 64) * n values beside the norms) and a second launch adds them in the order of b and applies alpha and
 *   beta.  No atomics.  Bit contract of value 2: row i of the result is a function of Z(:, i), X, B, alpha, beta, C(i, :) and g, and g is
 *   a function of (mz, nx) alone -- not of the row's place in Z, of the device or its CU count, of earlier calls or of the grid's
 *   scheduling.  With g == 1 the call runs the one-launch kernel and gives the bits of value 1.  A split apply counts as a fused apply
 *   (55) and in rlhip_rbf_split_count.
 *   Composed route (every other shape; RLHIP_OPT_RBF_FUSED = 0 always): row blocks of K of at most max(2^26, nx) entries in the scratch
 *   arena by rlhip_sqexp_cross_submatrix's kernels, one GEMM with B per block -- what rlhip_rbf_apply_* does, for two point sets.
 *   Returns 0, or -(position of the first bad argument): -2 rows_x < 1, -3 mz < 0, -4 Z NULL, -5 ldz < rows_x, -6 nx < 0, -7 X NULL,
 *   -8 ldx < rows_x, -9 bandwidth not > 0, -10 n < 0, -12 B NULL, -13 ldb < max(nx, 1), -15 C NULL, -16 ldc < max(mz, 1); a NULL array
 *   is an error only where the call would read (or write) it.  Nothing is launched on an argument error. */
#define RLHIP_RBF_FUSED_MAX_N 64
#define RLHIP_RBF_FUSED_MAX_ROWS_X 128
/* The split rule's constants: RLHIP_RBF_SPLIT_W work items (Z tile x chunk) are aimed at, four per CU of a 256-CU part; a chunk is never
 * shorter than RLHIP_RBF_SPLIT_CH_MIN points of X, so nx < 2 * RLHIP_RBF_SPLIT_CH_MIN is never split. */
#define RLHIP_RBF_SPLIT_W 1024
#define RLHIP_RBF_SPLIT_CH_MIN 512
int rlhip_sqexp_cross_submatrix_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, const double* sq_colnorms_z, int64_t nx,
                                    const double* X, int64_t ldx, const double* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, double* Ksub,
                                    int64_t ldk, int64_t ro_ksub, int64_t co_ksub, double bandwidth);
int rlhip_sqexp_cross_submatrix_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, const float* sq_colnorms_z, int64_t nx,
                                    const float* X, int64_t ldx, const float* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, float* Ksub,
                                    int64_t ldk, int64_t ro_ksub, int64_t co_ksub, float bandwidth);
int rlhip_rbf_cross_apply_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx,
                              double bandwidth, int64_t n, double alpha, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
int rlhip_rbf_cross_apply_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx,
                              float bandwidth, int64_t n, float alpha, const float* B, int64_t ldb, float beta, float* C, int64_t ldc);
/* The routes of this layer, one count per call that reached a route: 55 a fused cross apply, 56 a composed one, 57 rlhip_sqexp_cross_submatrix
 * calls.  -1 for any other index or a NULL context. */
int64_t rlhip_rbf_path_count(rlhip_ctx* ctx, int which);
/* The number g >= 1 of chunks that RLHIP_OPT_RBF_FUSED = 2 cuts X into for mz points of Z and nx points of X; no context: g depends on
 * nothing else.  ztiles = ceil(mz / 64); g = min(ceil(RLHIP_RBF_SPLIT_W / ztiles), floor(nx / RLHIP_RBF_SPLIT_CH_MIN)), 1 if that is < 2;
 * else CH = 64 ceil(nx / (64 g)) and g = ceil(nx / CH), so no chunk is empty.  1 for mz == 0 or nx == 0, -1 for a negative argument. */
int64_t rlhip_rbf_split_chunks(int64_t mz, int64_t nx);
/* Fused cross applies of this context that ran split over X (each counted under 55 as well); -1 for a NULL context. */
int64_t rlhip_rbf_split_count(rlhip_ctx* ctx);

/* rlhip_pdk_cross_var_*: the predictive variance of restricted kernel ridge regression as a row-wise weighted quadratic form of the cross
 * kernel (rbf_var.hip; RandLAPACK::krr_predict_restricted_var, rl_krill.hh).  Z rows_x x mz (ldz) evaluation points, Xs
 * rows_x x k (ldx) the centres, G k x k (ldg) and sigma_dev (k, decreasing) the basis of a restricted fit (KrillRestrictedBasis), mus_dev
 * num_mus regularizations >= 0, all DEVICE and of type T; kernel and bandwidth as in rlhip_pdk_cross_apply_*.  With
 *   t_i = K(Z(:, i), Xs) * G (k numbers),   e_jc = mu_c / (sigma_j^2 + mu_c),   mu_c = mus_dev[num_mus == 1 ? 0 : c],
 *   V(i, c) = max(0, 1 - sum_j t_ij^2) + sum_j e_jc t_ij^2            (mz x s, ldv).
 * e is formed in double as mu / fma(sigma, sigma, mu) for both precisions; mu_c == 0 is the pseudo-inverse of rlhip_ridge_filter_*: e = 0
 * where sigma_j > rcond * sigma_0 and 1 where that singular value is cut.  The kernel entries are those of the cross apply (the same
 * constants, the same clamp for the Matern kinds), t is accumulated in T, the squares and both sums are taken in double.  No atomics.
 *   Fused route (opt-in: rlhip_pdk_var_set_fused(ctx, 1), and rlhip_pdk_var_fused(rows_x, k, s) != 0; it keeps no mz x k block in
 *   memory, but measured slower than the composed route's products on the shapes of DESIGN 4.27, so no shape takes it by default): ONE
 *   launch beside the norms and the table of e; neither K nor t reaches memory.  A workgroup owns 64 points of Z and walks the columns of G
 *   in panels of 64, for each panel all k centres; at the end of a panel a lane squares its 16 accumulators and adds them, in the order
 *   of j, to its sums; the four lane groups of a point are added in the order 0, 1, 2, 3.  Scratch: mz + k norms and 64 ceil(k / 64) s
 *   doubles.  Bit contract: row i of V is a function of Z(:, i), Xs, G, sigma, mus and rcond alone -- not of mz, of the row's place in Z,
 *   of the grid or of the device.
 *   Composed route (the default, and every other shape): row blocks of Z sized as rlhip_pdk_cross_apply_* sizes its own (at most
 *   max(2^26 / k, 1) points, a multiple of 256 when there are several, never more than mz); per block t (rows x k) in the scratch arena
 *   by rlhip_pdk_cross_apply_*, then one thread per row adds the squares with j ascending.  This route has NO per-row bit contract: the
 *   GEMMs behind the cross apply choose their kernel and their split of the contraction by the shape and the CU count, so the bits of a
 *   row may change with mz and the device; two calls with the same arguments on the same device give the same bits.  The two routes
 *   differ in the order of the sums.
 * mz == 0 or s == 0: returns 0 and launches nothing.  k == 0: every entry of V is the prior variance 1.
 * Returns 0, or -(position of the first bad argument): -2 rows_x < 1, -3 mz < 0, -5 ldz < rows_x, -6 k < 0, -8 ldx < rows_x, -9 kernel,
 * -10 bandwidth not > 0, -12 ldg < max(k, 1), -14 s < 0, -19 ldv < max(mz, 1); then, when mz > 0 and s > 0: -100 num_mus neither 1 nor s,
 * -17 rcond < 0 or NaN, -18 V NULL, and with k > 0: -4 Z, -7 Xs, -11 G, -13 sigma_dev, -15 mus_dev NULL.  Nothing is launched on an
 * argument error. */
#define RLHIP_PDK_VAR_FUSED_MAX_S 8      /* regularizations whose sums the fused kernel carries in registers */
int rlhip_pdk_cross_var_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t k, const double* Xs, int64_t ldx,
                            int kernel, double bandwidth, const double* G, int64_t ldg, const double* sigma_dev, int64_t s, const double* mus_dev,
                            int64_t num_mus, double rcond, double* V, int64_t ldv);
int rlhip_pdk_cross_var_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t k, const float* Xs, int64_t ldx,
                            int kernel, float bandwidth, const float* G, int64_t ldg, const float* sigma_dev, int64_t s, const float* mus_dev,
                            int64_t num_mus, float rcond, float* V, int64_t ldv);
/* The shapes the fused kernel serves when it is asked for, a function of the shape alone: 1 where rows_x <=
 * RLHIP_RBF_FUSED_MAX_ROWS_X, 1 <= s <= RLHIP_PDK_VAR_FUSED_MAX_S and k >= 1, else 0. */
int rlhip_pdk_var_fused(int64_t rows_x, int64_t k, int64_t s);
/* on != 0: rlhip_pdk_cross_var_* on this context takes its fused kernel wherever rlhip_pdk_var_fused says so; 0 (the default): always the
 * composed route.  A switch of its own: RLHIP_OPT_RBF_FUSED steers the cross apply alone.  Returns the value found, -1 for a NULL context. */
int rlhip_pdk_var_set_fused(rlhip_ctx* ctx, int on);
/* The routes of rlhip_pdk_cross_var_*, one count per call that reached a route: 58 fused, 59 composed.  -1 for any other index. */
int64_t rlhip_pdk_var_path_count(rlhip_ctx* ctx, int which);

/* rlhip_pdk_cross_grad_*: the gradient of a kernel expansion with respect to the evaluation point (rbf_grad.hip;
 * RandLAPACK::krr_predict_grad, rl_krill.hh).  Z rows_x x mz (ldz) evaluation points, X rows_x x nx (ldx), B nx x n (ldb), all
 * DEVICE; kernel and bandwidth as in rlhip_pdk_cross_apply_*.  G is rows_x x (mz n) (ldg >= rows_x); its column r mz + i holds
 *   alpha * sum_j w(s_ij) (Z(:, i) - X(:, j)) B(j, r),   s_ij = |Z(:, i) - X(:, j)|^2,   w(s) = 2 dk/ds,
 * the gradient at point i of right-hand side r, laid out like Z.  w(s) = w(0) u(s):
 *        RLHIP_PDK_SQEXP     w(0) = -1 / l^2        u = exp(-s / (2 l^2))
 *        RLHIP_PDK_MATERN32  w(0) = -3 / l^2        u = exp(-a)
 *        RLHIP_PDK_MATERN52  w(0) = -5 / (3 l^2)    u = (1 + a) exp(-a)          a as for the kernel itself
 * with the kernels' constants, the cross apply's s = (|z|^2 + |x|^2) - 2 z.x and, for the Matern kinds, its clamp of s at 0, so the
 * gradient is finite and smooth at coincident points.  Coordinate c is evaluated as alpha * (w(0) * fma(z_c, T_0, -T_c)) with
 * T_0 = sum_j u_ij B(j, r) and T_c = sum_j u_ij (X(c, j) B(j, r)): a cross apply with rows_x + 1 times as many columns.  Its error is of
 * the order eps (|z_c| + |x_c|) sum_j |w_ij| |B(j, r)|, the class of the norm expansion's own.
 * G is written, never read.  alpha == 0, nx == 0: exact zeros, X and B are not read.  mz == 0 or n == 0: returns 0 and touches nothing.
 * Rows of G past rows_x and columns past mz n are not touched.
 *   Composed route (the default): B' = [B, x_1 o B, ..., x_d o B] per right-hand side (nx x n (rows_x + 1)) in the scratch arena, the
 *   cross apply's own machinery on it with u in place of the kernel function -- its fused kernel for n (rows_x + 1) <=
 *   RLHIP_RBF_FUSED_MAX_N and RLHIP_OPT_RBF_FUSED != 0, row blocks of the weight matrix otherwise, never split over X -- into an
 *   mz x n (rows_x + 1) block of scratch, and one thread per entry of G.  Z is cut into blocks of at most max(2^26 / (n (rows_x + 1)), 1)
 *   points, a multiple of 256 when there are several.
 *   Fused route (opt-in: rlhip_pdk_grad_set_fused(ctx, 1), and rlhip_pdk_grad_fused(rows_x, n) != 0): ONE launch beside the norms; B'
 *   is formed in LDS from the staged tiles of X and B, T in the accumulators of the cross apply's tile walk, and the combination is
 *   the kernel's epilogue.  The sums over j run in the order of j, sixteen at a time; no atomics.  Bit contract: column r mz + i of G is
 *   a function of Z(:, i), X, B and alpha alone -- not of mz, of the point's place in Z, of the grid or of the device.
 * Returns 0, or -(position of the first bad argument): -2 rows_x < 1, -3 mz < 0, -4 Z NULL, -5 ldz < rows_x, -6 nx < 0, -7 X NULL,
 * -8 ldx < rows_x, -9 kernel, -10 bandwidth not > 0, -11 n < 0, -13 B NULL, -14 ldb < max(nx, 1), -15 G NULL, -16 ldg < rows_x; a NULL
 * array is an error only where the call would read (or write) it.  Nothing is launched on an argument error. */
#define RLHIP_PDK_GRAD_FUSED_MAX_COLS 64      /* n (rows_x + 1) the fused kernel carries: four 16-column accumulator tiles, the cross apply's width */
int rlhip_pdk_cross_grad_f64(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx,
                             int kernel, double bandwidth, int64_t n, double alpha, const double* B, int64_t ldb, double* G, int64_t ldg);
int rlhip_pdk_cross_grad_f32(rlhip_ctx* ctx, int64_t rows_x, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx,
                             int kernel, float bandwidth, int64_t n, float alpha, const float* B, int64_t ldb, float* G, int64_t ldg);
/* The shapes the fused kernel serves when it is asked for, a function of the shape alone: 1 where 1 <= rows_x <=
 * RLHIP_RBF_FUSED_MAX_ROWS_X and 1 <= n (rows_x + 1) <= RLHIP_PDK_GRAD_FUSED_MAX_COLS, else 0. */
int rlhip_pdk_grad_fused(int64_t rows_x, int64_t n);
/* on != 0: rlhip_pdk_cross_grad_* on this context takes its fused kernel wherever rlhip_pdk_grad_fused says so; 0 (the default): always
 * the composed route.  Returns the value found, -1 for a NULL context. */
int rlhip_pdk_grad_set_fused(rlhip_ctx* ctx, int on);
/* The routes of rlhip_pdk_cross_grad_*, one count per call that reached a route: 74 fused, 75 composed.  -1 for any other index. */
int64_t rlhip_pdk_grad_path_count(rlhip_ctx* ctx, int which);

/* ---- row-block sharding across the GPUs of a node (new design; the reference has no
 *      distributed code).  One process per GPU.  Sum all-reduces run on the context's stream through RCCL
 *      (bound at run time), or through a host-installed hook.  With no communicator every call is a no-op,
 *      so single-GPU callers never notice. ---- */
typedef int (*rlhip_allreduce_hook)(void* user, void* dev_buf, int64_t count, int is_f64);
/* 1 when RCCL can be bound in this process, 0 otherwise.  ncclCommInitRank is collective, so ranks agree on this (MIN over the
 * ranks) BEFORE any of them calls rlhip_comm_init; a process that already maps an RCCL (PyTorch's) gets that copy, never a second one. */
int rlhip_comm_can_load(void);
const char* rlhip_comm_rccl_origin(void);   /* where the bound RCCL came from (diagnostics) */
/* ncclGetVersion of the bound RCCL (e.g. 22203; 0: not bound); how this context's collectives travel: 1 its own RCCL communicator, 2 the
 * caller's hook, 0 none (one rank) -- bench.py prints both next to rlhip_comm_size so that a scaling line proves what it ran on */
int rlhip_comm_rccl_version(void);
int rlhip_comm_kind(rlhip_ctx* ctx);
int rlhip_comm_unique_id(unsigned char id_out[128]);                 /* rank 0: ncclGetUniqueId */
int rlhip_comm_init(rlhip_ctx* ctx, int nranks, int rank, const unsigned char id[128]);
int rlhip_comm_set_hook(rlhip_ctx* ctx, rlhip_allreduce_hook hook, void* user, int nranks, int rank);
int rlhip_comm_destroy(rlhip_ctx* ctx);
int rlhip_comm_size(rlhip_ctx* ctx);
int rlhip_comm_rank(rlhip_ctx* ctx);
int rlhip_allreduce_sum_f64(rlhip_ctx* ctx, double* buf, int64_t count);
int rlhip_allreduce_sum_f32(rlhip_ctx* ctx, float* buf, int64_t count);
int rlhip_allreduce_sum_host_f64(rlhip_ctx* ctx, double* x_host, int64_t n);   /* n <= 16 scalars */

/* ---- diagnostics ---- */
/* number of times this context took a specialised kernel path: 0 persistent stream-K fp64 GEMM (gemm_sk.hip), 1 its fp32 twin,
 * 2 fused MFMA trsm block kernel (tri.hip), 3 row-per-lane substitution trsm sub-block, 4 fused out-of-place trsm (rlhip_trsm_gather),
 * 5 sketch-preconditioned Cholesky-QR panel inside geqrf (house.hip), 6 persistent one-launch Jacobi sweeps (jacobi.hip),
 * 7 column-at-a-time LU panel of a matrix taller than the resident register kernels hold (lu.hip), 8 register-resident block-pipelined
 * Householder QR of a sketch-sized matrix (qr_blk.hip), 9 its sign-modified LU twin inside orhr_col, 10 the Gram route of the device SVD
 * (svd.hip::gesdd_tall_gram: Jacobi on A^T A, one host read), 11 the one-stream Cholesky-QR (rlhip_cholqrq),
 * 12 block iterations of BQRRP whose sketch down-date and next QRCP ran on the side queue (the look-ahead of rl_bqrrp.hh; noted by the C++
 * layer through rlhip_path_note), 13 CQRRPT calls that took the split order (rl_cqrrpt.hh), 14 sparse-sign sketches applied by the LDS-DMA kernel
 * (sketch.hip::saso_apply_dma_kernel), 15 persistent Jacobi launches whose workers sat on one XCD and handed their blocks over through its L2
 * (jacobi.hip; the other launches use the uncached hand-over: same bits, slower).
 * The route a device SVD took (svd.hip::gesdd_tall, one count per call on the branch taken; 10 is its Gram route): 16 Cholesky-QR twice,
 * 17 one pass (the second factorization skipped), 18 V recovered from R Ux instead of accumulated (beside 16 or 17), 19 Jacobi on A after
 * the first factorization failed or its diagonal ratio reached the limit, 20 Jacobi on A after the second factorization failed and the
 * first pass was undone.  The sweep driver of a one-sided Jacobi (jacobi.hip::gesvdj, beside 6): 21 LDS-resident blocks of 16 columns x 256
 * rows, 22 of 16 x 512 rows, 23 of 32 columns x 256 rows, 24 one launch per round (more than 512 rows), 25 an fp32 problem run in fp64
 * (counted beside the driver it then takes).  The routes of a product that is not the persistent kernel's (gemm.hip::gemm_impl, counted on
 * the host where the launch is enqueued; 0 and 1 are the persistent ones): 26 a launch of the tiled kernel (gemm_kernel), 27 a tiled launch
 * that went split-K (slabs + splitk_reduce_kernel; counted beside 26), 28 the small-product kernel (gemm_small_kernel), 29 the narrow-panel
 * kernel (gemm_tn_skinny_kernel), 30 scale-only calls (k == 0 or alpha == 0: C = beta C, also counted for beta == 1, which launches nothing),
 * 31 a contraction cut in two or more calls by gemm_impl itself (the k-remainder peel, the fp32 chunks of 16384 and their Gram twin; the
 * pieces count their own routes), 32 a product whose last m % 128 rows were peeled off a persistent launch and given to another route.
 * The sketching operator (sketch.hip, one count per call): 33 a sketch application that launched the register-staged kernel
 * (saso_apply_kernel; beside 14 when a ragged first or last row block went to it), 34 that call used 2-column slabs, 35 a 1-column slab
 * (both beside 33; neither: 4 columns); an independent-column operator built 36 by the one-workgroup-per-block LDS kernel
 * (saso_ind_block_kernel) or 37 by the generate / scan / scatter / sort chain.  The CSR kernels (sparse.hip): a product served by 38 the
 * wavefront-per-row kernel (csr_spmm_rm_kernel), 39 the narrow row-major kernel (csr_spmm_rm_narrow_kernel), 40 the narrow kernel with a
 * column-major result (csr_spmm_cmout_narrow_kernel); a transpose scattered 41 by entry number and sorted row by row, 42 by the stable
 * counting sort over chunks.
 * -1 for an unknown index.  Tests use it to assert that the kernel / route under test is the one that ran. */
int64_t rlhip_path_count(rlhip_ctx* ctx, int which);
/* The routes of the LU layer (lu.hip), counted on the host where the launch is enqueued; they continue the numbering above but are read
 * here (7, the column-at-a-time panel, stays with rlhip_path_count).  A panel of rlhip_getrf_* / rlhip_getrf_piv_* factored by 60 the LDS
 * kernel (getrf_panel_kernel, fewer than 1024 rows on and below the diagonal), 61 the fast step of the type (at most 64 workgroups),
 * 62 the general register kernel (getrf_panel_reg_kernel); 63 a getrf call that ran with an outer block wider than a panel (two-level
 * blocking, m >= 49152 and n >= 256); 64 a launch of unit_lower_solve_kernel (the forward substitution right of such an outer block);
 * rlhip_luqrcp_piv served by 65 the LDS walk (min(sd, cols) <= 2048) or 66 the serial kernel.  -1 for any other index. */
int64_t rlhip_lu_path_count(rlhip_ctx* ctx, int which);
/* The routes of the triangular layer (tri.hip) that 2, 3, 4 and 11 above do not tell apart, counted on the host where the launch is enqueued,
 * one per launch: a 256-column block of rlhip_trsm_* solved by 67 the per-block MFMA kernel with one row tile per wavefront
 * (trsm_blk_kernel<T, 1>) or 68 with two (m >= 65536); 69 a fused launch that took the twelve-wavefront instantiation (fp32 in place, beside 2);
 * 70 a fused out-of-place solve that ran on the identity-column twin (no pivot vector; beside 4, only when the solve succeeded); 71 a
 * rlhip_trsm_gather_* call served by the column gather + the in-place solver; 72 a rlhip_trmm_* call with side Right, 73 with side Left.
 * -1 for any other index. */
int64_t rlhip_tri_path_count(rlhip_ctx* ctx, int which);
/* the host layers above this ABI (include/RandLAPACK_amd/) report their own route decisions into the same counters */
int rlhip_path_note(rlhip_ctx* ctx, int which, int64_t delta);
/* Profiler phase markers (the reference brackets every phase of BQRRP_GPU with NVTX ranges, drivers/rl_bqrrp_gpu.hh:11,335-403; these are the
 * ROCm equivalent, roctxRangePushA / roctxRangePop of librocprofiler-sdk-roctx, bound at run time).  Active when the roctx library is already
 * in the process (rocprofv3 --marker-trace) or RLHIP_ROCTX=1; otherwise both calls return 0 and do nothing.  Host-side ranges: they bracket
 * the ENQUEUE of a phase; with the drivers' timing switch on (every lap drains the stream) they bracket its execution too. */
int rlhip_range_push(const char* name);
int rlhip_range_pop(void);
/* Scope switch for the products this context launches: on != 0 -> no kernel of this context may hold every CU until it is done (the
 * persistent stream-K GEMMs give way to the tiled ones, whose workgroups retire continuously), so that work enqueued on a side queue
 * (rlhip_side_of) finds CUs beside it.  Returns the previous setting (0 / 1), -1 on a bad context. */
int rlhip_avoid_persistent(rlhip_ctx* ctx, int on);
/* pure-MFMA issue-rate microbenchmark; returns achieved TFLOP/s of v_mfma_{f64,f32}_16x16x4 in *tflops_host */
int rlhip_mfma_peak(rlhip_ctx* ctx, int is_f64, int iters, double* tflops_host);
/* diagnostic: keep `blocks` workgroups busy for `usec` microseconds (mode 0 sleeping, 1 fp64 FMA chain, 2 fp64 MFMA stream), on the context's
 * stream (side = 0) or on a second stream beside it (side = 1); scripts/dvfs_probe.py maps the part's clock response to load with it */
int rlhip_dvfs_burn(rlhip_ctx* ctx, int blocks, int mode, int usec, int side);
/* streaming-read bandwidth microbenchmark over `bytes` of device memory (GB/s) */
int rlhip_hbm_read_peak(rlhip_ctx* ctx, const void* buf, size_t bytes, double* gbps_host);

#ifdef __cplusplus
}
#endif
#endif /* RLHIP_H */
