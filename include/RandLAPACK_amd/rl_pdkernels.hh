// Squared-exponential (RBF) kernel matrices, device flavour (RandLAPACK/misc/rl_pdkernels.hh):
//   squared_exp_kernel_submatrix   rl_pdkernels.hh:133-148   MFMA GEMM for -2 X^T X + one epilogue kernel (rlhip_sqexp_submatrix_*)
//   linops::RBFKernelMatrix        rl_pdkernels.hh:205-294   over a DEVICE X (rows_x x dim, one column per point)
//
// Deviations:
//   - the kernel is exp(-|x_i - x_j|^2 / (2 h^2)), which is what the reference's code computes (its doc comment at :217 says / h);
//   - operator() forms K in full row blocks (rlhip_rbf_apply_*) instead of the reference's symmetric arrowhead (block_arrowhead_multiply):
//     twice the exp evaluations, one plain MFMA GEMM per block;
//   - the host functor operator()(i, j) cannot run on the device: rp_cholesky reads the operator through diag() and columns() instead,
//     which evaluate the same entries by differences (rlhip_sqexp_columns_*), so the diagonal is exactly 1 (+ reg).
// Extensions (the reference has neither):
//   linops::RBFCrossKernel         the rectangular kernel K(Z, X) between two DEVICE point sets: operator(), matvec, submatrix, grad
//                                  (rlhip_rbf_cross_apply_*, rlhip_sqexp_cross_submatrix_*) -- what KRR prediction multiplies by;
//   RBFKernelMatrix::set_matrix_free(true): operator() through the same kernels with Z = X (K never in memory); off by default.
// Extension: set_split_x(true) on either operator runs its cross apply with the fused kernel split over X; off by default.
// Extension: the kernel function is a member of both operators, PDKernel::SquaredExp by default; set_kernel selects Matern 3/2
// or 5/2 (rlhip_pdk_*).  rp_cholesky, rpchol_pc_data, krill_full_rpchol and krr_predict reach the kernel through these objects only.
#pragma once
#include <cstdint>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_lapackpp.hh"

namespace RandLAPACK {

/// the kernel functions of the device library, as a function of s = |z - x|^2 and the bandwidth l (include/rlhip.h, RLHIP_PDK_*):
/// exp(-s / (2 l^2)); (1 + a) exp(-a), a = sqrt(3 s) / l; (1 + a + a^2 / 3) exp(-a), a = sqrt(5 s) / l
enum class PDKernel : int { SquaredExp = RLHIP_PDK_SQEXP, Matern32 = RLHIP_PDK_MATERN32, Matern52 = RLHIP_PDK_MATERN52 };

// the squared exponential goes through the entries it always went through, the other kinds through their generalisations (the same code)
namespace _pdk_impl {
inline int sqexp_submatrix(blas::Queue& q, int64_t rx, int64_t cx, const double* X, int64_t ldx, const double* nr, int64_t r, int64_t c,
                           double* K, int64_t ldk, int64_t ro, int64_t co, PDKernel kf, double h) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_submatrix_f64(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, h)
                                      : rlhip_pdk_submatrix_f64(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, (int)kf, h);
}
inline int sqexp_submatrix(blas::Queue& q, int64_t rx, int64_t cx, const float* X, int64_t ldx, const float* nr, int64_t r, int64_t c,
                           float* K, int64_t ldk, int64_t ro, int64_t co, PDKernel kf, float h) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_submatrix_f32(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, h)
                                      : rlhip_pdk_submatrix_f32(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, (int)kf, h);
}
inline int sq_colnorms(blas::Queue& q, int64_t rx, int64_t cx, const double* X, int64_t ldx, double* nr) { return rlhip_sq_colnorms_f64(q.ctx(), rx, cx, X, ldx, nr); }
inline int sq_colnorms(blas::Queue& q, int64_t rx, int64_t cx, const float* X, int64_t ldx, float* nr) { return rlhip_sq_colnorms_f32(q.ctx(), rx, cx, X, ldx, nr); }
inline int columns(blas::Queue& q, int64_t rx, int64_t n, const double* X, int64_t ldx, int64_t nidx, const int64_t* idx, PDKernel kf, double h,
                   double reg, double* out, int64_t ldo) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_columns_f64(q.ctx(), rx, n, X, ldx, nidx, idx, h, reg, out, ldo)
                                      : rlhip_pdk_columns_f64(q.ctx(), rx, n, X, ldx, nidx, idx, (int)kf, h, reg, out, ldo);
}
inline int columns(blas::Queue& q, int64_t rx, int64_t n, const float* X, int64_t ldx, int64_t nidx, const int64_t* idx, PDKernel kf, float h,
                   float reg, float* out, int64_t ldo) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_columns_f32(q.ctx(), rx, n, X, ldx, nidx, idx, h, reg, out, ldo)
                                      : rlhip_pdk_columns_f32(q.ctx(), rx, n, X, ldx, nidx, idx, (int)kf, h, reg, out, ldo);
}
inline int apply(blas::Queue& q, int64_t rx, int64_t dim, const double* X, int64_t ldx, PDKernel kf, double h, const double* regs, int64_t nops,
                 int eir, int64_t n, double a, const double* B, int64_t ldb, double b, double* C, int64_t ldc) {
    return kf == PDKernel::SquaredExp ? rlhip_rbf_apply_f64(q.ctx(), rx, dim, X, ldx, h, regs, nops, eir, n, a, B, ldb, b, C, ldc)
                                      : rlhip_pdk_apply_f64(q.ctx(), rx, dim, X, ldx, (int)kf, h, regs, nops, eir, n, a, B, ldb, b, C, ldc);
}
inline int apply(blas::Queue& q, int64_t rx, int64_t dim, const float* X, int64_t ldx, PDKernel kf, float h, const float* regs, int64_t nops,
                 int eir, int64_t n, float a, const float* B, int64_t ldb, float b, float* C, int64_t ldc) {
    return kf == PDKernel::SquaredExp ? rlhip_rbf_apply_f32(q.ctx(), rx, dim, X, ldx, h, regs, nops, eir, n, a, B, ldb, b, C, ldc)
                                      : rlhip_pdk_apply_f32(q.ctx(), rx, dim, X, ldx, (int)kf, h, regs, nops, eir, n, a, B, ldb, b, C, ldc);
}
inline int cross_apply(blas::Queue& q, int64_t rx, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx, PDKernel kf,
                       double h, int64_t n, double a, const double* B, int64_t ldb, double b, double* C, int64_t ldc) {
    return kf == PDKernel::SquaredExp ? rlhip_rbf_cross_apply_f64(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, h, n, a, B, ldb, b, C, ldc)
                                      : rlhip_pdk_cross_apply_f64(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, (int)kf, h, n, a, B, ldb, b, C, ldc);
}
inline int cross_apply(blas::Queue& q, int64_t rx, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx, PDKernel kf,
                       float h, int64_t n, float a, const float* B, int64_t ldb, float b, float* C, int64_t ldc) {
    return kf == PDKernel::SquaredExp ? rlhip_rbf_cross_apply_f32(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, h, n, a, B, ldb, b, C, ldc)
                                      : rlhip_pdk_cross_apply_f32(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, (int)kf, h, n, a, B, ldb, b, C, ldc);
}
inline int cross_grad(blas::Queue& q, int64_t rx, int64_t mz, const double* Z, int64_t ldz, int64_t nx, const double* X, int64_t ldx, PDKernel kf,
                      double h, int64_t n, double a, const double* B, int64_t ldb, double* G, int64_t ldg) {
    return rlhip_pdk_cross_grad_f64(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, (int)kf, h, n, a, B, ldb, G, ldg);
}
inline int cross_grad(blas::Queue& q, int64_t rx, int64_t mz, const float* Z, int64_t ldz, int64_t nx, const float* X, int64_t ldx, PDKernel kf,
                      float h, int64_t n, float a, const float* B, int64_t ldb, float* G, int64_t ldg) {
    return rlhip_pdk_cross_grad_f32(q.ctx(), rx, mz, Z, ldz, nx, X, ldx, (int)kf, h, n, a, B, ldb, G, ldg);
}
/// while alive and `on`: RLHIP_OPT_RBF_FUSED = 2 (the fused cross apply split over X) on q's context; the value found is put back
struct split_x_scope {
    rlhip_ctx* ctx;
    int64_t found;
    bool on;
    split_x_scope(blas::Queue& q, bool on) : ctx(q.ctx()), found(-1), on(on) {
        if (!on) return;
        found = rlhip_get_option(ctx, RLHIP_OPT_RBF_FUSED);
        rlhip_set_option(ctx, RLHIP_OPT_RBF_FUSED, 2);
    }
    ~split_x_scope() { if (on) rlhip_set_option(ctx, RLHIP_OPT_RBF_FUSED, found); }
    split_x_scope(const split_x_scope&) = delete;
    split_x_scope& operator=(const split_x_scope&) = delete;
};
inline int cross_submatrix(blas::Queue& q, int64_t rx, int64_t mz, const double* Z, int64_t ldz, const double* nz, int64_t nx, const double* X,
                           int64_t ldx, const double* nxr, int64_t r, int64_t c, double* K, int64_t ldk, int64_t ro, int64_t co, PDKernel kf,
                           double h) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_cross_submatrix_f64(q.ctx(), rx, mz, Z, ldz, nz, nx, X, ldx, nxr, r, c, K, ldk, ro, co, h)
                                      : rlhip_pdk_cross_submatrix_f64(q.ctx(), rx, mz, Z, ldz, nz, nx, X, ldx, nxr, r, c, K, ldk, ro, co, (int)kf, h);
}
inline int cross_submatrix(blas::Queue& q, int64_t rx, int64_t mz, const float* Z, int64_t ldz, const float* nz, int64_t nx, const float* X,
                           int64_t ldx, const float* nxr, int64_t r, int64_t c, float* K, int64_t ldk, int64_t ro, int64_t co, PDKernel kf,
                           float h) {
    return kf == PDKernel::SquaredExp ? rlhip_sqexp_cross_submatrix_f32(q.ctx(), rx, mz, Z, ldz, nz, nx, X, ldx, nxr, r, c, K, ldk, ro, co, h)
                                      : rlhip_pdk_cross_submatrix_f32(q.ctx(), rx, mz, Z, ldz, nz, nx, X, ldx, nxr, r, c, K, ldk, ro, co, (int)kf, h);
}
inline int axpby(blas::Queue& q, int64_t n, double a, const double* x, double b, double* y) { return rlhip_axpby_f64(q.ctx(), n, a, x, b, y); }
inline int axpby(blas::Queue& q, int64_t n, float a, const float* x, float b, float* y) { return rlhip_axpby_f32(q.ctx(), n, a, x, b, y); }
}  // namespace _pdk_impl

/// Ksub (rows_ksub x cols_ksub, ld rows_ksub) = the (ro_ksub, co_ksub)-offset block of K(i, j) = exp(-|X(:,i) - X(:,j)|^2 / (2 h^2)).
/// X (rows_x x cols_x, ld rows_x) and sq_colnorms_x (|X(:,j)|^2, cols_x entries) are DEVICE arrays, as Ksub.            rl_pdkernels.hh:133
template <typename T>
void squared_exp_kernel_submatrix(int64_t rows_x, int64_t cols_x, const T* X, T* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, T* Ksub,
                                  int64_t ro_ksub, int64_t co_ksub, T bandwidth, blas::Queue& q = blas::default_queue()) {
    randlapack_require(bandwidth > 0) << "kernel bandwidth must be > 0; got bandwidth=" << bandwidth;
    blas::check(_pdk_impl::sqexp_submatrix(q, rows_x, cols_x, X, rows_x, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, rows_ksub > 0 ? rows_ksub : 1,
                                           ro_ksub, co_ksub, PDKernel::SquaredExp, bandwidth), "squared_exp_kernel_submatrix");
}

/// the same block for any kernel function of PDKernel (the Matern kinds clamp the expanded squared distance at 0)
template <typename T>
void pd_kernel_submatrix(PDKernel kernel, int64_t rows_x, int64_t cols_x, const T* X, T* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, T* Ksub,
                         int64_t ro_ksub, int64_t co_ksub, T bandwidth, blas::Queue& q = blas::default_queue()) {
    randlapack_require(bandwidth > 0) << "kernel bandwidth must be > 0; got bandwidth=" << bandwidth;
    blas::check(_pdk_impl::sqexp_submatrix(q, rows_x, cols_x, X, rows_x, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, rows_ksub > 0 ? rows_ksub : 1,
                                           ro_ksub, co_ksub, kernel, bandwidth), "pd_kernel_submatrix");
}

namespace linops {

/// num_ops >= 1 regularized RBF kernel matrices that differ only on their diagonals (1 + regs[k]); X is a DEVICE rows_x x dim matrix (ld
/// ldx, default rows_x), regs a HOST array the caller keeps alive, as in the reference (it holds argregs.data()).      rl_pdkernels.hh:205-294
template <typename T>
struct RBFKernelMatrix {
    const int64_t dim;
    const T* X;
    const int64_t rows_x;
    T bandwidth;
    int64_t num_ops;
    T* regs;
    int64_t ldx;
    bool _eval_includes_reg;
    bool _matrix_free = false;
    bool _split_x = false;
    PDKernel kernel = PDKernel::SquaredExp;
    blas::Queue& q;

    using scalar_t = T;

    RBFKernelMatrix(int64_t dim, const T* X, int64_t rows_x, T bandwidth, std::vector<T>& argregs, blas::Queue& queue = blas::default_queue(),
                    int64_t ldx = 0)
        : dim(dim), X(X), rows_x(rows_x), bandwidth(bandwidth), num_ops((int64_t)argregs.size()), regs(argregs.data()),
          ldx(ldx > 0 ? ldx : rows_x), _eval_includes_reg(false), q(queue) {
        randlapack_require(bandwidth > 0) << "kernel bandwidth must be > 0; got bandwidth=" << bandwidth;
        randlapack_require(this->ldx >= rows_x) << "ldx=" << this->ldx << " < rows_x=" << rows_x;
    }

    void set_eval_includes_reg(bool eir) { _eval_includes_reg = eir; }
    /// true: operator() multiplies through rlhip_rbf_cross_apply_* with Z = X (matrix-free inside that routine's fused limits) instead of
    /// rlhip_rbf_apply_*'s row blocks of K in scratch.  Off by default: the default path is the one that was measured.
    void set_matrix_free(bool mf) { _matrix_free = mf; }
    /// true: the matrix-free product runs with RLHIP_OPT_RBF_FUSED = 2, the fused kernel split over X where rlhip_rbf_split_chunks(dim, dim) > 1
    /// (DESIGN 4.25); the option is put back to what it was after the call.  No effect without set_matrix_free(true).  Off by default.
    void set_split_x(bool s) { _split_x = s; }
    /// the kernel function of every entry point of this operator: operator() on both branches, columns(); the diagonal is 1 for each
    void set_kernel(PDKernel k) { kernel = k; }

    /// C (dim x n) = alpha * (K [+ diag(regs)]) * B + beta * C                                                            (:255-283)
    void operator()(blas::Layout layout, int64_t n, T alpha, T* const B, int64_t ldb, T beta, T* C, int64_t ldc) {
        randlapack_require(layout == blas::Layout::ColMajor) << "this kernel matrix only supports ColMajor layout";
        randlapack_require(ldb >= dim) << "ldb=" << ldb << " < dim=" << dim << " (ldb must be >= operator dimension)";
        randlapack_require(ldc >= dim) << "ldc=" << ldc << " < dim=" << dim << " (ldc must be >= operator dimension)";
        if (_eval_includes_reg) {
            randlapack_require(num_ops == 1 || n == num_ops) << "with num_ops>1, n=" << n << " must equal num_ops=" << num_ops
                                                             << " so each column gets its own regularization";
        }
        if (_matrix_free) {
            _pdk_impl::split_x_scope split(q, _split_x);
            blas::check(_pdk_impl::cross_apply(q, rows_x, dim, X, ldx, dim, X, ldx, kernel, bandwidth, n, alpha, B, ldb, beta, C, ldc),
                        "RBFKernelMatrix");
            // the regularization term, exactly as rlhip_rbf_apply_* adds it: column i gets alpha * regs[min(i, num_ops - 1)] * B(:, i)
            for (int64_t i = 0; _eval_includes_reg && dim > 0 && i < n; ++i) {
                const T coeff = alpha * regs[i < num_ops - 1 ? i : num_ops - 1];
                blas::check(_pdk_impl::axpby(q, dim, coeff, B + i * ldb, T(1), C + i * ldc), "RBFKernelMatrix");
            }
            return;
        }
        blas::check(_pdk_impl::apply(q, rows_x, dim, X, ldx, kernel, bandwidth, regs, num_ops, _eval_includes_reg ? 1 : 0, n, alpha, B, ldb, beta, C,
                                     ldc), "RBFKernelMatrix");
    }

    /// the diagonal (DEVICE, dim entries): 1, or 1 + regs[0] when the evaluation includes the regularization (operator()(i, i), :285-292)
    void diag(T* d_dev) {
        const T v = T(1) + diag_reg();
        lapack::laset(MatrixType::General, dim, 1, v, v, d_dev, dim > 0 ? dim : 1, q);
    }
    /// out(:, l) = K(:, idx_dev[l]) (+ regs[0] on the diagonal), DEVICE indices and output (dim x nidx, ldo)
    void columns(int64_t nidx, const int64_t* idx_dev, T* out, int64_t ldo) {
        blas::check(_pdk_impl::columns(q, rows_x, dim, X, ldx, nidx, idx_dev, kernel, bandwidth, diag_reg(), out, ldo), "RBFKernelMatrix::columns");
    }

private:
    T diag_reg() const {
        if (!_eval_includes_reg) return T(0);
        randlapack_require(num_ops == 1) << "this operation requires num_ops=1; got num_ops=" << num_ops;
        return regs[0];
    }
};

/// The rectangular kernel K(Z, X) (mz x nx) between two DEVICE point sets, Z rows_x x mz (ldz, default rows_x) and X rows_x x nx (ldx,
/// default rows_x), one column per point: K(i, j) = exp(-|Z(:,i) - X(:,j)|^2 / (2 h^2)), or the Matern kind chosen by set_kernel.  Z == X is allowed.  ColMajor only.  This is
/// the operator of KRR prediction (krr_predict, rl_krill.hh), not a full LinearOperator: Side, trans_B and the sketch-operator overloads of
/// that concept are not provided.
template <typename T>
struct RBFCrossKernel {
    const int64_t n_rows;      // mz
    const int64_t n_cols;      // nx
    const int64_t rows_x;
    const T* Z;
    const T* X;
    T bandwidth;
    int64_t ldz, ldx;
    PDKernel kernel = PDKernel::SquaredExp;
    bool _split_x = false;
    blas::Queue& q;

    using scalar_t = T;

    void set_kernel(PDKernel k) { kernel = k; }
    /// true: operator() (and matvec) run with RLHIP_OPT_RBF_FUSED = 2, the fused kernel split over X where rlhip_rbf_split_chunks says so
    /// (DESIGN 4.25): for few evaluation points against many training points.  The option is put back after the call.  Off by default.
    void set_split_x(bool s) { _split_x = s; }

    RBFCrossKernel(int64_t rows_x, int64_t mz, const T* Z, int64_t nx, const T* X, T bandwidth, blas::Queue& queue = blas::default_queue(),
                   int64_t ldz = 0, int64_t ldx = 0)
        : n_rows(mz), n_cols(nx), rows_x(rows_x), Z(Z), X(X), bandwidth(bandwidth), ldz(ldz > 0 ? ldz : rows_x), ldx(ldx > 0 ? ldx : rows_x),
          q(queue) {
        randlapack_require(bandwidth > 0) << "kernel bandwidth must be > 0; got bandwidth=" << bandwidth;
        randlapack_require(rows_x >= 1) << "rows_x=" << rows_x << " must be >= 1";
        randlapack_require(mz >= 0 && nx >= 0) << "mz=" << mz << " and nx=" << nx << " must be >= 0";
        randlapack_require(this->ldz >= rows_x) << "ldz=" << this->ldz << " < rows_x=" << rows_x;
        randlapack_require(this->ldx >= rows_x) << "ldx=" << this->ldx << " < rows_x=" << rows_x;
    }

    /// C = alpha * op(K) * B + beta * C.  NoTrans: B nx x n, C mz x n.  Trans: K(Z, X)^T = K(X, Z), the same call with the point sets swapped.
    void operator()(blas::Layout layout, blas::Op trans, int64_t n, T alpha, const T* B, int64_t ldb, T beta, T* C, int64_t ldc) {
        randlapack_require(layout == blas::Layout::ColMajor) << "this kernel operator only supports ColMajor layout";
        const bool tr = trans != blas::Op::NoTrans;
        const int64_t rows = tr ? n_cols : n_rows, cols = tr ? n_rows : n_cols;
        randlapack_require(ldb >= cols) << "ldb=" << ldb << " < " << cols << " (ldb must be >= the columns of op(K))";
        randlapack_require(ldc >= rows) << "ldc=" << ldc << " < " << rows << " (ldc must be >= the rows of op(K))";
        const int64_t ldb1 = ldb > 0 ? ldb : 1, ldc1 = ldc > 0 ? ldc : 1;
        _pdk_impl::split_x_scope split(q, _split_x);
        blas::check(tr ? _pdk_impl::cross_apply(q, rows_x, n_cols, X, ldx, n_rows, Z, ldz, kernel, bandwidth, n, alpha, B, ldb1, beta, C, ldc1)
                       : _pdk_impl::cross_apply(q, rows_x, n_rows, Z, ldz, n_cols, X, ldx, kernel, bandwidth, n, alpha, B, ldb1, beta, C, ldc1),
                    "RBFCrossKernel");
    }

    /// G (rows_x x (mz n), ldg >= rows_x; DEVICE) = the gradients with respect to the points of Z of alpha * K(Z, X) * B, B nx x n: column
    /// r * mz + i is the gradient at Z(:, i) of right-hand side r, laid out like Z (rlhip_pdk_cross_grad_*).  G is not read.
    void grad(int64_t n, T alpha, const T* B, int64_t ldb, T* G, int64_t ldg) {
        randlapack_require(ldb >= n_cols) << "ldb=" << ldb << " < " << n_cols << " (ldb must be >= the columns of K)";
        randlapack_require(ldg >= rows_x) << "ldg=" << ldg << " < rows_x=" << rows_x;
        blas::check(_pdk_impl::cross_grad(q, rows_x, n_rows, Z, ldz, n_cols, X, ldx, kernel, bandwidth, n, alpha, B, ldb > 0 ? ldb : 1, G, ldg),
                    "RBFCrossKernel::grad");
    }

    /// y = alpha * op(K) * x + beta * y
    void matvec(blas::Op trans, T alpha, const T* x, T beta, T* y) {
        const bool tr = trans != blas::Op::NoTrans;
        (*this)(blas::Layout::ColMajor, trans, 1, alpha, x, tr ? n_rows : n_cols, beta, y, tr ? n_cols : n_rows);
    }

    /// Ksub (rows_ksub x cols_ksub, ldk; 0 = rows_ksub) = K(ro_ksub : ro_ksub + rows_ksub, co_ksub : co_ksub + cols_ksub), DEVICE
    void submatrix(int64_t rows_ksub, int64_t cols_ksub, T* Ksub, int64_t ro_ksub, int64_t co_ksub, int64_t ldk = 0) {
        if (ldk <= 0) ldk = rows_ksub > 0 ? rows_ksub : 1;
        blas::check(_pdk_impl::cross_submatrix(q, rows_x, n_rows, Z, ldz, (const T*)nullptr, n_cols, X, ldx, (const T*)nullptr, rows_ksub, cols_ksub,
                                               Ksub, ldk, ro_ksub, co_ksub, kernel, bandwidth), "RBFCrossKernel::submatrix");
    }
};

}  // namespace linops
}  // namespace RandLAPACK
