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
#pragma once
#include <cstdint>
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
#include "rl_lapackpp.hh"

namespace RandLAPACK {

namespace _pdk_impl {
inline int sqexp_submatrix(blas::Queue& q, int64_t rx, int64_t cx, const double* X, int64_t ldx, const double* nr, int64_t r, int64_t c,
                           double* K, int64_t ldk, int64_t ro, int64_t co, double h) {
    return rlhip_sqexp_submatrix_f64(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, h);
}
inline int sqexp_submatrix(blas::Queue& q, int64_t rx, int64_t cx, const float* X, int64_t ldx, const float* nr, int64_t r, int64_t c,
                           float* K, int64_t ldk, int64_t ro, int64_t co, float h) {
    return rlhip_sqexp_submatrix_f32(q.ctx(), rx, cx, X, ldx, nr, r, c, K, ldk, ro, co, h);
}
inline int sq_colnorms(blas::Queue& q, int64_t rx, int64_t cx, const double* X, int64_t ldx, double* nr) { return rlhip_sq_colnorms_f64(q.ctx(), rx, cx, X, ldx, nr); }
inline int sq_colnorms(blas::Queue& q, int64_t rx, int64_t cx, const float* X, int64_t ldx, float* nr) { return rlhip_sq_colnorms_f32(q.ctx(), rx, cx, X, ldx, nr); }
inline int columns(blas::Queue& q, int64_t rx, int64_t n, const double* X, int64_t ldx, int64_t nidx, const int64_t* idx, double h, double reg,
                   double* out, int64_t ldo) {
    return rlhip_sqexp_columns_f64(q.ctx(), rx, n, X, ldx, nidx, idx, h, reg, out, ldo);
}
inline int columns(blas::Queue& q, int64_t rx, int64_t n, const float* X, int64_t ldx, int64_t nidx, const int64_t* idx, float h, float reg,
                   float* out, int64_t ldo) {
    return rlhip_sqexp_columns_f32(q.ctx(), rx, n, X, ldx, nidx, idx, h, reg, out, ldo);
}
inline int apply(blas::Queue& q, int64_t rx, int64_t dim, const double* X, int64_t ldx, double h, const double* regs, int64_t nops, int eir,
                 int64_t n, double a, const double* B, int64_t ldb, double b, double* C, int64_t ldc) {
    return rlhip_rbf_apply_f64(q.ctx(), rx, dim, X, ldx, h, regs, nops, eir, n, a, B, ldb, b, C, ldc);
}
inline int apply(blas::Queue& q, int64_t rx, int64_t dim, const float* X, int64_t ldx, float h, const float* regs, int64_t nops, int eir,
                 int64_t n, float a, const float* B, int64_t ldb, float b, float* C, int64_t ldc) {
    return rlhip_rbf_apply_f32(q.ctx(), rx, dim, X, ldx, h, regs, nops, eir, n, a, B, ldb, b, C, ldc);
}
}  // namespace _pdk_impl

/// Ksub (rows_ksub x cols_ksub, ld rows_ksub) = the (ro_ksub, co_ksub)-offset block of K(i, j) = exp(-|X(:,i) - X(:,j)|^2 / (2 h^2)).
/// X (rows_x x cols_x, ld rows_x) and sq_colnorms_x (|X(:,j)|^2, cols_x entries) are DEVICE arrays, as Ksub.            rl_pdkernels.hh:133
template <typename T>
void squared_exp_kernel_submatrix(int64_t rows_x, int64_t cols_x, const T* X, T* sq_colnorms_x, int64_t rows_ksub, int64_t cols_ksub, T* Ksub,
                                  int64_t ro_ksub, int64_t co_ksub, T bandwidth, blas::Queue& q = blas::default_queue()) {
    randlapack_require(bandwidth > 0) << "kernel bandwidth must be > 0; got bandwidth=" << bandwidth;
    blas::check(_pdk_impl::sqexp_submatrix(q, rows_x, cols_x, X, rows_x, sq_colnorms_x, rows_ksub, cols_ksub, Ksub, rows_ksub > 0 ? rows_ksub : 1,
                                           ro_ksub, co_ksub, bandwidth), "squared_exp_kernel_submatrix");
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

    /// C (dim x n) = alpha * (K [+ diag(regs)]) * B + beta * C                                                            (:255-283)
    void operator()(blas::Layout layout, int64_t n, T alpha, T* const B, int64_t ldb, T beta, T* C, int64_t ldc) {
        randlapack_require(layout == blas::Layout::ColMajor) << "this kernel matrix only supports ColMajor layout";
        randlapack_require(ldb >= dim) << "ldb=" << ldb << " < dim=" << dim << " (ldb must be >= operator dimension)";
        randlapack_require(ldc >= dim) << "ldc=" << ldc << " < dim=" << dim << " (ldc must be >= operator dimension)";
        if (_eval_includes_reg) {
            randlapack_require(num_ops == 1 || n == num_ops) << "with num_ops>1, n=" << n << " must equal num_ops=" << num_ops
                                                             << " so each column gets its own regularization";
        }
        blas::check(_pdk_impl::apply(q, rows_x, dim, X, ldx, bandwidth, regs, num_ops, _eval_includes_reg ? 1 : 0, n, alpha, B, ldb, beta, C, ldc),
                    "RBFKernelMatrix");
    }

    /// the diagonal (DEVICE, dim entries): 1, or 1 + regs[0] when the evaluation includes the regularization (operator()(i, i), :285-292)
    void diag(T* d_dev) {
        const T v = T(1) + diag_reg();
        lapack::laset(MatrixType::General, dim, 1, v, v, d_dev, dim > 0 ? dim : 1, q);
    }
    /// out(:, l) = K(:, idx_dev[l]) (+ regs[0] on the diagonal), DEVICE indices and output (dim x nidx, ldo)
    void columns(int64_t nidx, const int64_t* idx_dev, T* out, int64_t ldo) {
        blas::check(_pdk_impl::columns(q, rows_x, dim, X, ldx, nidx, idx_dev, bandwidth, diag_reg(), out, ldo), "RBFKernelMatrix::columns");
    }

private:
    T diag_reg() const {
        if (!_eval_includes_reg) return T(0);
        randlapack_require(num_ops == 1) << "this operation requires num_ops=1; got num_ops=" << num_ops;
        return regs[0];
    }
};

}  // namespace linops
}  // namespace RandLAPACK
