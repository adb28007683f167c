// KRILL, full kernel ridge regression (RandLAPACK/drivers/rl_krill.hh:20-55): randomly pivoted Cholesky of the unregularized kernel
// operator -> spectral preconditioner -> block or lockstep PCG on (K + mu_i I) x_i = h_i, all on the device.
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
#include <vector>
#include "rl_exceptions.hh"
#include "rl_blaspp.hh"
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
template <typename T>
void krr_predict(linops::RBFCrossKernel<T>& Kzx, int64_t s, const T* coeffs, int64_t ldcoef, T* Y, int64_t ldy) {
    randlapack_require(s >= 0) << "s=" << s << " must be >= 0";
    randlapack_require(coeffs != nullptr || s == 0 || Kzx.n_cols == 0) << "coeffs buffer must not be null";
    randlapack_require(Y != nullptr || s == 0 || Kzx.n_rows == 0) << "Y buffer must not be null";
    Kzx(blas::Layout::ColMajor, blas::Op::NoTrans, s, (T)1, coeffs, ldcoef, (T)0, Y, ldy);
}

}  // namespace RandLAPACK
