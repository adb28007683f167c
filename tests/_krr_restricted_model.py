"""numpy restatement of restricted kernel ridge regression (include/RandLAPACK_amd/rl_krill.hh: krill_restricted_rpchol, krill_restricted,
krr_predict_restricted), in three parts:

  (a) truth()      the float64 dense solve of (K_S^T K_S + mu K_SS) x = K_S^T h, K by differences (tests/_pdk_model.py);
  (b) algorithm()  the device's tail in a given dtype on a factor F of tests/_rpchol_model.py: M = F(S, :), thin SVD of F, C = U^T H, the
                   filter, Y = W C, back substitution with tril(M)^T -- LAPACK's SVD and a row-by-row solve instead of the device's Jacobi
                   SVD and blocked trsm;
  (c) ridge_filter() the filter alone, in extended precision.

tests/test_krr_restricted_model.py checks (b) against (a) on the CPU; tests/test_gpu_krr_restricted.py compares the device with (a) and bounds
its error by the error of (b) in the same dtype."""
from __future__ import annotations

import numpy as np

import _pdk_model as pk
import _rpchol_model as M


def truth(kind, X, l, S, mus, H):
    """(a): column i solves (K_S^T K_S + mu_i K_SS) x = K_S^T H(:, i) in float64; one mu: for every column.  Returns (alpha k x s, K_S)."""
    S = np.asarray(S, dtype=np.int64)
    KS = pk.cross_kernel(kind, X, np.asarray(X, dtype=np.float64)[:, S], l)
    KSS = KS[S, :]
    H = np.asarray(H, dtype=np.float64)
    mus = np.broadcast_to(np.asarray(mus, dtype=np.float64), (H.shape[1],))
    G = KS.T @ KS
    return np.stack([np.linalg.solve(G + mu * KSS, KS.T @ H[:, i]) for i, mu in enumerate(mus)], axis=1), KS


def ridge_filter(C, sigma, mus, rcond=0.0):
    """(c): C(j, i) * sigma_j / (sigma_j^2 + mu_i) in extended precision, exactly 0 where mu_i == 0 and sigma_j <= rcond sigma_0.  C, sigma and
    mus are taken as they are (already rounded to the dtype under test); the result is np.longdouble."""
    L = np.longdouble
    C = np.asarray(C).astype(L)
    sg = np.asarray(sigma).astype(L)[:, None]
    mu = np.broadcast_to(np.asarray(mus).astype(L), (C.shape[1],))[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = sg / (sg * sg + mu)
    cut = (mu == 0) & (sg <= L(rcond) * sg[0, 0])
    return C * np.where(cut, L(0), f)


def back_substitute_lower_trans(Mt, Y):
    """solve tril(Mt)^T a = Y row by row from the bottom, every operation in Y's dtype; the strict upper triangle of Mt is not read"""
    T = Y.dtype.type
    Lo = np.tril(np.asarray(Mt, dtype=T))
    k = Lo.shape[0]
    a = np.zeros_like(Y)
    for j in range(k - 1, -1, -1):
        a[j] = ((Y[j] - Lo[j + 1:, j] @ a[j + 1:]).astype(T) / Lo[j, j]).astype(T)
    return a


def filtered_solution(F, mus, H, dtype, n_for_rcond=None):
    """the part of (b) in front of the triangular solve: (Y, sigma) with Y = W diag(filter) U^T H, the minimizer of |F y - h|^2 + mu |y|^2
    (mu == 0: the minimum-norm one, singular values <= n eps sigma_0 cut), everything in dtype"""
    T = dtype
    F = np.asarray(F, dtype=T)
    H = np.asarray(H, dtype=T)
    n = F.shape[0] if n_for_rcond is None else n_for_rcond
    U, sg, Wt = np.linalg.svd(F, full_matrices=False)
    assert U.dtype == T
    C = (U.T @ H).astype(T)
    mus_t = np.asarray(mus, dtype=T)
    f = ridge_filter(np.ones((sg.size, H.shape[1]), dtype=T), sg, mus_t, float(T(n) * np.finfo(T).eps)).astype(T)   # the factor, rounded once
    C = (C * f).astype(T)
    return (Wt.T @ C).astype(T), sg


def algorithm(F, S, mus, H, dtype):
    """(b): the tail on the factor F (n x k, rows in point order, columns in selection order) with the centres S, everything in dtype.
    Returns dict(alpha k x s, M, sigma)."""
    F = np.asarray(F, dtype=dtype)
    Mt = F[np.asarray(S, dtype=np.int64), :].copy()                         # before the SVD: the device's SVD destroys F
    Y, sg = filtered_solution(F, mus, H, dtype)
    return dict(alpha=back_substitute_lower_trans(Mt, Y), M=Mt, sigma=sg)


def factor(kind, X, l, k, b, dtype, key=(0, 0), forced_S=None):
    """tests/_rpchol_model.rp_cholesky on the unregularized kernel matrix of the points X, columns by differences rounded to dtype"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    cols = lambda idx: pk.cross_kernel(kind, X, X[:, np.asarray(idx, dtype=np.int64)], l)
    return M.rp_cholesky(n, np.ones(n), cols, k, b, key=key, dtype=dtype, forced_S=forced_S)


def given_centres_factor(kind, X, l, S, dtype):
    """krill_restricted's factor: A = K(:, S), U = potrf_upper(A(S, :)), F = A U^-1.  Returns (F, info)."""
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(S, dtype=np.int64)
    A = pk.cross_kernel(kind, X, X[:, S], l).astype(dtype)
    U, info = M.potrf_upper(A[S, :])
    if info:
        return None, info
    return np.linalg.solve(U.T.astype(np.float64), A.T.astype(np.float64)).T.astype(dtype), 0


def predict(kind, Z, X, l, S, alpha):
    """(K(Z, X(:, S)) alpha, |K| |alpha|)"""
    K = pk.cross_kernel(kind, Z, np.asarray(X, dtype=np.float64)[:, np.asarray(S, dtype=np.int64)], l)
    a = np.asarray(alpha, dtype=np.float64)
    return K @ a, np.abs(K) @ np.abs(a)
