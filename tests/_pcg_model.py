"""numpy restatement of block / lockstep PCG (RandLAPACK/comps/rl_determiter.hh:154-493) and of the spectral preconditioner
(RandLAPACK/linops/rl_sym_linops.hh:204-379), statement by statement, in the precision `dtype`.  The GPU tests compare the device
solver (include/RandLAPACK_amd/rl_determiter.hh, randlapack_amd/csrc/pcg.hip) against it; numpy only."""
from __future__ import annotations

import numpy as np


def zero_off_diagonal(mat):
    """rl_determiter.hh:154-161"""
    return np.diag(np.diag(mat)).astype(mat.dtype)


def psd_sqrt_pinv(A, dtype):
    """rl_determiter.hh:181-207.  Returns (code, B, w): code = dim(ker A), or -(n+1) when A is not PSD, -(n+2) when it is zero up to
    rounding (the reference's CODE; its comment has the two swapped); the trailing n - code columns of B satisfy pinv(A) = B B^T."""
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    w, B = np.linalg.eigh(np.tril(A) + np.tril(A, -1).T)                     # :187  syevd(Vec, Lower)
    w, B = w.astype(dtype), B.astype(dtype)
    rel_tol = dtype(10) * np.finfo(dtype).eps                                  # :188
    abs_tol = rel_tol * max(dtype(1), w[n - 1])                                # :189
    if w[0] < -abs_tol:
        return -(n + 1), B, w                                                  # :190-192
    if w[n - 1] < abs_tol:
        return -(n + 2), B, w                                                  # :193-195
    ker = n
    while ker > 0:                                                             # :198-205
        if w[ker - 1] > abs_tol:
            B[:, ker - 1] *= dtype(1) / np.sqrt(w[ker - 1])
            ker -= 1
        else:
            break
    return ker, B, w


def posm_square(LHS, RHS, dtype, diag_only=False):
    """rl_determiter.hh:231-282.  Returns (code, RHS_new): code = rank(LHS) or psd_sqrt_pinv's error; RHS_new is RHS itself on an error.
    diag_only: zero_off_diagonal applied to both first (what pcg's lockstep mode feeds it)."""
    LHS = np.asarray(LHS, dtype=dtype)
    RHS = np.asarray(RHS, dtype=dtype)
    n = LHS.shape[0]
    if diag_only:
        LHS, RHS = zero_off_diagonal(LHS), zero_off_diagonal(RHS)
    sym = np.tril(LHS) + np.tril(LHS, -1).T
    d = np.diag(sym)
    try:                                                                       # :246  potrf(Lower)
        if not np.all(np.isfinite(sym)):
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(sym).astype(dtype)
        if not np.all(np.diag(L) > 0) or not np.all(d > 0):
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        L = None
    if L is not None:
        if diag_only:                                                          # the two solves of :248-255 on a diagonal factor
            l = np.diag(L)
            return n, np.diag((np.diag(RHS) / l) / l).astype(dtype)
        y = np.linalg.solve(L, RHS).astype(dtype)                              # :248-251
        return n, np.linalg.solve(L.T, y).astype(dtype)                        # :252-255
    ker, B, _ = psd_sqrt_pinv(sym, dtype)                                      # :262
    if ker < 0:
        return ker, RHS
    if ker == n:
        return 0, np.zeros_like(RHS)                                           # :265-269
    pinv_sqrt = B[:, ker:]                                                     # :272
    work = (pinv_sqrt.T @ RHS).astype(dtype)                                   # :275-277
    return n - ker, (pinv_sqrt @ work).astype(dtype)                           # :278-280


class SpectralPrecond:
    """rl_sym_linops.hh:204-379: P_r = V diag(D_r) V^T + I with D_r = (eigvals[-1] + mu_r) / (eigvals + mu_r) - 1"""

    def __init__(self, V, eigvals, mus, dtype):
        self.dtype = dtype
        self.V = np.asarray(V, dtype=dtype)
        ev = np.asarray(eigvals, dtype=dtype)
        mus = np.asarray(mus, dtype=dtype)
        self.num_ops = mus.size
        self.D = np.stack([(ev[-1] + mu) / (ev + mu) - dtype(1) for mu in mus], axis=1).astype(dtype)      # :306-316, dim_pre x num_ops

    def __call__(self, B, alpha=1.0, beta=0.0, C=None):
        dt = self.dtype
        B = np.asarray(B, dtype=dt)
        W = (self.V.T @ B).astype(dt)                                          # :344
        W = (W * (self.D if self.num_ops != 1 else self.D[:, :1])).astype(dt)  # :349-353
        out = dt(alpha) * B if C is None or beta == 0 else dt(beta) * np.asarray(C, dtype=dt) + dt(alpha) * B     # :362-371
        return (out + dt(alpha) * (self.V @ W)).astype(dt)                     # :376 (with the alpha its comment gives it)


def reg_op(K, mus, dtype):
    """G(B) = K B + B diag(mu_i) (one mu: for every column): RegExplicitSymLinOp / RBFKernelMatrix with eval_includes_reg"""
    K = np.asarray(K, dtype=dtype)
    mus = np.asarray(mus, dtype=dtype)

    def G(B):
        B = np.asarray(B, dtype=dtype)
        m = mus if mus.size != 1 else np.full(B.shape[1], mus[0], dtype=dtype)
        return (K @ B + B * m[None, :]).astype(dtype)

    G.num_ops = mus.size
    return G


def rbf_kernel(pts, h, dtype):
    """K(i, j) = exp(-|x_i - x_j|^2 / (2 h^2)), pts: rows_x x n (one column per point)"""
    p = np.asarray(pts, dtype=np.float64)
    sq = np.sum(p * p, axis=0)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (p.T @ p), 0.0)
    np.fill_diagonal(d2, 0.0)
    return np.exp(-d2 / (2.0 * h * h)).astype(dtype)


def fro(M, dtype):
    """the norm the device solver records: squared column norms summed in double, their sum's root cast to dtype"""
    M64 = np.asarray(M, dtype=np.float64)
    return dtype(np.sqrt(np.sum(np.sum(M64 * M64, axis=0))))


def pcg(G, H, tol, max_iters, N, X0, dtype):
    """rl_determiter.hh:371-493.  G, N: callables on n x s blocks (G.num_ops > 1 selects the lockstep mode).  Returns
    (X, iters, normR, normNR): iters = iterations started, the norms as recorded by StatefulFrobeniusNorm (iteration 0 first)."""
    H = np.asarray(H, dtype=dtype)
    X = np.array(X0, dtype=dtype)
    n, s = H.shape
    sep = G.num_ops > 1                                                        # :386
    if sep:
        assert s == G.num_ops
    R = H.copy()
    GP = G(X)                                                                  # :410
    R = (R - GP).astype(dtype)                                                 # :412
    P = N(R)                                                                   # :414
    RNR = (R.T @ P).astype(dtype)                                              # :416
    if sep:
        RNR = zero_off_diagonal(RNR)                                           # :418
    alpha = RNR.copy()                                                         # :420
    k = 0
    normR, normNR = [fro(R, dtype)], [fro(P, dtype)]                           # :424-425
    stop_abstol = dtype(tol) * (dtype(1) + normNR[0])                          # :426
    subspace_dim = 0
    while subspace_dim < n and k < max_iters:                                  # :430
        k += 1
        GP = G(P)                                                              # :436
        ableft = (P.T @ GP).astype(dtype)                                      # :438
        incr, alpha = posm_square(ableft, alpha, dtype, diag_only=sep)         # :440-441
        if sep and incr > 0:
            incr = 1                                                           # :443-444
        if incr < -s:
            break                                                              # :446-447
        subspace_dim += incr
        X = (X + P @ alpha).astype(dtype)                                      # :450
        R = (R - GP @ alpha).astype(dtype)                                     # :452
        normR.append(fro(R, dtype))                                            # :460
        NR = N(R)                                                              # :462
        normNR.append(fro(NR, dtype))                                          # :464
        if normNR[-1] < stop_abstol:
            break                                                              # :467-468
        ableft = RNR.copy()                                                    # :472
        RNR = (R.T @ NR).astype(dtype)                                         # :474
        if sep:
            RNR = zero_off_diagonal(RNR)                                       # :476
        alpha = RNR.copy()                                                     # :477
        err, beta = posm_square(ableft, alpha.copy(), dtype, diag_only=sep)    # :479-481
        if err < -s:
            break                                                              # :483-484
        P = (NR + P @ beta).astype(dtype)                                      # :485-488
    return X, k, np.array(normR, dtype=dtype), np.array(normNR, dtype=dtype)


def reference_check(X, Xstar, dtype):
    """test/drivers/test_krill.cc:60-65: |X - X*| <= atol + rtol |X*| with atol = sqrt(n) eps^0.5, rtol = sqrt(n) atol.  Returns the largest
    ratio of the error to its allowance (the check holds when it is <= 1)."""
    n = Xstar.shape[0]
    atol = np.sqrt(n) * np.sqrt(float(np.finfo(dtype).eps))
    rtol = np.sqrt(n) * atol
    X64, S64 = np.asarray(X, dtype=np.float64), np.asarray(Xstar, dtype=np.float64)
    return float(np.max(np.abs(X64 - S64) / (atol + rtol * np.abs(S64))))


# ---- the cases of the solver tests (shared by test_pcg_model.py and test_gpu_pcg.py): operator, exact top-k eigenpairs, modes
def dense_case(seed=0, n=300, k=40):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    K = (Q * (1.0 / (1.0 + np.arange(n)) ** 2)) @ Q.T
    K = 0.5 * (K + K.T)
    return dict(kind="dense", n=n, k=k, K=K, mus=(1e-3, 1e-2, 1e-1))


def rbf_case(n, k, seed=0, h=1.5, rows_x=3):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((rows_x, n))
    return dict(kind="rbf", n=n, k=k, pts=pts, h=h, K=rbf_kernel(pts, h, np.float64), mus=(1e-2, 1e-1, 1.0))


def top_eigs(K, k):
    w, V = np.linalg.eigh(np.asarray(K, dtype=np.float64))
    return V[:, ::-1][:, :k].copy(), w[::-1][:k].copy()


MODES = (("lockstep", 3), ("block", 1), ("block", 8))


def mode_mus(case, mode):
    return case["mus"] if mode == "lockstep" else case["mus"][:1]
