"""numpy restatement of the regularization path of restricted kernel ridge regression (include/RandLAPACK_amd/rl_krill.hh:
krill_restricted_rpchol_cv, krill_restricted_cv; randlapack_amd/csrc/pcg.hip: rlhip_ridge_loo_*).

For min_y |F y - h|^2 + mu |y|^2 with the thin SVD F = U diag(sigma) W^T and C = U^T H the fitted values are U diag(d) U^T h with
d_j = sigma_j^2 / (sigma_j^2 + mu), and leaving point i out leaves the residual (Sherman-Morrison, exact)

    e_i = (h_i - yhat_i) / (1 - s_i),   s_i = sum_j U_ij^2 d_j,   yhat_i = sum_j U_ij d_j C_j.

  table()        loo(m, c) = sum_i e_ic(mu_m)^2 and rss(m, c) = sum_i (h_ic - yhat_ic(mu_m))^2 in np.longdouble from inputs taken as they are,
                 and next to every entry a first-order running-error bound for sums of k terms taken in double in any order;
  brute_force()  the leave-one-out residuals by n refits without row i;
  path()         the device's algorithm in a given dtype: LAPACK's SVD of F and C = U^T H in that dtype, then table();
  criterion(), select()   the two criteria and the selection rule;
  targets()      the right-hand sides of the driver tests.

The bound.  With u = 2^-53, gam = (k + 8) u, R_i = |h_i| + sum_j |U_ij d_j C_j| and t_i = 1 - s_i, a computed yhat_i is off by at most
(k + 2) u sum_j |U_ij d_j C_j| (k products of three factors, the table entry d_j C_j rounded once, k - 1 additions), d_j carries three
roundings (the square, the fused multiply-add, the division), the subtraction from h_i one more: the residual r_i is off by at most gam R_i.
s_i <= 1 is a sum of k positive terms, off by at most gam s_i <= gam, and 1 - s_i adds one rounding, so t_i is off by at most 2 gam and
e_i = r_i / t_i by gam R_i / t_i + 2 gam |e_i| / t_i.  The square doubles the relative error, and a sum of n terms in any order adds n u:

    bound_loo = sum_i 2 |e_i| (gam R_i / t_i + 2 gam |e_i| / t_i) + n u sum_i e_i^2
    bound_rss = sum_i 2 |r_i| gam R_i + n u sum_i r_i^2                                (the same with t_i = 1 exactly)

Inputs of type float32 are exact in double, so both precisions share the bound."""
from __future__ import annotations

import numpy as np

L = np.longdouble
U53 = 2.0 ** -53
LOO, GCV = 0, 1


def d_factor(sigma, mus, rcond=0.0):
    """d(j, m) = sigma_j^2 / (sigma_j^2 + mu_m) in extended precision; mu_m == 0: 1, or 0 where sigma_j <= rcond sigma_0"""
    sg = np.asarray(sigma).astype(L)[:, None]
    mu = np.asarray(mus).astype(L)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = sg * sg / (sg * sg + mu)
    zero = np.broadcast_to(mu == 0, d.shape)
    cut = np.broadcast_to(sg <= L(rcond) * sg[0, 0], d.shape)
    return np.where(zero, np.where(cut, L(0), L(1)), d)


def dof(sigma, mus, rcond=0.0):
    return d_factor(sigma, mus, rcond).sum(axis=0).astype(np.float64)


def rows(U, sigma, C, H, mus, rcond=0.0):
    """per row: (e, r, t, R) with e, r, R of shape (n, g, ell) and t of shape (n, g), all np.longdouble"""
    U = np.asarray(U).astype(L)
    C = np.asarray(C).astype(L)
    H = np.asarray(H).astype(L)
    d = d_factor(sigma, mus, rcond)                                          # k x g
    s = (U * U) @ d                                                          # n x g
    yhat = np.einsum("ij,jm,jc->imc", U, d, C)
    R = np.abs(H)[:, None, :] + np.einsum("ij,jm,jc->imc", np.abs(U), d, np.abs(C))
    r = H[:, None, :] - yhat
    t = 1 - s
    with np.errstate(divide="ignore", invalid="ignore"):
        e = r / t[:, :, None]
    return e, r, t, R


def table(U, sigma, C, H, mus, rcond=0.0):
    """dict(loo, rss, bound_loo, bound_rss: g x ell np.longdouble; min_t: the smallest 1 - s_i over rows and grid values)"""
    n, k = np.asarray(U).shape
    e, r, t, R = rows(U, sigma, C, H, mus, rcond)
    gam = L((k + 8) * U53)
    tt = t[:, :, None]
    loo, rss = (e * e).sum(axis=0), (r * r).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound_loo = (2 * np.abs(e) * (gam * R / tt + 2 * gam * np.abs(e) / tt)).sum(axis=0) + n * L(U53) * loo
    bound_rss = (2 * np.abs(r) * gam * R).sum(axis=0) + n * L(U53) * rss
    return dict(loo=loo, rss=rss, bound_loo=bound_loo, bound_rss=bound_rss, min_t=float(t.min()) if t.size else 1.0)


def brute_force(F, H, mu):
    """(n x ell) leave-one-out residuals h_i - f_i^T y_(-i), y_(-i) the minimizer of |F y - h|^2 + mu |y|^2 without row i, in float64"""
    F = np.asarray(F, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    n, k = F.shape
    out = np.empty_like(H)
    for i in range(n):
        keep = np.arange(n) != i
        Fi = F[keep]
        y = np.linalg.solve(Fi.T @ Fi + mu * np.eye(k), Fi.T @ H[keep])
        out[i] = H[i] - F[i] @ y
    return out


def path(F, H, mus, dtype, n_for_rcond=None):
    """the device's algorithm with LAPACK's SVD: U, sigma and C = U^T H in dtype, mus rounded to dtype, then table() on them"""
    T = dtype
    F = np.asarray(F, dtype=T)
    H = np.asarray(H, dtype=T)
    n = F.shape[0] if n_for_rcond is None else n_for_rcond
    U, sg, _ = np.linalg.svd(F, full_matrices=False)
    assert U.dtype == T
    C = (U.T @ H).astype(T)
    mus_t = np.asarray(mus, dtype=T)
    rcond = float(T(n) * np.finfo(T).eps)
    out = table(U, sg, C, H, mus_t, rcond)
    out["dof"] = dof(sg, mus_t, rcond)
    return out


def criterion(kind, n, loo, rss, dof_):
    """g x ell float64: the leave-one-out sums, or generalized cross-validation n rss / (n - dof)^2"""
    if kind == LOO:
        return np.asarray(loo).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return n * np.asarray(rss).astype(np.float64) / ((n - np.asarray(dof_, dtype=np.float64)) ** 2)[:, None]


def select(crit):
    """per column the index of the smallest finite entry, the lower index on a tie; a column without a finite entry raises ValueError"""
    crit = np.asarray(crit, dtype=np.float64)
    best = np.empty(crit.shape[1], dtype=np.int64)
    for c in range(crit.shape[1]):
        col = np.where(np.isfinite(crit[:, c]), crit[:, c], np.inf)
        if not np.isfinite(col).any():
            raise ValueError(f"column {c} has no finite criterion")
        best[c] = int(np.argmin(col))                                        # argmin returns the first of equal minima
    return best


def runner_up_gap(crit):
    """per column (second smallest - smallest finite entry) / largest finite entry"""
    crit = np.asarray(crit, dtype=np.float64)
    gaps = np.zeros(crit.shape[1])
    for c in range(crit.shape[1]):
        col = np.sort(crit[np.isfinite(crit[:, c]), c])
        gaps[c] = (col[1] - col[0]) / col[-1] if col.size > 1 else np.inf
    return gaps


GRID = tuple(10.0 ** p for p in range(-6, 2))                                # 1e-6 ... 1e1 in decades


def targets(X, s, dtype, rng):
    """H(i, c) = sin(2 pi (c + 1) x_0) cos(pi x_last) + 0.3 * standard normal, rounded to dtype; rng continues after the points were drawn"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    noise = rng.standard_normal((n, s))
    c = np.arange(1, s + 1)[None, :]
    H = np.sin(2 * np.pi * c * X[0][:, None]) * np.cos(np.pi * X[-1])[:, None] + 0.3 * noise
    return H.astype(dtype).astype(np.float64)


def problem(n, rows_x, s, dtype):
    """the points of tests/test_gpu_krr_restricted.py (uniform in the unit cube, seed 1000 n, rounded to dtype) with the targets above"""
    rng = np.random.default_rng(1000 * n)
    X = rng.random((rows_x, n)).astype(dtype).astype(np.float64)
    H = targets(X, s, dtype, rng)
    X.setflags(write=False)
    H.setflags(write=False)
    return X, H
