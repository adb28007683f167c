"""numpy restatement of the two-point-set RBF kernel and of kernel ridge regression fit-then-predict, in float64: what tests/test_krr_model.py
checks against closed forms and tests/test_gpu_krr.py compares the device against (rlhip_rbf_cross_apply_*, rlhip_sqexp_cross_submatrix_*,
RandLAPACK::krr_predict)."""
from __future__ import annotations

import numpy as np


def cross_kernel(Z, X, bandwidth):
    """K(Z, X)(i, j) = exp(-|Z(:, i) - X(:, j)|^2 / (2 h^2)) by differences; Z: rows_x x mz, X: rows_x x nx (one column per point)"""
    Z = np.asarray(Z, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros((Z.shape[1], X.shape[1]))
    for r in range(Z.shape[0]):                      # row by row: no rows_x x mz x nx temporary
        D += (Z[r][:, None] - X[r][None, :]) ** 2
    return np.exp(-D / (2.0 * bandwidth * bandwidth))


def cross_apply(Z, X, bandwidth, B, alpha=1.0, beta=0.0, C0=None):
    """(alpha K(Z, X) B + beta C0, |alpha| |K| |B| + |beta| |C0|): the result and the magnitude that a componentwise error bound scales with"""
    K = cross_kernel(Z, X, bandwidth)
    B = np.asarray(B, dtype=np.float64)
    out = alpha * (K @ B)
    mag = abs(alpha) * (np.abs(K) @ np.abs(B))
    if beta != 0.0:
        out = out + beta * np.asarray(C0, dtype=np.float64)
        mag = mag + abs(beta) * np.abs(np.asarray(C0, dtype=np.float64))
    return out, mag


def fit(X, bandwidth, mus, H):
    """coefficients of kernel ridge regression by a dense solve: column i solves (K(X, X) + mu_i I) a = H(:, i) (one mu: for every column)"""
    K = cross_kernel(X, X, bandwidth)
    H = np.asarray(H, dtype=np.float64)
    mus = np.broadcast_to(np.asarray(mus, dtype=np.float64), (H.shape[1],))
    return np.stack([np.linalg.solve(K + mu * np.eye(K.shape[0]), H[:, i]) for i, mu in enumerate(mus)], axis=1)


def predict(Z, X, bandwidth, coeffs):
    """Y = K(Z, X) coeffs"""
    return cross_kernel(Z, X, bandwidth) @ np.asarray(coeffs, dtype=np.float64)
