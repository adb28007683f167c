"""numpy restatement of the positive-definite kernel family of the device library: the squared exponential and the Matern
kernels of order 3/2 and 5/2 as functions of the squared distance s = |z - x|^2,

    kind 0  exp(-s / (2 l^2))
    kind 1  (1 + a) exp(-a),              a = sqrt(3) sqrt(s) / l
    kind 2  (1 + a + a^2 / 3) exp(-a),    a = sqrt(5) sqrt(s) / l

in two forms.  The MODEL evaluates s by differences in float64: what tests/test_gpu_pdk.py compares the device against.  The EMULATION
follows the device's norm-expansion route statement by statement in the precision T (squared norms, -2 Z^T X, their sum, the clamp, the
constant rounded once from double, Horner): tests/test_pdk_model.py measures on it the error constants that the device tolerances are
derived from, so that nothing is tuned to the device.  MATERN12 exists for that file's one check of why exp(-sqrt(s) / l) is not part of
the library; the device has no such kind."""
from __future__ import annotations

import numpy as np

SQEXP, MATERN32, MATERN52 = 0, 1, 2
MATERN12 = -1
KINDS = (SQEXP, MATERN32, MATERN52)


def lipschitz(kind, l):
    """sup |dK/ds|: how far an absolute error of s moves an entry"""
    return {SQEXP: 1.0 / 2.0, MATERN32: 3.0 / 2.0, MATERN52: 5.0 / 6.0}[kind] / (l * l)


def kernel_of_s(kind, s, l):
    """K as a function of the squared distance s >= 0, float64"""
    s = np.asarray(s, dtype=np.float64)
    if kind == SQEXP:
        return np.exp(-s / (2.0 * l * l))
    if kind == MATERN12:
        return np.exp(-np.sqrt(s) / l)
    a = np.sqrt(3.0 if kind == MATERN32 else 5.0) * np.sqrt(s) / l
    poly = 1.0 + a if kind == MATERN32 else 1.0 + a + a * a / 3.0
    return poly * np.exp(-a)


def sqdist(Z, X):
    """|Z(:, i) - X(:, j)|^2 by differences; Z: rows_x x mz, X: rows_x x nx (one column per point)"""
    Z = np.asarray(Z, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros((Z.shape[1], X.shape[1]))
    for r in range(Z.shape[0]):                      # row by row: no rows_x x mz x nx temporary
        D += (Z[r][:, None] - X[r][None, :]) ** 2
    return D


def cross_kernel(kind, Z, X, l):
    return kernel_of_s(kind, sqdist(Z, X), l)


def cross_apply(kind, Z, X, l, B, alpha=1.0, beta=0.0, C0=None):
    """(alpha K(Z, X) B + beta C0, |alpha| |K| |B| + |beta| |C0|): the result and the magnitude that a componentwise error bound scales with"""
    K = cross_kernel(kind, Z, X, l)
    B = np.asarray(B, dtype=np.float64)
    out = alpha * (K @ B)
    mag = abs(alpha) * (np.abs(K) @ np.abs(B))
    if beta != 0.0:
        out = out + beta * np.asarray(C0, dtype=np.float64)
        mag = mag + abs(beta) * np.abs(np.asarray(C0, dtype=np.float64))
    return out, mag


def entry_scale(kind, Z, X, l):
    """1 + L_kind (|z_i|^2 + |x_j|^2): an entry's error bound is C_e eps_T times this"""
    Z = np.asarray(Z, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    return 1.0 + lipschitz(kind, l) * (np.sum(Z * Z, axis=0)[:, None] + np.sum(X * X, axis=0)[None, :])


# ---- the emulation in T of the norm-expansion route
def _sq_norms(P, T):
    nr = np.zeros(P.shape[1], dtype=T)
    for r in range(P.shape[0]):                      # the order of the device's norm kernel: row after row
        nr = (nr + P[r] * P[r]).astype(T)
    return nr


def expanded_s(Z, X, T):
    """(|z_i|^2 + |x_j|^2) + (-2 z_i . x_j) with every operation rounded to T; NOT clamped: entries may be negative"""
    Zt, Xt = np.asarray(Z, dtype=T), np.asarray(X, dtype=T)
    # The matrix product in T by numpy's BLAS: like the device's MFMA product it sums over the rows in an order of its own, not in the norm
    # kernel's, so for z == x the three terms cancel exactly only when there is one row.
    G = np.ascontiguousarray((T(-2) * Zt).T) @ Xt
    assert G.dtype == T
    return ((_sq_norms(Zt, T)[:, None] + _sq_norms(Xt, T)[None, :]).astype(T) + G).astype(T)


def constants(kind, l, T):
    """the two constants the device kernels take, each computed in double and rounded once to T: (scale, third).  scale is -1 / (2 l^2)
    for the squared exponential and sqrt(3) / l, sqrt(5) / l for the Matern kinds; third is 1 / 3 for Matern 5/2 and 0 otherwise."""
    if kind == SQEXP:
        return T(-1.0 / (2.0 * float(l) * float(l))), T(0)
    if kind == MATERN12:
        return T(1.0 / float(l)), T(0)
    return T(np.sqrt(3.0 if kind == MATERN32 else 5.0) / float(l)), T(1.0 / 3.0) if kind == MATERN52 else T(0)


def emulate_of_s(kind, s, l, T):
    """the device's entry formula on a given s, every operation rounded to T"""
    s = np.asarray(s, dtype=T)
    c, third = constants(kind, l, T)
    if kind == SQEXP:
        return np.exp((c * s).astype(T)).astype(T)                     # no clamp: the squared exponential never had one
    s = np.where(s < 0, T(0), s).astype(T)                             # s < 0 ? 0 : s -- a NaN stays
    a = (c * np.sqrt(s).astype(T)).astype(T)
    e = np.exp(-a).astype(T)
    if kind == MATERN12:
        return e
    poly = (T(1) + a).astype(T) if kind == MATERN32 else (T(1) + (a * (T(1) + (a * third).astype(T)).astype(T)).astype(T)).astype(T)
    return (poly * e).astype(T)


def emulate_kernel(kind, Z, X, l, T):
    return emulate_of_s(kind, expanded_s(Z, X, T), l, T)


def emulate_apply(kind, Z, X, l, B, T, alpha=1.0, beta=0.0, C0=None):
    """alpha K B + beta C0 with K emulated and the product accumulated in T, one point of X after the other"""
    K = emulate_kernel(kind, Z, X, l, T)
    Bt = np.asarray(B, dtype=T)
    acc = np.zeros((K.shape[0], Bt.shape[1]), dtype=T)
    for j in range(K.shape[1]):
        acc = (acc + K[:, j:j + 1] * Bt[j:j + 1, :]).astype(T)
    out = (T(alpha) * acc).astype(T)
    if beta != 0.0:
        out = (out + T(beta) * np.asarray(C0, dtype=T)).astype(T)
    return out
