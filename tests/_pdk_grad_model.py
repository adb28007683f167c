"""numpy restatement of the gradient of a kernel expansion with respect to the evaluation point,

    grad_z sum_j k(z, x_j) b_j = sum_j w(s_j) (z - x_j) b_j,    s_j = |z - x_j|^2,    w(s) = 2 dk/ds = w(0) u(s)

    kind 0  w(0) = -1 / l^2        u = exp(-s / (2 l^2))
    kind 1  w(0) = -3 / l^2        u = exp(-a)                a = sqrt(3) sqrt(s) / l
    kind 2  w(0) = -5 / (3 l^2)    u = (1 + a) exp(-a)        a = sqrt(5) sqrt(s) / l

in two forms, as tests/_pdk_model.py has the kernels themselves.  The MODEL (a) evaluates s and z - x by differences in float64: what the
device tests compare against.  The EMULATION (b) follows the device's expanded formula statement by statement in the precision T -- s by the
norm expansion, the clamp, the constants rounded once from double, B' = [b, x_c o b], the sums over j in T, and
alpha * (w(0) * (z_c T_0 - T_c)) -- so that the device tolerances rest on its error, not on the device's."""
from __future__ import annotations

import numpy as np

import _pdk_model as pk


def weight0(kind, l):
    """w(0), float64"""
    return {pk.SQEXP: -1.0, pk.MATERN32: -3.0, pk.MATERN52: -5.0 / 3.0}[kind] / (float(l) * float(l))


def weight_of_s(kind, s, l):
    """w(s) = 2 dk/ds for s >= 0, float64"""
    s = np.asarray(s, dtype=np.float64)
    if kind == pk.SQEXP:
        return weight0(kind, l) * np.exp(-s / (2.0 * l * l))
    a = np.sqrt(3.0 if kind == pk.MATERN32 else 5.0) * np.sqrt(s) / l
    return weight0(kind, l) * (np.exp(-a) if kind == pk.MATERN32 else (1.0 + a) * np.exp(-a))


def cross_grad(kind, Z, X, l, B, alpha=1.0):
    """(G, mag): G[c, r, i] = alpha sum_j w(s_ij) (Z[c, i] - X[c, j]) B[j, r] by differences in float64, and the magnitude
    |alpha| sum_j |w_ij| (|z_ic| + |x_jc|) |b_jr| that a componentwise error bound of the expanded formula scales with"""
    Z, X, B = (np.asarray(a, dtype=np.float64) for a in (Z, X, B))
    W = weight_of_s(kind, pk.sqdist(Z, X), l)                            # mz x nx
    d, mz = Z.shape
    G, mag = np.zeros((d, B.shape[1], mz)), np.zeros((d, B.shape[1], mz))
    for c in range(d):
        D = Z[c][:, None] - X[c][None, :]
        G[c] = alpha * ((W * D) @ B).T
        mag[c] = abs(alpha) * ((np.abs(W) * (np.abs(Z[c])[:, None] + np.abs(X[c])[None, :])) @ np.abs(B)).T
    return G, mag


def weight_constants(kind, l, T):
    """(w(0), scale, lin), each computed in double and rounded once to T: the kernel's own scale; lin = 0 for Matern 3/2, 1 for 5/2"""
    scale, _ = pk.constants(kind, l, T)
    return T(weight0(kind, l)), scale, T(1) if kind == pk.MATERN52 else T(0)


def emulate_u(kind, s, l, T):
    """u on a given s, every operation rounded to T; the Matern kinds clamp s at 0 by a select, the squared exponential does not"""
    s = np.asarray(s, dtype=T)
    _, c, lin = weight_constants(kind, l, T)
    if kind == pk.SQEXP:
        return np.exp((c * s).astype(T)).astype(T)
    s = np.where(s < 0, T(0), s).astype(T)
    a = (c * np.sqrt(s).astype(T)).astype(T)
    poly = (T(1) + (a * lin).astype(T)).astype(T)                        # fma(a, lin, 1): a * lin is exact for lin in {0, 1}
    return (poly * np.exp(-a).astype(T)).astype(T)


def emulate_grad(kind, Z, X, l, B, T, alpha=1.0):
    """G[c, r, i] by the expanded formula in T: T_0 = U b, T_c = U (x_c o b) accumulated one point of X after the other,
    alpha * (w(0) * fma(z_c, T_0, -T_c))"""
    Zt, Xt, Bt = (np.asarray(a, dtype=T) for a in (Z, X, B))
    U = emulate_u(kind, pk.expanded_s(Z, X, T), l, T)                    # mz x nx
    w0, _, _ = weight_constants(kind, l, T)
    d, mz = Zt.shape
    n = Bt.shape[1]
    out = np.zeros((d, n, mz), dtype=T)

    def apply(Bp):
        acc = np.zeros((mz, n), dtype=T)
        for j in range(U.shape[1]):
            acc = (acc + U[:, j:j + 1] * Bp[j:j + 1, :]).astype(T)
        return acc

    T0 = apply(Bt)
    for c in range(d):
        Tc = apply((Bt * Xt[c][:, None]).astype(T))
        # the fused multiply-add: the product is exact in the wider type (float32) or rounded once more at 1e-19 relative (float64)
        f = (Zt[c].astype(np.longdouble)[:, None] * T0.astype(np.longdouble) - Tc.astype(np.longdouble)).astype(T)
        out[c] = (T(alpha) * (w0 * f).astype(T)).astype(T).T
    return out
