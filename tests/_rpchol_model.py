"""numpy restatement of randomly pivoted Cholesky (RandLAPACK/comps/rl_rpchol.hh), line by line, with the library's sampling stream
(include/rlhip.h, rlhip_sample_indices_iid_*) built on oracle.philox_np.  The GPU tests compare the device driver against it."""
from __future__ import annotations

import numpy as np

import oracle

CHUNK = 256


def prefix_sums(d):
    """(prefix, total, lastpos): w = max(d, 0) in double; sequential sums inside 256-chunks, sequential chunk offsets, prefix = off_c + loc_i"""
    w = np.maximum(np.asarray(d, dtype=np.float64), 0.0)
    w[np.isnan(w)] = 0.0
    n = w.size
    nch = (n + CHUNK - 1) // CHUNK
    loc = np.empty(n)
    S = np.empty(nch)
    for c in range(nch):
        seg = np.add.accumulate(w[c * CHUNK:(c + 1) * CHUNK])      # sequential, left to right
        loc[c * CHUNK:c * CHUNK + seg.size] = seg
        S[c] = seg[-1]
    off = np.concatenate([[0.0], np.add.accumulate(S)])
    chunk_of = np.arange(n) // CHUNK
    prefix = off[chunk_of] + loc
    pos = np.nonzero(w > 0)[0]
    return prefix, float(off[-1]), int(pos[-1]) if pos.size else -1


def weights_status(d, dtype):
    """2 if some d < -eps(T) or NaN, else 1 if the total < sqrt(n) eps(T), else 0"""
    eps = float(np.finfo(dtype).eps)
    d64 = np.asarray(d, dtype=np.float64)
    if np.any(np.isnan(d64)) or np.any(d64 < -eps):
        return 2
    _, total, _ = prefix_sums(d64)
    return 1 if total < np.sqrt(d64.size) * eps else 0


def uniforms(k, ctr, key):
    """u_j for j < k: Philox block ctr + j/2, words 2(j%2), 2(j%2)+1 -> 64 bits -> 53-bit uniform in (0, 1)"""
    nb = (k + 1) // 2
    if nb == 0:
        return np.zeros(0)
    W = oracle.philox_np(oracle._ctr_array(ctr, range(nb)), key).astype(np.uint64)
    j = np.arange(k)
    h = 2 * (j % 2)
    w = W[j // 2, h] | (W[j // 2, h + 1] << np.uint64(32))
    return ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def ctr_add(ctr, inc):
    return oracle._ctr_add(ctr, inc)


def sample(d, k, ctr, key, dtype=np.float64, unique=False):
    """(samples, status, next_ctr) of rlhip_sample_indices_iid_*"""
    st = weights_status(d, dtype)
    if st:
        return np.zeros(0, dtype=np.int64), st, tuple(int(c) for c in ctr)
    prefix, total, lastpos = prefix_sums(d)
    t = uniforms(k, ctr, key) * total
    idx = np.searchsorted(prefix, t, side="right")
    idx = np.minimum(np.where(idx >= prefix.size, lastpos, idx), lastpos).astype(np.int64)
    if unique:
        idx = np.unique(idx)
    return idx, 0, ctr_add(ctr, (k + 1) // 2)


def potrf_upper(G):
    """(U, info): LAPACK potrf('U') semantics; info = 1-based order of the first non-positive pivot, U valid in its leading info-1 block"""
    n = G.shape[0]
    U = np.zeros_like(G)
    for j in range(n):
        s = G[j, j] - U[:j, j] @ U[:j, j]
        if not s > 0:
            return U, j + 1
        U[j, j] = np.sqrt(s)
        U[j, j + 1:] = (G[j, j + 1:] - U[:j, j] @ U[:j, j + 1:]) / U[j, j]
    return U, 0


def rp_cholesky(n, diag, columns, k, b, ctr=(0, 0, 0, 0), key=(0, 0), dtype=np.float64, forced_S=None):
    """rl_rpchol.hh:114-187.  diag: the n diagonal entries; columns(idx) -> A[:, idx] (n x len(idx)).  forced_S: replay these pivots (a list of
    per-block sorted index arrays) instead of sampling.  Returns dict(F (n x k), S, k, status, c_status, next_ctr, d)."""
    T = dtype
    F = np.zeros((n, k), dtype=T)
    d = np.array(diag, dtype=T)
    S = []
    w_status = c_status = 0
    ell = 0
    blk = 0
    first = True
    while ell < k and w_status == 0 and c_status == 0:
        curr_B = min(b, k - ell)
        if forced_S is not None:
            if blk >= len(forced_S):
                break
            Sp, st, nxt = np.asarray(forced_S[blk], dtype=np.int64), 0, ctr
        else:
            Sp, st, nxt = sample(d, curr_B, ctr, key, T, unique=True)            # :141-143
        if st:
            if first:
                raise ValueError(f"weights_to_cdf status {st}")
            w_status = st
            break
        first = False
        ctr = nxt
        blk += 1
        cnt = Sp.size
        Fp = np.asarray(columns(Sp), dtype=T).copy()                                # :158
        if ell > 0:
            Fp -= F[:, :ell] @ F[Sp, :ell].T                                        # :160-165
        U, info = potrf_upper(Fp[Sp, :].astype(T))                                  # :169-170
        ell_incr = cnt
        if info:
            c_status = info
            ell_incr = info - 1                                                     # :171-173
        Sp = Sp[:ell_incr]
        Fp = Fp[:, :ell_incr]
        if ell_incr:
            Fp = np.linalg.solve(U[:ell_incr, :ell_incr].T.astype(np.float64), Fp.T.astype(np.float64)).T.astype(T)   # :174 (F U^-1)
        F[:, ell:ell + ell_incr] = Fp
        S.extend(int(s) for s in Sp)
        for j in range(ell_incr):                                                   # :51-56
            d -= Fp[:, j] * Fp[:, j]
        d[Sp] = 0                                                                   # :58-59
        ell += ell_incr
    if w_status == 0 and not first:
        w_status = weights_status(d, T)                                             # :184
    return dict(F=F[:, :ell], S=np.array(S, dtype=np.int64), k=ell, status=w_status, c_status=c_status, next_ctr=tuple(int(c) for c in ctr), d=d)


def rp_cholesky_dense(A, k, b, seed=None, ctr=(0, 0, 0, 0), key=(0, 0), dtype=np.float64, forced_S=None):
    if seed is not None:
        key = (seed, 0)                     # RandBLAS::RNGState(seed): key[0] = seed
    A = np.asarray(A, dtype=dtype)
    return rp_cholesky(A.shape[0], np.diag(A).copy(), lambda idx: A[:, idx], k, b, ctr, key, dtype, forced_S)


def sqexp_matrix(X, bandwidth, cols=None):
    """K(:, cols) of the RBF kernel of the points X (rows_x x n), by differences, in float64"""
    X = np.asarray(X, dtype=np.float64)
    cols = np.arange(X.shape[1]) if cols is None else np.asarray(cols)
    D = ((X[:, :, None] - X[:, None, cols]) ** 2).sum(axis=0)
    return np.exp(-D / (2.0 * bandwidth * bandwidth))


def blocks_of(S, sizes):
    out, p = [], 0
    for s in sizes:
        out.append(np.sort(S[p:p + s]))
        p += s
    return out


def kahan_gram(n, theta=1.2, perturb=10.0, dtype=np.float64):
    """(Gram, Kahan) of RandLAPACK::gen::gen_kahan_mat (testing/rl_gen.hh:409-434) in dtype, as test_rpchol.cc:77-86 builds it"""
    i = np.arange(n)
    Smat = np.diag(np.sin(theta) ** i)
    Cmat = np.triu(np.full((n, n), -np.cos(theta)), 1) + np.eye(n)
    K = (np.diag(perturb * np.finfo(np.float64).eps * (n - i)) + Smat @ Cmat).astype(dtype)
    return (K.T @ K).astype(dtype), K
