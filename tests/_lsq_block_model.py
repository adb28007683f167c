"""The model of pcg_saddle_block (include/RandLAPACK_amd/rl_determiter.hh) and the problems its two tests share.  The block
solver runs pcg_saddle's recurrence on every column and shares nothing between columns but the products, so its model is
_lsq_model.pcg_saddle, unchanged, run column by column: that is exact, not an approximation."""
import numpy as np

import _lsq_model as lm

DT = {"f64": np.float64, "f32": np.float32}


def pcg_saddle_block(A, B, C, delta, iter_lim, tol, M, X0, T):
    """B (m, s), C and X0 (n, s) or None.  Returns (X (n, s), Y (m, s), iters (list of s), resid (list of s arrays, iters[j] + 1 entries))"""
    A = np.asarray(A, dtype=T)
    m, n = A.shape
    B = np.asarray(B, dtype=T).reshape(m, -1)
    s = B.shape[1]
    C = np.zeros((n, s), dtype=T) if C is None else np.asarray(C, dtype=T).reshape(n, s)
    X0 = np.zeros((n, s), dtype=T) if X0 is None else np.asarray(X0, dtype=T).reshape(n, s)
    X, Y, iters, resid = np.zeros((n, s), dtype=T), np.zeros((m, s), dtype=T), [], []
    for j in range(s):
        x, y, it, r = lm.pcg_saddle(A, B[:, j].copy(), C[:, j].copy(), delta, iter_lim, tol, M, X0[:, j].copy(), T)
        X[:, j], Y[:, j] = x, y
        iters.append(it)
        resid.append(r)
    return X, Y, iters, resid


def three_step_case(name, T):
    """(A, b, c, delta, M, x0) of tests/test_gpu_lsq.py::_three_step_case, restated"""
    rng = np.random.default_rng(11)
    if name == "dense300":
        m, n = 300, 12
        return rng.standard_normal((m, n)), rng.standard_normal(m), np.zeros(n), 0.1, np.eye(n), np.zeros(n)
    m, n, d, delta = {"sketched4099": (4099, 33, 132, 0.0), "sketched2048": (2048, 128, 512, 0.1)}[name]
    A, b = lm.conv_case(m, n)
    S, _ = lm.saso(d, m, lm.CONV_NNZ, lm.CONV_KEY)
    V, sig = lm.rpc_data_svd(A.astype(T), S, T)
    M, rank = lm.make_right_orthogonalizer(V, sig, delta, T)
    if name == "sketched2048":                                         # c != 0 and x0 != 0
        return A, b, rng.standard_normal(n), delta, M[:, :rank], 1e-2 * rng.standard_normal(n)
    return A, b, np.zeros(n), delta, M[:, :rank], np.zeros(n)


def three_step_block(name, T):
    """(A, B (m, 3), C (n, 3), delta, M, X0 (n, 3)): column 0 the case itself, column 1 an independent Gaussian b with the case's c and,
    where the case uses zero for both c and x0, 1e-2 times a Gaussian for x0, column 2 the case's b times 1e6"""
    A, b, c, delta, M, x0 = three_step_case(name, T)
    m, n = A.shape
    rng = np.random.default_rng(12)
    b1 = rng.standard_normal(m)
    x1 = x0 if (np.any(x0) or np.any(c)) else 1e-2 * rng.standard_normal(n)
    B = np.stack([b, b1, 1e6 * b], axis=1)
    C = np.stack([c, c, c], axis=1)
    X0 = np.stack([x0, x1, x0], axis=1)
    return A, B, C, delta, M, X0


CONV_RHS = ("gaussian", "u_max", "u_max + u_min", "four spread", "zero")


def conv_rhs(A, M, b):
    """the five right-hand sides of the convergence test for the preconditioner M (n x rank), formed in float64: the case's Gaussian b;
    W u_max, W (u_max + u_min) and W times the sum of four spread eigenvectors, W = A M and u the eigenvectors of W^T W -- in the
    preconditioned variable their normal equations have a right-hand side in an invariant subspace of dimension 1, 2 and 4, so conjugate
    gradients ends in that many iterations; and zero"""
    A64, M64 = np.asarray(A, dtype=np.float64), np.asarray(M, dtype=np.float64)
    W = A64 @ M64
    _, U = np.linalg.eigh(W.T @ W)                                     # ascending
    r = U.shape[1]
    spread = [int(v) for v in np.linspace(0, r - 1, 4)]
    cols = [np.asarray(b, dtype=np.float64), W @ U[:, -1], W @ (U[:, -1] + U[:, 0]), W @ U[:, spread].sum(axis=1), np.zeros(A64.shape[0])]
    return np.stack(cols, axis=1)


def conv_block_model(A, M, B, prec):
    """the model's solve of the five columns with the preconditioner M: dict(iters, ratio (None for a zero column), X, Y, resid)"""
    T = DT[prec]
    A = np.asarray(A, dtype=T)
    n = A.shape[1]
    B = np.asarray(B, dtype=T)
    X, Y, iters, resid = pcg_saddle_block(A, B, None, 0.0, lm.CONV_ITER_LIM, lm.CONV_TOL[T], np.asarray(M, dtype=T), None, T)
    ratio = [lm.precond_residual(A, B[:, j], np.zeros(n), 0.0, X[:, j], M) if np.any(B[:, j]) else None for j in range(B.shape[1])]
    return dict(iters=iters, ratio=ratio, X=X, Y=Y, resid=resid)
