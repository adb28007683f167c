"""numpy restatement, at a given dtype, of the reference's sketch-and-precondition least-squares pieces: pcg_saddle
(RandLAPACK/comps/rl_determiter.hh:18-134, including the residual refresh on iter % 25 == 1 and the stop test), rpc_data_svd on a dense S
(comps/rl_preconditioners.hh:29-86) and make_right_orthogonalizer (:193-224).  Every array and every scalar of the loop is kept in the dtype
T, as the reference keeps them in its template type.  Also the problems the model test and the device test share."""
import functools

import numpy as np


def pcg_saddle(A, b, c, delta, iter_lim, tol, M, x0, T):
    """returns (x, y, iters, resid): resid[i] = delta_1 at the start of iteration i, and of the iteration not run (iters + 1 entries)"""
    A, b, c, M, x0 = (np.asarray(v, dtype=T) for v in (A, b, c, M, x0))
    delta, tol = T(delta), T(tol)
    b1 = A.T @ b - c                                                     # :49-50
    r = b1 - (A.T @ (A @ x0) + delta * x0)                               # :57-61
    d = M @ (M.T @ r)                                                    # :64-65
    reg = delta > 0                                                      # :67
    x = x0.copy()                                                        # :68
    d1_old = T(d @ r)                                                    # :69
    d1_new = d1_old
    rel_sq_tol = T(T(d1_old * tol) * tol)                                # :71
    resid = []
    it = 0
    with np.errstate(all="ignore"):
        while it < iter_lim and d1_new > rel_sq_tol:                     # :76
            resid.append(d1_new)                                         # :77
            q = A.T @ (A @ d)                                            # :81-82
            if reg:
                q = q + delta * d                                        # :83
            alpha = T(d1_new / T(d @ q))                                 # :86
            x = x + alpha * d                                            # :89
            if it % 25 == 1:                                             # :92
                r = b1 - A.T @ (A @ x)                                   # :99-102
                if reg:
                    r = r - delta * x                                    # :103
            else:
                r = r - alpha * q                                        # :106
            s = M @ (M.T @ r)                                            # :113-114
            d1_old = d1_new                                              # :117
            d1_new = T(r @ s)                                            # :118
            beta = T(d1_new / d1_old)                                    # :119
            d = beta * d + s                                             # :120-122
            it += 1                                                      # :124
    resid.append(d1_new)                                                 # :127
    y = b - A @ x                                                        # :130-131
    return x.astype(T), y.astype(T), it, np.array(resid, dtype=T)


def rpc_data_svd(A, S, T):
    """(V, sigma) of the sketch S A formed in the dtype T (:55-84).  The SVD of that sketch is taken in float64 and rounded to T: the
    library's Jacobi SVD runs an fp32 problem in fp64 (include/rlhip.h, rlhip_gesvdj_*)."""
    A_sk = np.asarray(S, dtype=T) @ np.asarray(A, dtype=T)
    _, sig, Vt = np.linalg.svd(A_sk.astype(np.float64), full_matrices=False)
    return Vt.T.astype(T), sig.astype(T)


def make_right_orthogonalizer(V, sigma, mu, T, cols_V=-1):
    """(M, rank): a copy of V with its first `rank` columns scaled by 1 / sqrt(sigma_i^2 + mu) (:193-224)"""
    V = np.array(V, dtype=T)
    n = V.shape[0]
    if cols_V < 0:
        cols_V = n
    sqrtmu = np.sqrt(np.float64(mu))

    def regularized(s):
        return T(s) if sqrtmu == 0 else T(np.hypot(np.float64(s), sqrtmu))

    curr = regularized(sigma[0])
    abstol = T(T(curr * T(cols_V)) * np.finfo(T).eps)
    rank = 0
    while rank < cols_V:
        curr = regularized(sigma[rank])
        if curr < abstol:
            break
        V[:, rank] *= T(T(1.0) / curr)
        rank += 1
    return V, rank


def precond_residual(A, b, c, delta, x, M):
    """||M^T (A^T (b - A x) - delta x - c)|| / ||M^T (A^T b - c)|| in float64"""
    A, b, c, x, M = (np.asarray(v, dtype=np.float64) for v in (A, b, c, x, M))
    num = M.T @ (A.T @ (b - A @ x) - delta * x - c)
    den = M.T @ (A.T @ b - c)
    return float(np.linalg.norm(num) / np.linalg.norm(den))


def cond(X):
    s = np.linalg.svd(np.asarray(X, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1])


# ---- shared problems.  S is the library's sparse sign operator restated by the oracle (oracle.saso_dense, independent columns) for the
# counter (0, 0, 0, 0) and the key the device test passes.
@functools.lru_cache(maxsize=None)
def saso(d, m, nnz, key):
    import oracle

    S, nxt = oracle.saso_dense(d, m, nnz, ctr=(0, 0, 0, 0), key=(key, 0), mode=1)
    S.setflags(write=False)
    return S, tuple(int(v) for v in nxt)


PRECOND_KEYS = (42, 1)
PRECOND_SHAPE = dict(m=500, n=10, d=30, nnz=8)


@functools.lru_cache(maxsize=None)
def precond_case(kind, key):
    """test_preconditioners.cc: a Gaussian 500 x 10 matrix, first column times 1e5, second times 1e-5 ('noreg', mu = 0); the same with
    the first column then zeroed and mu = 1e-6 ('reg')"""
    m, n = PRECOND_SHAPE["m"], PRECOND_SHAPE["n"]
    A = np.random.default_rng(1000 + key).standard_normal((m, n))
    A[:, 0] *= 1e5
    A[:, 1] *= 1e-5
    mu = 0.0
    if kind == "reg":
        A[:, 0] = 0.0
        mu = 1e-6
    A.setflags(write=False)
    return A, mu


CONV_SHAPES = ((3000, 64, 256), (4099, 33, 132), (2048, 128, 512))
CONV_NNZ = 8
CONV_KEY = 7
CONV_TOL = {np.float64: 1e-10, np.float32: 1e-4}
CONV_ITER_LIM = 60


@functools.lru_cache(maxsize=None)
def conv_case(m, n):
    """A = Gaussian diag(logspace(0, -6, n)), b Gaussian"""
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)) * np.logspace(0, -6, n)[None, :]
    b = rng.standard_normal(m)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def conv_model(m, n, d, prec, delta=0.0, zero_col=-1):
    """the model's solve of conv_case in the dtype `prec`: dict(A, b, M, rank, x, y, iters, resid, ratio)"""
    T = {"f64": np.float64, "f32": np.float32}[prec]
    A, b = conv_case(m, n)
    if zero_col >= 0:
        A = A.copy()
        A[:, zero_col] = 0.0
    A, b = A.astype(T), b.astype(T)
    S, _ = saso(d, m, CONV_NNZ, CONV_KEY)
    V, sig = rpc_data_svd(A, S, T)
    Mfull, rank = make_right_orthogonalizer(V, sig, delta, T)
    M = Mfull[:, :rank]
    c = np.zeros(n, dtype=T)
    x, y, it, resid = pcg_saddle(A, b, c, delta, CONV_ITER_LIM, CONV_TOL[T], M, np.zeros(n, dtype=T), T)
    return dict(A=A, b=b, c=c, M=M, rank=rank, x=x, y=y, iters=it, resid=resid, ratio=precond_residual(A, b, c, delta, x, M), sigma=sig)
