"""Shared cases of the sparse least-squares tests (test_splsq_cases.py without a GPU, test_gpu_splsq.py on one): small CSR matrices with
values in {-1, 0, 1} on which either precision must equal numpy bit for bit, and sparse convergence problems scaled like
_lsq_model.conv_case with the numpy model's own solve of the densified matrix as the yardstick.  numpy only; every array is computed
once and left read-only."""
import functools

import numpy as np

import _lsq_model as lm

CH = 512                      # RLHIP_SPMV_CHUNK (include/rlhip.h): entries of a chunk of the split route
X_LDS_BYTES = 32768           # RLHIP_SPMV_X_LDS_BYTES: x is staged in LDS when ncols * sizeof(T) is at most this
ROW_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 200)
NROWS = (1, 2, 5, 63, 64, 65, 257)
NCOLS = (1, 7, 64, 300)
LONG_LENGTHS = (0, CH - 1, CH, CH + 1, 3 * CH + 7)
ALPHA_BETA = ((1.0, 0.0), (-1.0, 1.0), (2.0, -0.5))
LANES = (-1, 4, 16, 64, 0)    # RLHIP_OPT_SPMV_LANES: default, the three widths, the split route
ROUTE_INDEX = {4: 50, 16: 51, 64: 52, 0: 53}


def default_route(nrows, nnz):
    """the documented choice of rlhip_csr_spmv_* (include/rlhip.h), from the mean row length alone"""
    mean = nnz // nrows
    if nrows <= 512 and mean >= 2 * CH:
        return 0
    return 4 if mean <= 64 else (16 if mean <= 1023 else 64)


def lds_limit(T):
    return X_LDS_BYTES // np.dtype(T).itemsize


def transpose_csr(nrows, ncols, rowptr, colidx, vals):
    """the CSR of the transpose by a stable sort on the column: entries of a transposed row keep the source order (ascending source row),
    duplicates and stored zeros stay separate entries -- what rlhip_csr_transpose_* builds"""
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(colidx, kind="stable")
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=ncols))]).astype(np.int64)
    return rowptr_t, rows[order], vals[order]


def densify(nrows, ncols, rowptr, colidx, vals):
    A = np.zeros((nrows, ncols))
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptr))
    np.add.at(A, (rows, colidx), vals)
    return A


def _csr_from_lengths(rng, lengths, ncols, distinct=True):
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cols = []
    for ln in lengths:
        cols.append(rng.permutation(ncols)[:ln] if distinct else rng.integers(0, ncols, size=ln))
    colidx = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, dtype=np.int64)
    vals = rng.integers(-1, 2, size=colidx.size).astype(np.float64)              # stored zeros included
    return rowptr, colidx, vals


def _finish(name, nrows, ncols, rowptr, colidx, vals, rng):
    case = dict(name=name, nrows=nrows, ncols=ncols, rowptr=rowptr, colidx=colidx, vals=vals)
    case["rowptr_t"], case["colidx_t"], case["vals_t"] = transpose_csr(nrows, ncols, rowptr, colidx, vals)
    case["A"] = densify(nrows, ncols, rowptr, colidx, vals)
    case["x"] = rng.integers(-1, 2, size=ncols).astype(np.float64)               # operand of A x, and d of the normal matvec
    case["xt"] = rng.integers(-1, 2, size=nrows).astype(np.float64)              # operand of A^T x
    case["y0"] = rng.integers(-3, 4, size=nrows).astype(np.float64)
    case["y0t"] = rng.integers(-3, 4, size=ncols).astype(np.float64)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def exact_cases(prec):
    """every exact case for the precision `prec` ('f64' / 'f32': the LDS staging limit of x depends on it)"""
    T = {"f64": np.float64, "f32": np.float32}[prec]
    lim = lds_limit(T)
    out = []
    shapes = [(nr, nc) for nr in NROWS for nc in NCOLS] + [(5, lim), (5, lim + 1), (65, lim), (65, lim + 1)]
    for k, (nr, nc) in enumerate(shapes):
        rng = np.random.default_rng(7000 + 31 * nr + nc)
        lengths = [min(ROW_LENGTHS[(k + i) % len(ROW_LENGTHS)], nc) for i in range(nr)]      # distinct columns: a row holds at most ncols
        out.append(_finish(f"{nr}x{nc}", nr, nc, *_csr_from_lengths(rng, lengths, nc), rng))
    rng = np.random.default_rng(7001)
    out.append(_finish("duplicates", 5, 7, *_csr_from_lengths(rng, [20, 0, 3, 65, 7], 7, distinct=False), rng))
    assert any(np.unique(out[-1]["colidx"][out[-1]["rowptr"][r]:out[-1]["rowptr"][r + 1]]).size < out[-1]["rowptr"][r + 1] - out[-1]["rowptr"][r]
               for r in range(5))
    out.append(_finish("all-empty", 5, 7, *_csr_from_lengths(rng, [0] * 5, 7), rng))
    ncl = 3 * CH + 40
    for i, ln in enumerate(LONG_LENGTHS):
        rng = np.random.default_rng(7100 + i)
        out.append(_finish(f"long1-{ln}", 1, ncl, *_csr_from_lengths(rng, [ln], ncl), rng))
        three = [LONG_LENGTHS[(i + j) % len(LONG_LENGTHS)] for j in range(3)]
        out.append(_finish(f"long3-{'-'.join(map(str, three))}", 3, ncl, *_csr_from_lengths(rng, three, ncl), rng))
    return tuple(out)


def exact_sum_bound(case):
    """the largest absolute partial sum any order of summation can meet in y = alpha A x + beta y0, A^T x likewise, and in the normal
    matvec q = A^T (A d) + delta d with d = x, its t = A d and d^T q"""
    A, x, xt = np.abs(case["A"]), np.abs(case["x"]), np.abs(case["xt"])
    rows = np.repeat(np.arange(case["nrows"]), np.diff(case["rowptr"]))
    absA = np.zeros_like(A)
    np.add.at(absA, (rows, case["colidx"]), np.abs(case["vals"]))                # duplicates: the entries, not their sum
    fwd = absA @ x
    bwd = absA.T @ xt
    worst_ab = max(abs(a) for a, _ in ALPHA_BETA), max(abs(b) for _, b in ALPHA_BETA)
    spmv = max(np.max(worst_ab[0] * fwd + worst_ab[1] * np.abs(case["y0"]), initial=0.0), np.max(worst_ab[0] * bwd + worst_ab[1] * np.abs(case["y0t"]), initial=0.0))
    t_abs = fwd
    q_abs = absA.T @ t_abs + 0.5 * x
    return float(max(spmv, np.max(t_abs, initial=0.0), np.max(q_abs, initial=0.0), float(x @ q_abs)))


# ---- convergence problems: sparse rows scaled by diag(logspace(0, -6, n)) as _lsq_model.conv_case scales its Gaussian matrix
CONV_ROW_NNZ = (4, 3, 6)      # nonzeros per row for the three shapes of lm.CONV_SHAPES


@functools.lru_cache(maxsize=None)
def conv_case(idx):
    """dict(m, n, d, rowptr, colidx, vals, A (dense), b): canonical CSR (sorted columns, no duplicates); every 97th row is empty, row 5 is full"""
    m, n, d = lm.CONV_SHAPES[idx]
    k = CONV_ROW_NNZ[idx]
    rng = np.random.default_rng(m + n + 1)
    scale = np.logspace(0, -6, n)
    lengths = np.full(m, k, dtype=np.int64)
    lengths[::97] = 0
    lengths[5] = n
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    colidx = np.concatenate([np.sort(rng.permutation(n)[:ln]) for ln in lengths]).astype(np.int64)
    vals = rng.standard_normal(colidx.size) * scale[colidx]
    b = rng.standard_normal(m)
    out = dict(m=m, n=n, d=d, rowptr=rowptr, colidx=colidx, vals=vals, A=densify(m, n, rowptr, colidx, vals), b=b)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def conv_model(idx, prec, delta=0.0, zero_col=-1):
    """the numpy model's solve (tests/_lsq_model.py) of the densified conv_case(idx) in the dtype `prec` with the oracle's sign operator for
    key lm.CONV_KEY: dict(A, b, c, M, rank, x, y, iters, resid, ratio, sigma)"""
    T = {"f64": np.float64, "f32": np.float32}[prec]
    cs = conv_case(idx)
    A = cs["A"]
    if zero_col >= 0:
        A = A.copy()
        A[:, zero_col] = 0.0
    A, b = A.astype(T), cs["b"].astype(T)
    S, nxt = lm.saso(cs["d"], cs["m"], lm.CONV_NNZ, lm.CONV_KEY)
    V, sig = lm.rpc_data_svd(A, S, T)
    Mfull, rank = lm.make_right_orthogonalizer(V, sig, delta, T)
    M = Mfull[:, :rank]
    c = np.zeros(cs["n"], dtype=T)
    x, y, it, resid = lm.pcg_saddle(A, b, c, delta, lm.CONV_ITER_LIM, lm.CONV_TOL[T], M, np.zeros(cs["n"], dtype=T), T)
    return dict(A=A, b=b, c=c, M=M, rank=rank, x=x, y=y, iters=it, resid=resid, ratio=lm.precond_residual(A, b, c, delta, x, M), sigma=sig,
                next_ctr=nxt)
