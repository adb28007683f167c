"""-m gpu: every marked region of the scratch arena inside csrc/ is closed on the way out of its routine (rlhip_internal.h: ws_scope).

Each call below leaves its routine through a different exit of a marked region -- the early returns included -- on ordinary, legal inputs.
After every call the arena's stack must be back at 0 (rlhip_scratch_mark), and after the whole battery rlhip_reserve_workspace must still
be accepted: it answers -2 from then on if any region was left open.  The context is this module's own, so a mark left behind cannot be
another test's.  Numeric results are checked against numpy / LAPACK, return codes against the values include/rlhip.h documents.

Tolerances.  eps is the rounding unit of the precision under test.  A backward-stable factorization of an n-column matrix is held to a
small multiple of n eps ||A||; singular values to 100 n eps sigma_1 (one-sided Jacobi and the Cholesky-QR routes are both far inside it);
a Frobenius norm, accumulated in fp64 whatever the input, to 4 eps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
EPS = {p: float(np.finfo(t).eps) for p, t in NP.items()}
PRECS = ["f64", "f32"]


@pytest.fixture(scope="module")
def ctx():
    from randlapack_amd import device as dev

    c = dev.Context(0)
    yield c
    c.close()


def _cm(a, p):
    from randlapack_amd import device as dev

    return dev.cm_from_numpy(np.asarray(a, dtype=NP[p]))


def _np(t):
    from randlapack_amd import device as dev

    return dev.cm_to_numpy(t).astype(np.float64)


def _i64(v):
    import torch

    return torch.from_numpy(np.asarray(v, dtype=np.int64)).cuda()


def _closed(ctx):
    assert ctx.lib.rlhip_scratch_mark(ctx.h) == 0, "a marked region of the scratch arena was left open"


# ---------------------------------------------------------------------------------------------------------------------------------------
# lange_fro (aux.hip): the plain pass, the two early returns of the rescaled pass (all zero, NaN), and the rescaled pass itself
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
def test_lange_fro_every_exit(ctx, p):
    rng = np.random.default_rng(1)
    m, n = 300, 40
    A = rng.standard_normal((m, n)).astype(NP[p])
    got = ctx.lange_fro(m, n, _cm(A, p), m)
    _closed(ctx)
    assert abs(got - np.linalg.norm(A.astype(np.float64))) <= 4 * EPS[p] * np.linalg.norm(A.astype(np.float64))
    assert ctx.lange_fro(m, n, _cm(np.zeros((m, n)), p), m) == 0.0
    _closed(ctx)
    B = A.copy()
    B[17, 5] = np.nan
    assert np.isnan(ctx.lange_fro(m, n, _cm(B, p), m))
    _closed(ctx)
    if p == "f64":
        got = ctx.lange_fro(m, n, _cm(A * 1e200, p), m)           # the squares overflow: one more pass, relative to the largest entry
        _closed(ctx)
        assert abs(got / 1e200 - np.linalg.norm(A)) <= 4 * EPS[p] * np.linalg.norm(A)


# ---------------------------------------------------------------------------------------------------------------------------------------
# potrf (chol.hip): the one-workgroup kernel (n = 96) and the blocked route with its transposed copy (n = 600), info = 0 and info > 0
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("n,j", [(96, 40), (600, 300)])
def test_potrf_spd_and_not_positive_definite(ctx, p, n, j):
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, 2 * n))
    A = (G @ G.T / (2 * n) + np.eye(n)).astype(NP[p]).astype(np.float64)
    A = (A + A.T) / 2
    Ad = _cm(A, p)
    assert ctx.potrf(n, Ad, n) == 0
    _closed(ctx)
    U = np.triu(_np(Ad))
    assert np.linalg.norm(U.T @ U - A) <= 4 * n * EPS[p] * np.linalg.norm(A)
    # a_jj = -1: the leading minor of order j + 1 is the first that is not positive (the leading j x j block is still SPD)
    A[j, j] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A)
    assert ctx.potrf(n, _cm(A, p), n) == j + 1
    _closed(ctx)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the SVDs (jacobi.hip, svd.hip): gesvdj; gesdd by its Gram route, and by the classic route after the Gram route has declined
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
def test_gesvdj(ctx, p):
    import torch

    rng = np.random.default_rng(2)
    m, n = 64, 32
    A = rng.standard_normal((m, n)).astype(NP[p])
    Ad = _cm(A, p)
    S = torch.empty(n, dtype=Ad.dtype, device="cuda")
    VT = _cm(np.zeros((n, n)), p)
    info, _ = ctx.gesvdj(m, n, Ad, m, S, VT, n)
    _closed(ctx)
    assert info == 0
    A = A.astype(np.float64)
    Sref = np.linalg.svd(A, compute_uv=False)
    Sg = S.cpu().numpy().astype(np.float64)
    assert np.abs(Sg - Sref).max() <= 100 * n * EPS[p] * Sref[0]
    assert np.linalg.norm((_np(Ad) * Sg) @ _np(VT) - A) <= 100 * n * EPS[p] * np.linalg.norm(A)


@pytest.mark.parametrize("graded", [False, True])
def test_gesdd_gram_route_taken_and_declined(ctx, graded):
    import torch

    rng = np.random.default_rng(3)
    m, n = 400, 64
    A = rng.standard_normal((m, n))
    if graded:
        A = A * np.logspace(0, -8, n)                               # cond(A)^2 far beyond what the Gram matrix can carry: it returns 1
    Ad, Ud, VTd = _cm(A, "f64"), _cm(np.zeros((m, n)), "f64"), _cm(np.zeros((n, n)), "f64")
    S = torch.empty(n, dtype=torch.float64, device="cuda")
    sw = C.c_int(0)
    gram = ctx.path_count(10)
    assert ctx.lib.rlhip_gesdd_f64(ctx.h, m, n, Ad.data_ptr(), m, S.data_ptr(), Ud.data_ptr(), m, VTd.data_ptr(), n, C.byref(sw)) == 0
    _closed(ctx)
    assert ctx.path_count(10) - gram == (0 if graded else 1)
    Sref = np.linalg.svd(A, compute_uv=False)
    Sg = S.cpu().numpy()
    assert np.abs(Sg - Sref).max() <= 100 * n * EPS["f64"] * Sref[0]
    assert np.linalg.norm((_np(Ud) * Sg) @ _np(VTd) - A) <= 100 * n * EPS["f64"] * np.linalg.norm(A)


# ---------------------------------------------------------------------------------------------------------------------------------------
# trsm_gather (tri.hip): the fused attempt taken, the fused attempt refusing the pivot vector, the gather-copy route refusing it
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
def test_trsm_gather_fused_and_refusals(ctx, p):
    rng = np.random.default_rng(4)
    fn = getattr(ctx.lib, f"rlhip_trsm_gather_{p}")
    one = C.c_double(1.0) if p == "f64" else C.c_float(1.0)
    for m, n, fused in [(16384, 256, True), (512, 96, False)]:      # the smallest shape the fused solve serves; a gather-copy shape
        U = (np.triu(rng.standard_normal((n, n))) / np.sqrt(n) + 2 * np.eye(n)).astype(NP[p])
        Src = rng.standard_normal((m, n)).astype(NP[p])
        Ud, Sd = _cm(U, p), _cm(Src, p)
        jp = rng.permutation(n) + 1
        if fused:
            Bd = _cm(np.zeros((m, n)), p)
            took = ctx.path_count(4)
            assert fn(ctx.h, b"N", m, n, one, Ud.data_ptr(), n, Sd.data_ptr(), m, _i64(jp).data_ptr(), Bd.data_ptr(), m) == 0
            _closed(ctx)
            assert ctx.path_count(4) - took == 1
            X, U64, S64 = _np(Bd), U.astype(np.float64), Src.astype(np.float64)
            assert np.linalg.norm(X @ U64 - S64[:, jp - 1]) <= 4 * n * EPS[p] * np.linalg.norm(X) * np.linalg.norm(U64, 2)
        jp[7] = jp[3]                                                # a repeated index: not a permutation of 1..n
        Bd = _cm(np.full((m, n), -3.0), p)
        assert fn(ctx.h, b"N", m, n, one, Ud.data_ptr(), n, Sd.data_ptr(), m, _i64(jp).data_ptr(), Bd.data_ptr(), m) == -7
        _closed(ctx)
        assert bool((Bd == -3.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# col_swap (sketch.hip): the gather route of a small matrix, and the cycle walk (n >= 4096) with its host-side refusal
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
def test_col_swap_permutation_and_refusal(ctx, p):
    rng = np.random.default_rng(5)
    fn = getattr(ctx.lib, f"rlhip_col_swap_{p}")
    for m, n, refusal in [(8, 4096, -7), (30, 96, 0)]:             # (the gather route keeps its hands off the matrix and reports 0)
        A = rng.standard_normal((m, n)).astype(NP[p])
        perm = rng.permutation(n) + 1
        Ad = _cm(A, p)
        assert fn(ctx.h, m, n, n, Ad.data_ptr(), m, _i64(perm).data_ptr()) == 0
        _closed(ctx)
        assert np.array_equal(_np(Ad), A.astype(np.float64)[:, perm - 1])
        perm[9] = perm[2]
        Ad = _cm(A, p)
        assert fn(ctx.h, m, n, n, Ad.data_ptr(), m, _i64(perm).data_ptr()) == refusal
        _closed(ctx)
        ctx.sync()
        assert np.array_equal(_np(Ad), A.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stabilisers (house.hip, tri.hip): CholQRQ; HQRQ on a panel Cholesky-QR serves, and on one where it gives up (geqrf_q, then
# geqrf_cholqr inside geqrf, both leave through their "not good" exit) and the Householder kernels take over
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,deficient", [(0, False), (1, False), (1, True)])
def test_stabilisers_cholesky_qr_taken_and_given_up(ctx, kind, deficient):
    from randlapack_amd import device as dev

    rng = np.random.default_rng(6)
    m, k = 2000, 64
    Y = rng.standard_normal((m, k))
    if deficient:
        Y[:, 41] = Y[:, 12]                                          # two equal columns
    Yd = _cm(Y, "f64")
    rc, fail = dev.drv_stab(ctx, kind, Yd, m, k)
    _closed(ctx)
    assert rc == 0 and not fail
    Q = _np(Yd)
    assert np.linalg.norm(Q.T @ Q - np.eye(k)) <= 4 * k * EPS["f64"] * np.sqrt(k)
    if not deficient:                                                # same column space: Q Q^T Y = Y
        assert np.linalg.norm(Q @ (Q.T @ Y) - Y) <= 4 * k * EPS["f64"] * np.linalg.norm(Y) * np.linalg.cond(Y)


# ---------------------------------------------------------------------------------------------------------------------------------------
# geqp3 (qrcp.hip): the tag-exchange kernel with its scratch copy of the output, and the rendezvous kernel (wide input)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECS)
@pytest.mark.parametrize("m,n", [(1280, 64), (96, 2000)])
def test_geqp3_tag_and_rendezvous(ctx, p, m, n):
    import torch

    rng = np.random.default_rng(m + n)
    kmin = min(m, n)
    A = (rng.standard_normal((m, n)) * np.logspace(0, -3, n)[rng.permutation(n)]).astype(NP[p])
    Ad = _cm(A, p)
    J = torch.zeros(n, dtype=torch.int64, device="cuda")
    tau = torch.zeros(kmin, dtype=Ad.dtype, device="cuda")
    assert getattr(ctx.lib, f"rlhip_geqp3_{p}")(ctx.h, m, n, Ad.data_ptr(), m, J.data_ptr(), tau.data_ptr()) == 0
    _closed(ctx)
    jp = J.cpu().numpy()
    assert np.array_equal(np.sort(jp), np.arange(1, n + 1))
    # A P = Q R with Q orthonormal <=> R^T R = (A P)^T (A P); column pivoting leaves a diagonal that does not grow
    R = np.triu(_np(Ad)[:kmin])
    AP = A.astype(np.float64)[:, jp - 1]
    assert np.linalg.norm(R.T @ R - AP.T @ AP) <= 8 * kmin * EPS[p] * np.linalg.norm(AP) ** 2
    d = np.abs(np.diag(R))
    assert np.all(d[1:] <= d[:-1] + 100 * kmin * EPS[p] * d[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# after the battery (this module's tests run in file order on one context): the arena is empty, so it may be reserved
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_reserve_workspace_is_still_accepted(ctx):
    _closed(ctx)
    assert ctx.lib.rlhip_reserve_workspace(ctx.h, 1 << 20) == 0
