"""The fused cross apply split over X (randlapack_amd/csrc/rbf.hip under RLHIP_OPT_RBF_FUSED = 2), in fp64 and fp32, for the
squared exponential and Matern 5/2, against the float64 models by differences (tests/_krr_model.py, tests/_pdk_model.py).

The bound is the project's componentwise bound of the apply, 64 eps_T (|alpha| |K| |B| + |beta| |C0|) (tests/test_gpu_krr.py,
tests/test_gpu_pdk.py).  It covers the split: every chunk's sum is shorter than the unsplit sum, and the g - 1 additions of the partials
add at most (g - 1) eps_T of the same magnitude, g <= 8 on the shapes here.

The shapes are the smallest at which the split can go wrong: nx >= 1024 (below it nothing is split), nx = 1100 and 4113 put the end of X
inside the last staged tile of the last chunk, 4113 gives 8 chunks, mz = 70, 130 and 200 are more than one tile of Z with a ragged last
one, n = 1, 3, 16, 17, 64 reach the three column-tile instantiations, rows_x = 1 ... 128 the six row instantiations."""
import functools

import numpy as np
import pytest

import _krr_model as km
import _pcg_model as pm
import _pdk_model as pk

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
FACTOR = 64.0
KINDS = [pk.SQEXP, pk.MATERN52]
SHAPES = [(1, 1024, 1), (70, 1100, 3), (17, 4113, 17), (200, 2500, 64), (130, 1300, 16)]
ROWS = [1, 5, 16, 20, 33, 128]


def _pts(a, T, ld=None):
    """points / matrix (rows x cols, numpy) -> column-major device tensor (cols, ld) whose first `rows` entries of every column are the data"""
    import torch

    rows, cols = a.shape
    ld = ld or rows
    buf = np.zeros((cols, ld), dtype=T)
    buf[:, :rows] = np.asarray(a, dtype=T).T
    return torch.from_numpy(buf).to("cuda:0")


def _host(t, rows):
    """column-major device tensor (cols, ld) -> numpy rows x cols, float64"""
    return t.detach().cpu().numpy()[:, :rows].T.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _inputs(prec, rows_x, mz, nx, n):
    """inputs rounded to T (as float64); computed once, never modified"""
    T = DT[prec]
    rng = np.random.default_rng(1000 * rows_x + mz + nx + n)
    r = lambda *s: rng.standard_normal(s).astype(T).astype(np.float64)
    Z, X, B = r(rows_x, mz), r(rows_x, nx), r(nx, n)
    for a in (Z, X, B):
        a.setflags(write=False)
    return Z, X, B, 0.7 * float(np.sqrt(rows_x))


@functools.lru_cache(maxsize=None)
def _kernel(kind, prec, rows_x, mz, nx, n):
    """the model's K(Z, X) for the inputs above, float64, read-only"""
    Z, X, _, h = _inputs(prec, rows_x, mz, nx, n)
    K = km.cross_kernel(Z, X, h) if kind == pk.SQEXP else pk.cross_kernel(kind, Z, X, h)
    K.setflags(write=False)
    return K


def _model(kind, prec, rows_x, mz, nx, n, alpha=1.0, beta=0.0, C0=None):
    """(alpha K B + beta C0, |alpha| |K| |B| + |beta| |C0|) from the cached kernel"""
    B = _inputs(prec, rows_x, mz, nx, n)[2]
    K = _kernel(kind, prec, rows_x, mz, nx, n)
    out, mag = alpha * (K @ B), abs(alpha) * (np.abs(K) @ np.abs(B))
    if beta != 0.0:
        out, mag = out + beta * C0, mag + abs(beta) * np.abs(C0)
    return out, mag


def _apply(ctx, kind, *args, **kw):
    """Z, X, rows_x, mz, nx, h, B, n [, alpha, beta, C_]: the squared exponential through its own entry, Matern through rlhip_pdk_*"""
    from randlapack_amd import device as dev

    if kind == pk.SQEXP:
        return dev.rbf_cross_apply(ctx, *args, **kw)
    Z, X, rows_x, mz, nx, h, B, n = args
    return dev.pdk_cross_apply(ctx, Z, X, rows_x, mz, nx, kind, h, B, n, **kw)


def _counts(ctx):
    """fused, composed, cross-submatrix calls, split applies"""
    return [ctx.rbf_path_count(w) for w in (55, 56, 57)] + [ctx.rbf_split_count()]


def _moved(ctx, before):
    return [a - b for a, b in zip(_counts(ctx), before)]


def _check(got, want, mag, T, what, factor=FACTOR):
    eps = float(np.finfo(T).eps)
    bound = factor * eps * mag
    err = np.abs(got - want)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f"{what}: max error / bound = {ratio:.3g} (in eps |K||B|: {ratio * factor:.3g})")
    assert np.all(err <= bound), f"{what}: max error / bound = {ratio:.3g}"


# ---------------------------------------------------------------------------------------------------
# 1. the split apply against the model
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rows_x", ROWS)
def test_split_apply_matches_model(ctx, rows_x, shape, kind, prec):
    import torch
    from randlapack_amd import device as dev

    T = DT[prec]
    mz, nx, n = shape
    assert dev.rbf_split_chunks(mz, nx) >= 2
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    want, mag = _model(kind, prec, rows_x, mz, nx, n)
    padded = shape == (70, 1100, 3)                         # leading dimensions larger than the sizes
    Zd = _pts(Z, T, rows_x + 3 if padded else None)
    Xd = _pts(X, T, rows_x + 2 if padded else None)
    Bd = _pts(B, T, nx + 5 if padded else None)
    Cd = torch.full((n, mz + 1 if padded else mz), float("nan"), dtype=Zd.dtype, device="cuda:0")      # beta = 0 on NaN: C is not read
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        _apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n, C_=Cd)
    assert _moved(ctx, before) == [1, 0, 0, 1]             # one fused apply, and it ran split
    _check(_host(Cd, mz), want, mag, T, f"kind={kind} rows_x={rows_x} {shape} split {prec}")
    if padded:
        assert bool(torch.isnan(Cd[:, mz:]).all())         # the rows of C past mz are not written


# ---------------------------------------------------------------------------------------------------
# 2. alpha / beta, and what lies behind the last point, row and row of B is never read
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_alpha_beta(ctx, kind, prec):
    import torch

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (70, 1100, 3)
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    C0 = np.random.default_rng(9).standard_normal((mz, n)).astype(T).astype(np.float64)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=2):
        for alpha, beta in [(-0.5, 2.0), (1.0, 1.0), (3.0, -1.0), (1.5, 0.0)]:
            before = _counts(ctx)
            Cd = _pts(C0, T) if beta != 0.0 else torch.full((n, mz), float("nan"), dtype=Zd.dtype, device="cuda:0")
            got = _host(_apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n, alpha=alpha, beta=beta, C_=Cd), mz)
            assert _moved(ctx, before) == [1, 0, 0, 1]
            assert not np.any(np.isnan(got))                                    # beta == 0: the NaNs of C are not read
            want, mag = _model(kind, prec, rows_x, mz, nx, n, alpha, beta, C0)
            _check(got, want, mag, T, f"kind={kind} alpha={alpha} beta={beta} split {prec}")
        # alpha = 0 and nx = 0 leave before any route: C = beta C exactly, no counter moves
        before = _counts(ctx)
        got = _host(_apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n, alpha=0.0, beta=2.0, C_=_pts(C0, T)), mz)
        assert np.array_equal(got, 2.0 * C0) and _moved(ctx, before) == [0, 0, 0, 0]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(70, 1100, 3), (17, 4113, 17)], ids=lambda s: "x".join(map(str, s)))
def test_padding_is_masked(ctx, shape, kind, prec):
    """nx = 1100 and 4113: the last chunk ends inside a staged tile, whatever the tile length of the instantiation"""
    import torch

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, shape
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    Zd = _pts(Z, T)
    with ctx.options(rbf_fused=2):
        tight = _apply(ctx, kind, Zd, _pts(X, T), rows_x, mz, nx, h, _pts(B, T), n).cpu().numpy()
        # X with 61 more "points" and 3 more rows per point, B with 61 more rows and one more column: all 1e30
        Xb = torch.full((nx + 61, rows_x + 3), 1e30, dtype=Zd.dtype, device="cuda:0")
        Xb[:nx, :rows_x] = _pts(X, T)
        Bb = torch.full((n + 1, nx + 61), 1e30, dtype=Zd.dtype, device="cuda:0")
        Bb[:n, :nx] = _pts(B, T)
        before = _counts(ctx)
        loose = _apply(ctx, kind, Zd, Xb, rows_x, mz, nx, h, Bb, n).cpu().numpy()
        assert _moved(ctx, before) == [1, 0, 0, 1]
    assert np.array_equal(tight, loose)


# ---------------------------------------------------------------------------------------------------
# 3. nothing changes under value 1, under the default, or where g = 1
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_default_and_value_1_never_split(ctx, prec):
    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (70, 1100, 3)
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    want, mag = _model(pk.SQEXP, prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    before = _counts(ctx)
    assert ctx.get_option("rbf_fused") == -1
    by_default = _host(_apply(ctx, pk.SQEXP, Zd, Xd, rows_x, mz, nx, h, Bd, n), mz)
    assert _moved(ctx, before) == [1, 0, 0, 0]
    with ctx.options(rbf_fused=1):
        one = _host(_apply(ctx, pk.SQEXP, Zd, Xd, rows_x, mz, nx, h, Bd, n), mz)
    assert _moved(ctx, before) == [2, 0, 0, 0]
    assert np.array_equal(by_default, one)
    _check(one, want, mag, T, f"value 1 on a shape that value 2 splits {prec}")
    with ctx.options(rbf_fused=0):
        _apply(ctx, pk.SQEXP, Zd, Xd, rows_x, mz, nx, h, Bd, n)
    assert _moved(ctx, before) == [2, 1, 0, 0]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_chunk_gives_the_bits_of_value_1(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, (mz, nx, n) = 16, (200, 1000, 64)
    assert dev.rbf_split_chunks(mz, nx) == 1
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    before = _counts(ctx)
    with ctx.options(rbf_fused=1):
        one = _apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
    with ctx.options(rbf_fused=2):
        two = _apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
    assert np.array_equal(one, two) and _moved(ctx, before) == [2, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------
# 4. the bit contract of value 2
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows_x", [5, 16])
def test_split_bit_contract(ctx, rows_x, kind, prec):
    import torch

    T = DT[prec]
    mz, nx, n = 200, 2500, 64
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    _, mag = _model(kind, prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=2):
        before = _counts(ctx)
        a = _apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
        b = _apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(a, b)                                             # the same call twice
        # two selections of 70 of the 200 points, both run with mz = 70 (the same g): the points 30 .. 74 of Z are at the places 25 .. 69
        # of the first and 0 .. 44 of the second, in other lanes, waves and Z tiles
        first = _apply(ctx, kind, Zd[5:75].contiguous(), Xd, rows_x, 70, nx, h, Bd, n).cpu().numpy()
        second = _apply(ctx, kind, Zd[30:100].contiguous(), Xd, rows_x, 70, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(first[:, 25:70], second[:, 0:45])                 # a row does not depend on its place in Z
        rev = _apply(ctx, kind, torch.flip(Zd[5:75], dims=[0]).contiguous(), Xd, rows_x, 70, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(rev[:, ::-1], first)
        assert _moved(ctx, before) == [5, 0, 0, 5]
    with ctx.options(rbf_fused=1):
        one = _host(_apply(ctx, kind, Zd, Xd, rows_x, mz, nx, h, Bd, n), mz)
    _check(a.T.astype(np.float64), one, mag, T, f"kind={kind} rows_x={rows_x} value 2 against value 1 {prec}", factor=2 * FACTOR)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_partials_are_added_in_chunk_order(ctx, kind, prec):
    """Every point is the number 1 (rows_x = 1): |z|^2 + |x|^2 - 2 z x = 0 exactly, so K = 1 exactly and a chunk's partial is the sum of its
    part of B.  Three chunks of 512 points, B = 1 in the first and eps / 2 in the second and in the third, zero elsewhere: the three partials
    are exact.  In chunk order (1 + eps / 2) + eps / 2 = 1, a tie rounded to even twice; in any order that adds the two small ones first,
    1 + eps.  The 64 eps bound cannot see the difference; this can."""
    from randlapack_amd import device as dev

    T = DT[prec]
    eps = float(np.finfo(T).eps)
    mz, nx = 3, 1536
    assert dev.rbf_split_chunks(mz, nx) == 3
    B = np.zeros((nx, 2))
    B[0, 0], B[512, 0], B[1024, 0] = 1.0, eps / 2, eps / 2
    B[511, 1], B[1023, 1], B[1535, 1] = eps / 2, eps / 2, 1.0           # the mirror image: eps / 2 + eps / 2 = eps first, then 1 + eps
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        got = _host(_apply(ctx, kind, _pts(np.ones((1, mz)), T), _pts(np.ones((1, nx)), T), 1, mz, nx, 0.7, _pts(B, T), 2), mz)
    assert _moved(ctx, before) == [1, 0, 0, 1]
    assert np.array_equal(got, np.tile([1.0, 1.0 + eps], (mz, 1))), got


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_chunks_do_not_depend_on_n(ctx, prec):
    """g is a function of (mz, nx) alone, and a column of the result depends on its own column of B alone: the first three of 64 columns
    are the three columns of the same product with n = 3, bit for bit (other instantiations of the kernel, the same chunks: 8 here)"""
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, mz, nx, n = 5, 200, 4096, 64
    assert dev.rbf_split_chunks(mz, nx) == 8
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    Zd, Xd = _pts(Z, T), _pts(X, T)
    with ctx.options(rbf_fused=2):
        before = _counts(ctx)
        wide = _apply(ctx, pk.SQEXP, Zd, Xd, rows_x, mz, nx, h, _pts(B, T), n).cpu().numpy()
        narrow = _apply(ctx, pk.SQEXP, Zd, Xd, rows_x, mz, nx, h, _pts(B[:, :3], T), 3).cpu().numpy()
        assert _moved(ctx, before) == [2, 0, 0, 2]
    assert np.array_equal(wide[:3], narrow)


# ---------------------------------------------------------------------------------------------------
# 5. outside the fused kernel's limits value 2 is the composed route
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("rows_x,n", [(129, 16), (8, 65)])
def test_outside_the_fused_limits_takes_the_composed_route(ctx, rows_x, n, prec):
    T = DT[prec]
    mz, nx = 70, 1100
    Z, X, B, h = _inputs(prec, rows_x, mz, nx, n)
    want, mag = _model(pk.SQEXP, prec, rows_x, mz, nx, n)
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        Cd = _apply(ctx, pk.SQEXP, _pts(Z, T), _pts(X, T), rows_x, mz, nx, h, _pts(B, T), n)
    assert _moved(ctx, before) == [0, 1, 0, 0]
    _check(_host(Cd, mz), want, mag, T, f"rows_x={rows_x} n={n} value 2 {prec}")


# ---------------------------------------------------------------------------------------------------
# 6. above the C ABI: krr_predict and the matrix-free RBFKernelMatrix under value 2
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", [("lockstep", 3), ("block", 4)])
def test_fit_then_predict_split(ctx, mode, s, prec):
    """the problem of test_gpu_krr.py::test_fit_then_predict with 1100 training points, so that the prediction at 130 points is split"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, h, k, blk = 1100, 5, 3.0, 128, 16
    pts = np.random.default_rng(2).standard_normal((rows_x, n)).astype(T).astype(np.float64)
    mus = (1e-2, 1e-1, 1.0) if mode == "lockstep" else (1e-2,)
    G = pm.reg_op(pm.rbf_kernel(pts, h, np.float64), mus, np.float64)
    Xstar = np.random.default_rng(101).standard_normal((n, s)).astype(T)
    H = G(Xstar)
    tol = 100 * float(np.finfo(T).eps)
    Pd = _pts(pts, T)
    r = dev.krill_full_rpchol_rbf(ctx, Pd, rows_x, n, h, list(mus), _pts(H, T), _pts(np.zeros_like(H), T), s, tol, 40, k=k, b=blk, key=(7, 0))
    Xdev = _host(r["X"], n)
    mz = 130
    assert dev.rbf_split_chunks(mz, n) == 2
    Zh = np.random.default_rng(303).standard_normal((rows_x, mz)).astype(T).astype(np.float64)
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        Y = _host(dev.krr_predict(ctx, _pts(Zh, T), mz, Pd, rows_x, n, h, r["X"], s), mz)
    assert _moved(ctx, before) == [1, 0, 0, 1]
    K = km.cross_kernel(Zh, pts, h)
    mag = np.abs(K) @ np.abs(Xdev)
    _check(Y, K @ Xdev, mag, T, f"split predict on the device's coefficients {mode} {prec}")
    eps = float(np.finfo(T).eps)
    slack = np.sum(np.abs(K), axis=1, keepdims=True) * float(np.max(np.abs(Xdev - Xstar.astype(np.float64))))
    err = np.abs(Y - K @ Xstar.astype(np.float64))
    print(f"split predict against the planted coefficients {mode} {prec}: max error / allowed = {float(np.max(err / (slack + FACTOR * eps * mag))):.3g}")
    assert np.all(err <= slack + FACTOR * eps * mag)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rbf_kernel_matrix_matrix_free_split(ctx, prec):
    """test_gpu_krr.py::test_rbf_kernel_matrix_matrix_free with dim = 1100: Z = X, 18 tiles of Z times 2 chunks"""
    from randlapack_amd import device as dev

    T = DT[prec]
    m, d = 1100, 7
    assert dev.rbf_split_chunks(m, m) == 2
    rng = np.random.default_rng(m + d)
    Xh = rng.standard_normal((d, m)).astype(T).astype(np.float64)
    Xd = _pts(Xh, T)
    regs = (0.1, 1.0, 10.0)
    B = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    C0 = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    K = km.cross_kernel(Xh, Xh, 1.0)
    rg = np.array(regs, dtype=T).astype(np.float64)
    want = -0.5 * (K @ B + B * rg) + 2.0 * C0
    mag = 0.5 * (np.abs(K) @ np.abs(B) + np.abs(B) * rg) + 2.0 * np.abs(C0)
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        got = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True,
                                   matrix_free=True)
    assert _moved(ctx, before) == [1, 0, 0, 1]
    _check(_host(got, m), want, mag, T, f"matrix-free split with regs {prec}")
    # not matrix-free: rlhip_rbf_apply_*'s route, which value 2 does not touch
    before = _counts(ctx)
    with ctx.options(rbf_fused=2):
        a = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True)
    b = dev.rbf_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and _moved(ctx, before) == [0, 0, 0, 0]
