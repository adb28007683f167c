"""The Matern 3/2 and 5/2 kernels on the device: the rlhip_pdk_* entries of rpchol.hip / rbf.hip and the rlhip_drv_*_pdk_*
drivers over linops::RBFKernelMatrix / RBFCrossKernel with set_kernel, in fp64 and fp32 on every route, against the float64 model by
differences (tests/_pdk_model.py).

Two bounds, both measured on the CPU emulation of the norm-expansion route (tests/test_pdk_model.py), none tuned to the device:
  entry   |K_T - K_model| <= C_E eps_T (1 + L_kind (|z_i|^2 + |x_j|^2)), C_E = 16: the emulation stays at or below 2.1, the factor between
          is for the device's exp, sqrt and summation order;
  apply   |C_T - C_model| <= 64 eps_T (|alpha| |K| |B| + |beta| |C0|), the bound of tests/test_gpu_krr.py: the emulation stays at or below 9.5
          at the bandwidths used here.
An indexing, masking or formula error moves entries by O(1) times the scale of either bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import _pcg_model as pm
import _pdk_model as pk
import _rpchol_model as M

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
FACTOR = 64.0
C_E = 16.0
MATERN = [pk.MATERN32, pk.MATERN52]
SHAPES = [(1, 1, 1), (17, 63, 3), (65, 67, 17), (130, 130, 16)]
ROWS = [1, 4, 5, 20, 33, 128]


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


def _counts(ctx):
    return [ctx.rbf_path_count(w) for w in (55, 56, 57)]


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
def _case(kind, prec, rows_x, mz, nx, n):
    """the inputs and the model's result and magnitude for alpha = 1, beta = 0"""
    Z, X, B, l = _inputs(prec, rows_x, mz, nx, n)
    want, mag = pk.cross_apply(kind, Z, X, l, B)
    want.setflags(write=False)
    mag.setflags(write=False)
    return Z, X, B, l, want, mag


def _check(got, want, mag, T, what, factor=FACTOR):
    eps = float(np.finfo(T).eps)
    bound = factor * eps * mag
    err = np.abs(got - want)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f"{what}: max error / bound = {ratio:.3g} (in eps times the scale: {ratio * factor:.3g})")
    assert np.all(err <= bound), f"{what}: max error / bound = {ratio:.3g}"


def _check_entries(got, kind, Z, X, l, T, what):
    """the entry bound; a NaN fails it"""
    _check(got, pk.cross_kernel(kind, Z, X, l), pk.entry_scale(kind, Z, X, l), T, what, factor=C_E)


# ---------------------------------------------------------------------------------------------------
# 1. cross apply against the model, both precisions, both routes
# ---------------------------------------------------------------------------------------------------
def _run_cross_apply(ctx, kind, rows_x, shape, fused, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    mz, nx, n = shape
    Z, X, B, l, want, mag = _case(kind, prec, rows_x, mz, nx, n)
    padded = shape == (65, 67, 17)                          # leading dimensions larger than the sizes
    Zd = _pts(Z, T, rows_x + 3 if padded else None)
    Xd = _pts(X, T, rows_x + 2 if padded else None)
    Bd = _pts(B, T, nx + 5 if padded else None)
    Cd = torch.full((n, mz + 1 if padded else mz), float("nan"), dtype=Zd.dtype, device="cuda:0")
    before = _counts(ctx)
    with ctx.options(rbf_fused=fused):
        dev.pdk_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, kind, l, Bd, n, C_=Cd)
    assert [a - b for a, b in zip(_counts(ctx), before)] == ([1, 0, 0] if fused else [0, 1, 0])
    _check(_host(Cd, mz), want, mag, T, f"kind={kind} rows_x={rows_x} {shape} fused={fused} {prec}")
    if padded:
        assert bool(torch.isnan(Cd[:, mz:]).all())         # the rows of C past mz are not written


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("kind", MATERN)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rows_x", ROWS)
def test_cross_apply_matches_model(ctx, rows_x, shape, kind, fused, prec):
    _run_cross_apply(ctx, kind, rows_x, shape, fused, prec)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("kind", MATERN)
def test_cross_apply_four_column_tiles_and_many_x_tiles(ctx, kind, fused, prec):
    """n = 64 is the NT = 4 instantiation of the fused kernel; 1000 points of X are a walk over many staged tiles"""
    _run_cross_apply(ctx, kind, 16, (200, 1000, 64), fused, prec)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("kind", MATERN)
def test_alpha_beta(ctx, kind, fused, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (65, 67, 17)
    Z, X, B, l = _inputs(prec, rows_x, mz, nx, n)
    C0 = np.random.default_rng(9).standard_normal((mz, n)).astype(T).astype(np.float64)
    want, mag = pk.cross_apply(kind, Z, X, l, B, -0.5, 2.0, C0)
    with ctx.options(rbf_fused=fused):
        got = _host(dev.pdk_cross_apply(ctx, _pts(Z, T), _pts(X, T), rows_x, mz, nx, kind, l, _pts(B, T), n, alpha=-0.5, beta=2.0, C_=_pts(C0, T)), mz)
    _check(got, want, mag, T, f"kind={kind} alpha=-0.5 beta=2 fused={fused} {prec}")


# ---------------------------------------------------------------------------------------------------
# 2. entries: columns (by differences), the square and the cross submatrix (norm expansion)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
@pytest.mark.parametrize("rows_x", [1, 3, 64, 300])
def test_pdk_columns(ctx, rows_x, kind, prec):
    """the index list of test_gpu_rpchol.py::test_sqexp_columns: repeats, the first and the last point"""
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    rng = np.random.default_rng(rows_x)
    n = 1000 + 37
    X = rng.standard_normal((rows_x, n)).astype(T).astype(np.float64)
    Xd = _pts(X, T, rows_x + 5)
    idx = np.array([5, 1036, 5, 0, 700, 3, 999, 70] + list(rng.integers(0, n, 70)), dtype=np.int64)
    l = float(np.sqrt(rows_x)) * 0.7
    want = pk.cross_kernel(kind, X, X[:, idx], l)
    scale = pk.entry_scale(kind, X, X[:, idx], l)
    for reg in (0.0, 0.25):
        out = dev.pdk_columns(ctx, Xd, rows_x, n, torch.from_numpy(idx).cuda(), kind, l, reg)
        raw = out.cpu().numpy().T
        assert np.all(raw[idx, np.arange(idx.size)] == T(1) + T(reg))     # by differences: exactly 1 + reg
        got = raw.astype(np.float64)
        got[idx, np.arange(idx.size)] -= reg                                # exact: those entries are T(1) + T(0.25)
        _check(got, want, scale, T, f"columns kind={kind} rows_x={rows_x} reg={reg} {prec}", factor=C_E)


@functools.lru_cache(maxsize=None)
def _blocked_points(prec):
    """the points of test_gpu_rpchol.py::test_sqexp_submatrix_blocked_vs_entrywise: a repeated column, orthogonal columns"""
    T = DT[prec]
    rng = np.random.default_rng(3)
    rows_x, n = 7, 300
    Xh = rng.standard_normal((rows_x, n))
    Xh[:, 10] = Xh[:, 20]
    Xh[:, 30:37] = np.eye(rows_x) * 2.0
    Zh = rng.standard_normal((rows_x, 200))
    Zh[:, 40] = Xh[:, 20]                                                     # a point of Z that is a point of X
    Xh, Zh = Xh.astype(T).astype(np.float64), Zh.astype(T).astype(np.float64)
    Xh.setflags(write=False)
    Zh.setflags(write=False)
    return Xh, Zh


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
def test_pdk_submatrix(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    Xh, _ = _blocked_points(prec)
    rows_x, n = Xh.shape
    Xd = _pts(Xh, T)
    for l in (0.5, 1.0, 3.0):
        K = dev.pdk_submatrix(ctx, Xd, rows_x, n, 120, 90, 15, 7, kind, l).cpu().numpy().T.astype(np.float64)
        _check_entries(K, kind, Xh[:, 15:135], Xh[:, 7:97], l, T, f"submatrix kind={kind} l={l} {prec}")
        nr = dev.sq_colnorms(ctx, Xd, rows_x, n)
        K2 = dev.pdk_submatrix(ctx, Xd, rows_x, n, 120, 90, 15, 7, kind, l, sq_colnorms=nr).cpu().numpy().T
        assert np.array_equal(K, K2)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
def test_pdk_cross_submatrix(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    Xh, Zh = _blocked_points(prec)
    rows_x, nx = Xh.shape
    mz = Zh.shape[1]
    Xd, Zd = _pts(Xh, T, rows_x + 1), _pts(Zh, T)
    for l in (0.5, 3.0):
        before = _counts(ctx)
        K = dev.pdk_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 120, 90, 15, 7, kind, l).cpu().numpy().T
        assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 0, 1]
        _check_entries(K.astype(np.float64), kind, Zh[:, 15:135], Xh[:, 7:97], l, T, f"cross submatrix kind={kind} l={l} {prec}")
        # norms handed in: the same block
        nz, nxr = dev.sq_colnorms(ctx, Zd, rows_x, mz), dev.sq_colnorms(ctx, Xd, rows_x, nx)
        K2 = dev.pdk_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 120, 90, 15, 7, kind, l, sq_colnorms_z=nz, sq_colnorms_x=nxr).cpu().numpy().T
        assert np.array_equal(K, K2)


# ---------------------------------------------------------------------------------------------------
# 3. the clamp, and what it must not swallow
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
def test_clamp(ctx, kind, prec):
    """Z = X with duplicated points and large norms: the expanded s of coincident points is rounding noise of either sign.  Without the clamp
    sqrt of a negative s is NaN; with fmax a NaN coordinate would be swallowed (test_nan_propagates)."""
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, m = 5, 130
    X = 8.0 * np.random.default_rng(77).standard_normal((rows_x, m))
    src = np.arange(30) * 3
    X[:, 100:] = X[:, src]                                                    # 30 copies of earlier points
    X = X.astype(T).astype(np.float64)
    l = 0.7 * 8.0 * float(np.sqrt(rows_x))
    same = np.zeros((m, m), dtype=bool)
    same[np.arange(m), np.arange(m)] = True
    same[100 + np.arange(30), src] = True
    assert np.any(pk.expanded_s(X, X, T)[same] < 0), "the inputs do not exercise the clamp"
    want = pk.cross_kernel(kind, X, X, l)
    assert np.all(want[same] == 1.0)
    Xd = _pts(X, T)
    results = {"cross_submatrix": dev.pdk_cross_submatrix(ctx, Xd, Xd, rows_x, m, m, m, m, 0, 0, kind, l).cpu().numpy().T.astype(np.float64)}
    eye = np.eye(m)
    for fused in (1, 0):
        with ctx.options(rbf_fused=fused):
            blocks = [_host(dev.pdk_cross_apply(ctx, Xd, Xd, rows_x, m, m, kind, l, _pts(eye[:, c0:c0 + 64], T), min(64, m - c0)), m)
                      for c0 in range(0, m, 64)]
        results[f"apply fused={fused}"] = np.concatenate(blocks, axis=1)
    scale = pk.entry_scale(kind, X, X, l)
    eps = float(np.finfo(T).eps)
    for name, K in results.items():
        assert K.shape == (m, m) and not np.any(np.isnan(K)), name
        _check(K, want, scale, T, f"clamp {name} kind={kind} {prec}", factor=C_E)
        assert np.all(np.abs(K[same] - 1.0) <= C_E * eps * scale[same]), name


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
def test_nan_propagates(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, mz, nx, j = 5, 40, 50, 13
    Z, X, _, l = _inputs(prec, rows_x, mz, nx, 1)
    Xn = X.copy()
    Xn[2, j] = np.nan
    K = dev.pdk_cross_submatrix(ctx, _pts(Z, T), _pts(Xn, T), rows_x, mz, nx, mz, nx, 0, 0, kind, l).cpu().numpy().T
    assert np.all(np.isnan(K[:, j]))
    assert np.all(np.isfinite(np.delete(K, j, axis=1)))


# ---------------------------------------------------------------------------------------------------
# 4. the row-block apply of the square operator
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
@pytest.mark.parametrize("m,d", [(100, 3), (256, 4)])
def test_pdk_apply(ctx, m, d, kind, prec):
    """the inputs of test_gpu_rpchol.py::test_rbf_apply: K * I with and without a regularization, then num_ops = 3 with alpha and beta"""
    from randlapack_amd import device as dev

    T = DT[prec]
    rng = np.random.default_rng(m + d)
    Xh = rng.standard_normal((d, m)).astype(T).astype(np.float64)
    Xd = _pts(Xh, T)
    K = pk.cross_kernel(kind, Xh, Xh, 1.0)
    eye = np.eye(m)
    before = _counts(ctx)
    got = _host(dev.pdk_apply(ctx, Xd, d, m, kind, 1.0, _pts(eye, T), m), m)
    _check(got, K, K, T, f"K * I kind={kind} m={m} {prec}")                   # |K| |I| = K
    got = _host(dev.pdk_apply(ctx, Xd, d, m, kind, 1.0, _pts(eye, T), m, regs=(0.5,), eval_includes_reg=True), m)
    _check(got, K + 0.5 * eye, K + 0.5 * eye, T, f"(K + 0.5 I) * I kind={kind} m={m} {prec}")
    regs = (0.1, 1.0, 10.0)
    rg = np.array(regs, dtype=T).astype(np.float64)
    B = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    C0 = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    got = _host(dev.pdk_apply(ctx, Xd, d, m, kind, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True), m)
    want = -0.5 * (K @ B + B * rg) + 2.0 * C0
    mag = 0.5 * (np.abs(K) @ np.abs(B) + np.abs(B) * rg) + 2.0 * np.abs(C0)
    _check(got, want, mag, T, f"regs, alpha, beta kind={kind} m={m} {prec}")
    assert _counts(ctx) == before                                             # the square routine is none of the cross routes


# ---------------------------------------------------------------------------------------------------
# 5. the bit contract of the fused route
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
def test_fused_bit_contract(ctx, kind, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (200, 1000, 64)
    Z, X, B, l = _inputs(prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=1):
        before = _counts(ctx)
        a = dev.pdk_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, kind, l, Bd, n).cpu().numpy()
        b = dev.pdk_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, kind, l, Bd, n).cpu().numpy()
        assert np.array_equal(a, b)                                             # the same call twice
        part = dev.pdk_cross_apply(ctx, Zd[:17], Xd, rows_x, 17, nx, kind, l, Bd, n).cpu().numpy()
        assert np.array_equal(part, a[:, :17])                                  # a row does not depend on mz
        part = dev.pdk_cross_apply(ctx, Zd[5:75], Xd, rows_x, 70, nx, kind, l, Bd, n).cpu().numpy()
        assert np.array_equal(part, a[:, 5:75])                                 # nor on its place in Z
        assert [x - y for x, y in zip(_counts(ctx), before)] == [4, 0, 0]
    other = dev.Context(0)                                                      # nor on the context
    try:
        other.set_option("rbf_fused", 1)
        c = dev.pdk_cross_apply(other, Zd, Xd, rows_x, mz, nx, kind, l, Bd, n).cpu().numpy()
    finally:
        other.close()
    assert np.array_equal(a, c)


# ---------------------------------------------------------------------------------------------------
# 6. argument codes; kind 0 through the new entries is the existing entry, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_unknown_kernel_is_refused(ctx, prec):
    import torch

    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    rows_x, mz, nx, n = 3, 5, 6, 2
    Z = torch.ones((mz, rows_x), dtype=dt, device="cuda:0")
    X = torch.ones((nx, rows_x), dtype=dt, device="cuda:0")
    B = torch.ones((n, nx), dtype=dt, device="cuda:0")
    Cm = torch.full((nx, nx), 7.0, dtype=dt, device="cuda:0")
    idx = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    regs = (ct * 1)(0.0)
    lib, h = ctx.lib, ctx.h
    one, zero = ct(1.0), ct(0.0)
    before = _counts(ctx)
    for kernel in (3, -1):
        # the code is the position of `kernel` in each argument list
        assert getattr(lib, f"rlhip_pdk_columns_{prec}")(h, rows_x, nx, X.data_ptr(), rows_x, 2, idx.data_ptr(), kernel, one, zero, Cm.data_ptr(), nx) == -8
        assert getattr(lib, f"rlhip_pdk_submatrix_{prec}")(h, rows_x, nx, X.data_ptr(), rows_x, None, nx, nx, Cm.data_ptr(), nx, 0, 0, kernel, one) == -13
        assert getattr(lib, f"rlhip_pdk_apply_{prec}")(h, rows_x, nx, X.data_ptr(), rows_x, kernel, one, regs, 1, 0, n, one, B.data_ptr(), nx, zero,
                                                        Cm.data_ptr(), nx) == -6
        assert getattr(lib, f"rlhip_pdk_cross_submatrix_{prec}")(h, rows_x, mz, Z.data_ptr(), rows_x, None, nx, X.data_ptr(), rows_x, None, mz, nx,
                                                                  Cm.data_ptr(), mz, 0, 0, kernel, one) == -17
        assert getattr(lib, f"rlhip_pdk_cross_apply_{prec}")(h, rows_x, mz, Z.data_ptr(), rows_x, nx, X.data_ptr(), rows_x, kernel, one, n, one,
                                                              B.data_ptr(), nx, zero, Cm.data_ptr(), mz) == -9
    # the arguments behind `kernel` moved by one: the bandwidth of the cross apply is now the tenth
    assert getattr(lib, f"rlhip_pdk_cross_apply_{prec}")(h, rows_x, mz, Z.data_ptr(), rows_x, nx, X.data_ptr(), rows_x, 1, zero, n, one, B.data_ptr(), nx,
                                                          zero, Cm.data_ptr(), mz) == -10
    assert getattr(lib, f"rlhip_pdk_cross_apply_{prec}")(h, rows_x, mz, Z.data_ptr(), rows_x, nx, X.data_ptr(), rows_x, 1, one, n, one, B.data_ptr(), nx,
                                                          zero, Cm.data_ptr(), mz - 1) == -17
    assert getattr(lib, f"rlhip_pdk_cross_submatrix_{prec}")(h, rows_x, mz, Z.data_ptr(), rows_x, None, nx, X.data_ptr(), rows_x, None, mz, nx,
                                                              Cm.data_ptr(), mz, 0, 0, 2, zero) == -18
    torch.cuda.synchronize()
    assert _counts(ctx) == before and bool((Cm == 7.0).all())                 # nothing was launched


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_unknown_kernel_is_refused_by_the_drivers(ctx, prec):
    """the four driver entries: the code is the position of `kernel` there too, and nothing runs"""
    import torch

    ct = C.c_double if prec == "f64" else C.c_float
    dt = torch.float64 if prec == "f64" else torch.float32
    n, rows_x = 8, 2
    X = torch.ones((n, rows_x), dtype=dt, device="cuda:0")
    W = torch.full((n, n), 7.0, dtype=dt, device="cuda:0")
    lib, h = ctx.lib, ctx.h
    one = ct(1.0)
    regs = (ct * 1)(0.5)
    k, it = C.c_int64(4), C.c_int64(0)
    S = (C.c_int64 * 8)()
    st = (C.c_uint32 * 6)()
    status = (C.c_int * 2)()
    hist = (ct * 8)()
    for kernel in (3, -1):
        assert getattr(lib, f"rlhip_drv_rpchol_pdk_{prec}")(h, X.data_ptr(), rows_x, rows_x, n, kernel, one, ct(0.0), C.byref(k), 2, S, W.data_ptr(), n, st,
                                                             status) == -6
        assert getattr(lib, f"rlhip_drv_krill_full_rpchol_pdk_{prec}")(h, X.data_ptr(), rows_x, rows_x, n, kernel, one, regs, 1, W.data_ptr(), W.data_ptr(),
                                                                        1, one, 3, C.byref(k), 2, st, C.byref(it), hist) == -6
        assert getattr(lib, f"rlhip_drv_krr_predict_pdk_{prec}")(h, rows_x, n, X.data_ptr(), rows_x, n, X.data_ptr(), rows_x, kernel, one, 1, W.data_ptr(), n,
                                                                  W.data_ptr(), n) == -9
        assert getattr(lib, f"rlhip_drv_pdk_kernel_apply_{prec}")(h, X.data_ptr(), rows_x, rows_x, n, kernel, one, regs, 1, 0, 0, 1, one, W.data_ptr(), n,
                                                                   ct(0.0), W.data_ptr(), n) == -6
    torch.cuda.synchronize()
    assert bool((W == 7.0).all())


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kind_zero_is_the_existing_entry_bit_for_bit(ctx, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (65, 67, 17)
    Z, X, B, l = _inputs(prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    eq = lambda a, b: np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    idx = torch.tensor([5, 66, 5, 0], dtype=torch.int64, device="cuda:0")
    assert eq(dev.pdk_columns(ctx, Xd, rows_x, nx, idx, 0, l, 0.25), dev.sqexp_columns(ctx, Xd, rows_x, nx, idx, l, 0.25))
    assert eq(dev.pdk_submatrix(ctx, Xd, rows_x, nx, 40, 30, 3, 7, 0, l), dev.sqexp_submatrix(ctx, Xd, rows_x, nx, 40, 30, 3, 7, l))
    assert eq(dev.pdk_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 40, 30, 3, 7, 0, l), dev.sqexp_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 40, 30, 3, 7, l))
    Bsq = _pts(np.asarray(B[:, :3]), T)
    assert eq(dev.pdk_apply(ctx, Xd, rows_x, nx, 0, l, Bsq, 3, alpha=-0.5, regs=(0.1, 1.0, 10.0), eval_includes_reg=True),
              dev.rbf_apply(ctx, Xd, rows_x, nx, l, Bsq, 3, alpha=-0.5, regs=(0.1, 1.0, 10.0), eval_includes_reg=True))
    for fused in (1, 0):
        with ctx.options(rbf_fused=fused):
            before = _counts(ctx)
            a = dev.pdk_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, 0, l, Bd, n)
            b = dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, l, Bd, n)
            assert eq(a, b)
            assert [x - y for x, y in zip(_counts(ctx), before)] == ([2, 0, 0] if fused else [0, 2, 0])
    for mf in (False, True):
        assert eq(dev.pdk_kernel_apply(ctx, Xd, rows_x, nx, 0, l, Bsq, 3, regs=(0.5,), eval_includes_reg=True, matrix_free=mf),
                  dev.rbf_kernel_apply(ctx, Xd, rows_x, nx, l, Bsq, 3, regs=(0.5,), eval_includes_reg=True, matrix_free=mf))


# ---------------------------------------------------------------------------------------------------
# 7. RBFKernelMatrix with set_kernel, through the object
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("matrix_free", [True, False])
@pytest.mark.parametrize("kind", MATERN)
def test_kernel_matrix_through_the_object(ctx, kind, matrix_free, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    m, d = 333, 7
    rng = np.random.default_rng(m + d)
    Xh = rng.standard_normal((d, m)).astype(T).astype(np.float64)
    regs = (0.1, 1.0, 10.0)
    rg = np.array(regs, dtype=T).astype(np.float64)
    B = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    C0 = rng.standard_normal((m, 3)).astype(T).astype(np.float64)
    l = 0.7 * float(np.sqrt(d))
    K = pk.cross_kernel(kind, Xh, Xh, l)
    want = -0.5 * (K @ B + B * rg) + 2.0 * C0
    mag = 0.5 * (np.abs(K) @ np.abs(B) + np.abs(B) * rg) + 2.0 * np.abs(C0)
    before = _counts(ctx)
    got = dev.pdk_kernel_apply(ctx, _pts(Xh, T), d, m, kind, l, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True,
                               matrix_free=matrix_free)
    assert [a - b for a, b in zip(_counts(ctx), before)] == ([1, 0, 0] if matrix_free else [0, 0, 0])
    _check(_host(got, m), want, mag, T, f"object kind={kind} matrix_free={matrix_free} {prec}")


# ---------------------------------------------------------------------------------------------------
# 8. randomly pivoted Cholesky of a Matern kernel matrix
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", MATERN)
@pytest.mark.parametrize("n,rows_x,l,k,b", [(2000, 3, 0.5, 200, 16), (2500, 4, 8.0, 100, 256)])
def test_rpchol_driver(ctx, n, rows_x, l, k, b, kind, prec):
    """test_gpu_rpchol.py::test_rbf_driver with Matern columns: the model replays the device's pivots in float64.  Its float32 run differs
    from its float64 run by 1.0e-5 to 1.8e-5 (b = 256) and 1.4e-6 (b = 16) relative on F, inside the 1e-4 asked of the device."""
    from randlapack_amd import device as dev

    T = DT[prec]
    rng = np.random.default_rng(n + rows_x)
    Xh = rng.standard_normal((rows_x, n)).astype(T).astype(np.float64)
    reg = 1e-3
    r = dev.drv_rpchol_pdk(ctx, _pts(Xh, T), rows_x, n, kind, l, k, b, reg=reg, key=(5, 1))
    kk = r["k"]
    assert kk > 0 and len(set(r["S"].tolist())) == kk
    F = r["F"].cpu().numpy().T[:, :kk].astype(np.float64)
    blocks = [r["S"][p:p + b] for p in range(0, kk, b)]
    cols = lambda idx: pk.cross_kernel(kind, Xh, Xh[:, idx], l) + reg * (np.arange(n)[:, None] == np.asarray(idx)[None, :])
    m = M.rp_cholesky(n, np.full(n, 1.0 + reg), cols, kk, b, forced_S=blocks)
    assert m["k"] == kk
    tol = 1e-12 if T is np.float64 else 1e-4
    err = np.max(np.abs(F - m["F"])) / max(1.0, np.abs(m["F"]).max())
    print(f"rpchol kind={kind} n={n} b={b} {prec}: max |F - model| = {err:.3g} (allowed {tol:g})")
    assert err <= tol
    # trace(K - F F^T) = sum of the final d; F is a pivoted Cholesky factor in the order S: row S[i] is zero after column i
    tr = n * (1.0 + reg) - np.sum(F * F)
    assert abs(tr - m["d"].sum()) <= (1e-9 if T is np.float64 else 1e-2) * n
    later = np.triu(np.ones((kk, kk), dtype=bool), 1)
    assert np.max(np.abs(F[r["S"], :][later]), initial=0.0) <= (1e-10 if T is np.float64 else 1e-3)


# ---------------------------------------------------------------------------------------------------
# 9. fit, then predict
# ---------------------------------------------------------------------------------------------------
# Iterations that the float64 CPU PCG (tests/_pcg_model.py) needs on the same operator, right-hand sides and tolerance (100 eps_T) with the exact
# rank-128 spectral preconditioner -- the device gets max_iters = twice that:
#   Matern 3/2   lockstep: 23 (tol of fp64), 7 (tol of fp32) -> 46, 14     block: 25, 10 -> 50, 20
#   Matern 5/2   lockstep: 17, 5 -> 34, 10                                 block: 19, 7 -> 38, 14
CPU_ITERS = {(pk.MATERN32, "lockstep", "f64"): 23, (pk.MATERN32, "lockstep", "f32"): 7, (pk.MATERN32, "block", "f64"): 25, (pk.MATERN32, "block", "f32"): 10,
             (pk.MATERN52, "lockstep", "f64"): 17, (pk.MATERN52, "lockstep", "f32"): 5, (pk.MATERN52, "block", "f64"): 19, (pk.MATERN52, "block", "f32"): 7}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", [("lockstep", 3), ("block", 4)])
@pytest.mark.parametrize("kind", MATERN)
def test_fit_then_predict(ctx, kind, mode, s, prec):
    """test_gpu_krr.py::test_fit_then_predict with a Matern kernel.  Matern spectra decay more slowly than the squared exponential's (lambda_129
    of these points is about 0.25 / 0.13 against 0.009), so the regularizations start at 1e-1, not 1e-2."""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, l, k, blk = 1000, 5, 3.0, 128, 16
    pts = np.random.default_rng(2).standard_normal((rows_x, n)).astype(T).astype(np.float64)
    mus = (1e-1, 1.0, 10.0) if mode == "lockstep" else (1e-1,)
    G = pm.reg_op(pk.cross_kernel(kind, pts, pts, l), mus, np.float64)
    Xstar = np.random.default_rng(101).standard_normal((n, s)).astype(T)
    H = G(Xstar)
    tol = 100 * float(np.finfo(T).eps)
    Pd = _pts(pts, T)
    max_iters = 2 * CPU_ITERS[(kind, mode, prec)]
    r = dev.krill_full_rpchol_pdk(ctx, Pd, rows_x, n, kind, l, list(mus), _pts(H, T), _pts(np.zeros_like(H), T), s, tol, max_iters, k=k, b=blk, key=(7, 0))
    print(f"fit kind={kind} {mode} {prec}: {r['iters']} iterations of at most {max_iters}, rank {r['k']}")
    assert r["k"] == k and 1 <= r["iters"] <= max_iters
    Xdev = _host(r["X"], n)
    mz = 130
    Zh = np.random.default_rng(303).standard_normal((rows_x, mz)).astype(T).astype(np.float64)
    before = _counts(ctx)
    Y = _host(dev.krr_predict_pdk(ctx, _pts(Zh, T), mz, Pd, rows_x, n, kind, l, r["X"], s), mz)
    assert [a - b for a, b in zip(_counts(ctx), before)] == [1, 0, 0]
    K = pk.cross_kernel(kind, Zh, pts, l)
    mag = np.abs(K) @ np.abs(Xdev)
    _check(Y, K @ Xdev, mag, T, f"predict on the device's coefficients kind={kind} {mode} {prec}")
    eps = float(np.finfo(T).eps)
    slack = np.sum(np.abs(K), axis=1, keepdims=True) * float(np.max(np.abs(Xdev - Xstar.astype(np.float64))))
    err = np.abs(Y - K @ Xstar.astype(np.float64))
    print(f"predict against the planted coefficients kind={kind} {mode} {prec}: max error / allowed = "
          f"{float(np.max(err / (slack + FACTOR * eps * mag))):.3g}")
    assert np.all(err <= slack + FACTOR * eps * mag)
