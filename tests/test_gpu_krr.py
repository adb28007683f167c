"""The RBF kernel between two point sets on the device (randlapack_amd/csrc/rbf.hip: rlhip_rbf_cross_apply_*, rlhip_sqexp_cross_submatrix_*),
linops::RBFCrossKernel / krr_predict / RBFKernelMatrix::set_matrix_free through their C entries, in fp64 and fp32 on both routes, against the
float64 model by differences (tests/_krr_model.py).

The componentwise bound of the apply is 64 eps_T (|alpha| |K| |B| + |beta| |C0|): a numpy emulation of the norm-expansion route in T stays
within 7 eps_T (fp32) / 3 eps_T (fp64) of the model on these shapes and seeds, 64 leaves about a tenfold margin for the device's summation
order and exp; an indexing or masking error moves entries by O(1) times the bound's scale."""
import ctypes as C
import functools

import numpy as np
import pytest

import _krr_model as km
import _pcg_model as pm
import _rpchol_model as M

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}
FACTOR = 64.0
SHAPES = [(1, 1, 1), (17, 63, 3), (65, 67, 17), (200, 1000, 64), (130, 130, 16)]
ROWS = [1, 3, 4, 5, 16, 20, 33, 128]


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
def _case(prec, rows_x, mz, nx, n):
    """inputs rounded to T (as float64) and the model's result and magnitude for alpha = 1, beta = 0; computed once, never modified"""
    T = DT[prec]
    rng = np.random.default_rng(1000 * rows_x + mz + nx + n)
    r = lambda *s: rng.standard_normal(s).astype(T).astype(np.float64)
    Z, X, B = r(rows_x, mz), r(rows_x, nx), r(nx, n)
    h = 0.7 * float(np.sqrt(rows_x))
    want, mag = km.cross_apply(Z, X, h, B)
    for a in (Z, X, B, want, mag):
        a.setflags(write=False)
    return Z, X, B, h, want, mag


def _counts(ctx):
    return [ctx.rbf_path_count(w) for w in (55, 56, 57)]


def _check(got, want, mag, T, what, factor=FACTOR):
    eps = float(np.finfo(T).eps)
    bound = factor * eps * mag
    err = np.abs(got - want)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    print(f"{what}: max error / bound = {ratio:.3g} (in eps |K||B|: {ratio * factor:.3g})")
    assert np.all(err <= bound), f"{what}: max error / bound = {ratio:.3g}"


# ---------------------------------------------------------------------------------------------------
# 1. cross apply against the model, both precisions, both routes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rows_x", ROWS)
def test_cross_apply_matches_model(ctx, rows_x, shape, fused, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    mz, nx, n = shape
    Z, X, B, h, want, mag = _case(prec, rows_x, mz, nx, n)
    padded = shape == (65, 67, 17)                          # leading dimensions larger than the sizes
    Zd = _pts(Z, T, rows_x + 3 if padded else None)
    Xd = _pts(X, T, rows_x + 2 if padded else None)
    Bd = _pts(B, T, nx + 5 if padded else None)
    Cd = torch.full((n, mz + 1 if padded else mz), float("nan"), dtype=Zd.dtype, device="cuda:0")
    before = _counts(ctx)
    with ctx.options(rbf_fused=fused):
        dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n, C_=Cd)
    after = _counts(ctx)
    assert [a - b for a, b in zip(after, before)] == ([1, 0, 0] if fused else [0, 1, 0])
    got = _host(Cd, mz)
    _check(got, want, mag, T, f"rows_x={rows_x} {shape} fused={fused} {prec}")
    if padded:
        assert bool(torch.isnan(Cd[:, mz:]).all())         # the rows of C past mz are not written


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("rows_x,n", [(129, 16), (8, 65)])
def test_outside_the_fused_limits_takes_the_composed_route(ctx, rows_x, n, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    mz, nx = 65, 67
    Z, X, B, h, want, mag = _case(prec, rows_x, mz, nx, n)
    before = _counts(ctx)
    with ctx.options(rbf_fused=1):
        Cd = dev.rbf_cross_apply(ctx, _pts(Z, T), _pts(X, T), rows_x, mz, nx, h, _pts(B, T), n)
    assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 1, 0]
    _check(_host(Cd, mz), want, mag, T, f"rows_x={rows_x} n={n} {prec}")


# ---------------------------------------------------------------------------------------------------
# 2. alpha / beta and the empty shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
def test_alpha_beta(ctx, fused, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (65, 67, 17)
    Z, X, B, h, _, _ = _case(prec, rows_x, mz, nx, n)
    C0 = np.random.default_rng(9).standard_normal((mz, n)).astype(T).astype(np.float64)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=fused):
        # alpha = -0.5, beta = 2 on a random C
        want, mag = km.cross_apply(Z, X, h, B, -0.5, 2.0, C0)
        got = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n, alpha=-0.5, beta=2.0, C_=_pts(C0, T)), mz)
        _check(got, want, mag, T, f"alpha=-0.5 beta=2 fused={fused} {prec}")
        # beta = 0: C is not read
        Cn = torch.full((n, mz), float("nan"), dtype=Zd.dtype, device="cuda:0")
        got = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n, alpha=1.5, beta=0.0, C_=Cn), mz)
        assert not np.any(np.isnan(got))
        want, mag = km.cross_apply(Z, X, h, B, 1.5)
        _check(got, want, mag, T, f"beta=0 on NaN fused={fused} {prec}")
        # alpha = 0: C = beta C, exactly (one product per entry)
        got = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n, alpha=0.0, beta=2.0, C_=_pts(C0, T)), mz)
        assert np.array_equal(got, 2.0 * C0)
        # nx = 0: beta C
        Cn = torch.full((n, mz), float("nan"), dtype=Zd.dtype, device="cuda:0")
        got = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, 0, h, Bd, n, beta=0.0, C_=Cn), mz)
        assert np.array_equal(got, np.zeros((mz, n))) and not np.any(np.signbit(got))
        got = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, 0, h, Bd, n, beta=1.0, C_=_pts(C0, T)), mz)
        assert np.array_equal(got, C0)
        # mz = 0 and n = 0: nothing is touched
        before = _counts(ctx)
        Cd = _pts(C0, T)
        dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, 0, nx, h, Bd, n, alpha=3.0, beta=5.0, C_=Cd)
        dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, 0, alpha=3.0, beta=5.0, C_=Cd)
        assert np.array_equal(_host(Cd, mz), C0) and _counts(ctx) == before


# ---------------------------------------------------------------------------------------------------
# 3. what lies behind the last point is never read
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("fused", [1, 0])
def test_padding_is_masked(ctx, fused, prec):
    from randlapack_amd import device as dev
    import torch

    T = DT[prec]
    rows_x, (mz, nx, n) = 5, (65, 67, 17)
    Z, X, B, h, _, _ = _case(prec, rows_x, mz, nx, n)
    Zd = _pts(Z, T)
    with ctx.options(rbf_fused=fused):
        tight = dev.rbf_cross_apply(ctx, Zd, _pts(X, T), rows_x, mz, nx, h, _pts(B, T), n).cpu().numpy()
        # X with 61 more "points" and 3 more rows per point, B with 61 more rows: all 1e30
        Xb = torch.full((nx + 61, rows_x + 3), 1e30, dtype=Zd.dtype, device="cuda:0")
        Xb[:nx, :rows_x] = _pts(X, T)
        Bb = torch.full((n + 1, nx + 61), 1e30, dtype=Zd.dtype, device="cuda:0")
        Bb[:n, :nx] = _pts(B, T)
        loose = dev.rbf_cross_apply(ctx, Zd, Xb, rows_x, mz, nx, h, Bb, n).cpu().numpy()
    assert np.array_equal(tight, loose)


# ---------------------------------------------------------------------------------------------------
# 4. the bit contract of the fused route
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("rows_x", [5, 16])
def test_fused_bit_contract(ctx, rows_x, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    mz, nx, n = 200, 1000, 64
    Z, X, B, h, _, _ = _case(prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=1):
        before = _counts(ctx)
        a = dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
        b = dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(a, b)                                             # the same call twice
        part = dev.rbf_cross_apply(ctx, Zd[5:75], Xd, rows_x, 70, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(part, a[:, 5:75])                                 # a row does not depend on mz or on its place in Z
        same = dev.rbf_cross_apply(ctx, Xd, Xd, rows_x, nx, nx, h, Bd, n).cpu().numpy()
        copy = dev.rbf_cross_apply(ctx, Xd.clone(), Xd, rows_x, nx, nx, h, Bd, n).cpu().numpy()
        assert np.array_equal(same, copy)                                       # Z == X by pointer
        assert [x - y for x, y in zip(_counts(ctx), before)] == [5, 0, 0]


# ---------------------------------------------------------------------------------------------------
# 5. the two routes agree
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_routes_agree(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rows_x, (mz, nx, n) = 16, (200, 1000, 64)
    Z, X, B, h, _, mag = _case(prec, rows_x, mz, nx, n)
    Zd, Xd, Bd = _pts(Z, T), _pts(X, T), _pts(B, T)
    with ctx.options(rbf_fused=1):
        f = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n), mz)
    with ctx.options(rbf_fused=0):
        c = _host(dev.rbf_cross_apply(ctx, Zd, Xd, rows_x, mz, nx, h, Bd, n), mz)
    _check(f, c, mag, T, f"fused against composed {prec}", factor=2 * FACTOR)


@pytest.mark.parametrize("fused", [1, 0])
def test_fp32_scale_is_rounded_once_from_double(ctx, fused):
    """-1 / (2 h^2) is computed in double and rounded to float once.  A bandwidth is searched for which float arithmetic gives the
    neighbouring float; one entry with z = 0, x = (2, 2): both norms and the inner product are exact, the argument of exp is scale * 8
    (about -40), so the entry is expf of an exact product.  expf is accurate to 1 ulp; 4 eps are allowed.  The neighbouring scale moves
    the entry by |arg| ulp(scale) / scale >= 40 * 2^-24 = 20 eps."""
    from randlapack_amd import device as dev

    f = np.float32
    for i in range(1000):
        h = f(0.3) + f(i) * f(1e-4)
        once = f(-1.0 / (2.0 * float(h) * float(h)))
        in_t = f(-1.0) / (f(2.0) * h * h)
        if once != in_t:
            break
    assert once != in_t and 40.0 <= -8.0 * float(once) <= 48.0
    Z, X, B = np.zeros((2, 1)), np.full((2, 1), 2.0), np.ones((1, 1))
    with ctx.options(rbf_fused=fused):
        got = float(dev.rbf_cross_apply(ctx, _pts(Z, f), _pts(X, f), 2, 1, 1, float(h), _pts(B, f), 1).cpu().numpy()[0, 0])
    want = float(np.exp(float(once) * 8.0))
    print(f"h={float(h)!r}: error {abs(got - want) / want / float(np.finfo(f).eps):.3g} eps; the other scale would move it by "
          f"{abs(np.exp(float(in_t) * 8.0) - want) / want / float(np.finfo(f).eps):.3g} eps")
    assert abs(got - want) <= 4 * float(np.finfo(f).eps) * want


# ---------------------------------------------------------------------------------------------------
# 6. cross submatrix
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_cross_submatrix(ctx, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    rng = np.random.default_rng(3)
    rows_x, mz, nx = 7, 200, 300
    Xh = rng.standard_normal((rows_x, nx))
    Xh[:, 10] = Xh[:, 20]                                                     # repeated point
    Xh[:, 30:37] = np.eye(rows_x) * 2.0                                      # orthogonal points
    Zh = rng.standard_normal((rows_x, mz))
    Zh[:, 40] = Xh[:, 20]                                                     # a point of Z that is a point of X
    Zh[:, 50:57] = np.eye(rows_x) * 2.0
    Xd, Zd = _pts(Xh, T, rows_x + 1), _pts(Zh, T)
    Xh, Zh = Xh.astype(T).astype(np.float64), Zh.astype(T).astype(np.float64)
    tol = 1e-12 if T is np.float64 else 3e-5
    for h in (0.5, 1.0, 3.0):
        before = _counts(ctx)
        K = dev.sqexp_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 120, 90, 15, 7, h).cpu().numpy().T
        assert [a - b for a, b in zip(_counts(ctx), before)] == [0, 0, 1]
        np.testing.assert_allclose(K, km.cross_kernel(Zh, Xh, h)[15:135, 7:97], atol=tol, rtol=tol)
        # norms handed in: the same block
        nz, nxr = dev.sq_colnorms(ctx, Zd, rows_x, mz), dev.sq_colnorms(ctx, Xd, rows_x, nx)
        K2 = dev.sqexp_cross_submatrix(ctx, Zd, Xd, rows_x, mz, nx, 120, 90, 15, 7, h, sq_colnorms_z=nz, sq_colnorms_x=nxr).cpu().numpy().T
        assert np.array_equal(K, K2)
        # Z = X: the square routine's block
        Kc = dev.sqexp_cross_submatrix(ctx, Xd, Xd, rows_x, nx, nx, 120, 90, 15, 7, h).cpu().numpy().T
        Ks = dev.sqexp_submatrix(ctx, Xd, rows_x, nx, 120, 90, 15, 7, h).cpu().numpy().T
        np.testing.assert_allclose(Kc, Ks, atol=tol, rtol=tol)
        np.testing.assert_allclose(Kc, M.sqexp_matrix(Xh, h)[15:135, 7:97], atol=tol, rtol=tol)


# ---------------------------------------------------------------------------------------------------
# 7. argument codes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_argument_codes(ctx, prec):
    import torch

    T = DT[prec]
    ct = C.c_double if prec == "f64" else C.c_float
    rows_x, mz, nx, n = 3, 5, 6, 2
    dt = torch.float64 if prec == "f64" else torch.float32
    Z = torch.ones((mz, rows_x), dtype=dt, device="cuda:0")
    X = torch.ones((nx, rows_x), dtype=dt, device="cuda:0")
    B = torch.ones((n, nx), dtype=dt, device="cuda:0")
    Cm = torch.full((n, mz), 7.0, dtype=dt, device="cuda:0")
    good = dict(rows_x=rows_x, mz=mz, Z=Z.data_ptr(), ldz=rows_x, nx=nx, X=X.data_ptr(), ldx=rows_x, h=1.0, n=n, alpha=1.0, B=B.data_ptr(), ldb=nx,
                beta=0.0, C=Cm.data_ptr(), ldc=mz)
    fn = getattr(ctx.lib, f"rlhip_rbf_cross_apply_{prec}")

    def call(**kw):
        a = dict(good, **kw)
        return fn(ctx.h, a["rows_x"], a["mz"], a["Z"], a["ldz"], a["nx"], a["X"], a["ldx"], ct(a["h"]), a["n"], ct(a["alpha"]), a["B"], a["ldb"],
                  ct(a["beta"]), a["C"], a["ldc"])

    before = _counts(ctx)
    bad = [(dict(rows_x=0), -2), (dict(mz=-1), -3), (dict(Z=None), -4), (dict(ldz=rows_x - 1), -5), (dict(nx=-1), -6), (dict(X=None), -7),
           (dict(ldx=rows_x - 1), -8), (dict(h=0.0), -9), (dict(h=-1.0), -9), (dict(h=float("nan")), -9), (dict(n=-1), -10), (dict(B=None), -12),
           (dict(ldb=nx - 1), -13), (dict(C=None), -15), (dict(ldc=mz - 1), -16), (dict(rows_x=0, ldc=0), -2)]
    for kw, code in bad:
        assert call(**kw) == code, kw
    assert fn(None, rows_x, mz, Z.data_ptr(), rows_x, nx, X.data_ptr(), rows_x, ct(1.0), n, ct(1.0), B.data_ptr(), nx, ct(0.0), Cm.data_ptr(), mz) == -1
    torch.cuda.synchronize()
    assert _counts(ctx) == before and bool((Cm == 7.0).all())                 # nothing was launched
    # a NULL array that is not read is no error
    assert call(Z=None, X=None, B=None, alpha=0.0, beta=1.0) == 0
    assert call(Z=None, X=None, B=None, C=None, mz=0, ldc=1) == 0
    assert call() == 0
    assert ctx.rbf_path_count(54) == -1 and ctx.rbf_path_count(58) == -1 and ctx.path_count(55) == -1 and ctx.lsq_path_count(55) == -1
    # the submatrix entry
    sub = getattr(ctx.lib, f"rlhip_sqexp_cross_submatrix_{prec}")
    K = torch.zeros((nx, mz), dtype=dt, device="cuda:0")

    def csub(rows_x=rows_x, mz=mz, Zp=Z.data_ptr(), ldz=rows_x, nx=nx, Xp=X.data_ptr(), ldx=rows_x, rk=mz, ck=nx, Kp=K.data_ptr(), ldk=mz, ro=0, co=0,
             h=1.0):
        return sub(ctx.h, rows_x, mz, Zp, ldz, None, nx, Xp, ldx, None, rk, ck, Kp, ldk, ro, co, ct(h))

    before = _counts(ctx)
    for kw, code in [(dict(rows_x=0), -2), (dict(mz=-1), -3), (dict(Zp=None), -4), (dict(ldz=2), -5), (dict(nx=-1), -7), (dict(Xp=None), -8),
                     (dict(ldx=2), -9), (dict(ro=1), -11), (dict(rk=-1), -11), (dict(co=1), -12), (dict(Kp=None), -13), (dict(ldk=mz - 1), -14),
                     (dict(h=0.0), -17)]:
        assert csub(**kw) == code, kw
    assert _counts(ctx) == before
    assert csub() == 0
    assert np.array_equal(K.cpu().numpy(), np.ones((nx, mz), dtype=T))        # all points equal: K = 1 exactly


# ---------------------------------------------------------------------------------------------------
# 8. RBFKernelMatrix: matrix-free on request, the default untouched
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rbf_kernel_matrix_matrix_free(ctx, prec):
    """the inputs of test_gpu_rpchol.py::test_rbf_apply's (999, 7) case"""
    from randlapack_amd import device as dev

    T = DT[prec]
    m, d = 999, 7
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
    got = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True,
                               matrix_free=True)
    assert [a - b for a, b in zip(_counts(ctx), before)] == [1, 0, 0]
    _check(_host(got, m), want, mag, T, f"matrix-free with regs {prec}")
    eye = _pts(np.eye(m), T)
    got = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, eye, m, regs=(0.5,), eval_includes_reg=True, matrix_free=True)    # n = 999: composed
    tol = 1e-11 if T is np.float64 else 2e-4                                  # test_rbf_apply's tolerance for the same product
    np.testing.assert_allclose(_host(got, m), K + 0.5 * np.eye(m), atol=tol, rtol=tol)
    # the default: the bits of rlhip_rbf_apply_*, and no cross-kernel route
    before = _counts(ctx)
    a = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True)
    b = dev.rbf_apply(ctx, Xd, d, m, 1.0, _pts(B, T), 3, alpha=-0.5, beta=2.0, C_=_pts(C0, T), regs=regs, eval_includes_reg=True)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and _counts(ctx) == before
    a = dev.rbf_kernel_apply(ctx, Xd, d, m, 1.0, eye, m)
    b = dev.rbf_apply(ctx, Xd, d, m, 1.0, eye, m)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------------------------------------
# 9. fit, then predict
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", [("lockstep", 3), ("block", 4)])
def test_fit_then_predict(ctx, mode, s, prec):
    """the problem of test_gpu_pcg.py::test_krill_full_rpchol_rbf, then krr_predict at 130 fresh points"""
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, h, k, blk = 1000, 5, 3.0, 128, 16
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
    Zh = np.random.default_rng(303).standard_normal((rows_x, mz)).astype(T).astype(np.float64)
    before = _counts(ctx)
    Y = _host(dev.krr_predict(ctx, _pts(Zh, T), mz, Pd, rows_x, n, h, r["X"], s), mz)
    assert [a - b for a, b in zip(_counts(ctx), before)] == [1, 0, 0]
    K = km.cross_kernel(Zh, pts, h)
    mag = np.abs(K) @ np.abs(Xdev)
    _check(Y, K @ Xdev, mag, T, f"predict on the device's coefficients {mode} {prec}")
    eps = float(np.finfo(T).eps)
    slack = np.sum(np.abs(K), axis=1, keepdims=True) * float(np.max(np.abs(Xdev - Xstar.astype(np.float64))))
    err = np.abs(Y - K @ Xstar.astype(np.float64))
    print(f"predict against the planted coefficients {mode} {prec}: max error / allowed = {float(np.max(err / (slack + FACTOR * eps * mag))):.3g}")
    assert np.all(err <= slack + FACTOR * eps * mag)
