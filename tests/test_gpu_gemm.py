"""Every route of the product layer (rlhip_gemm_*, rlhip_syrk_*, rlhip_gemm_norma_f64) in fp64 and fp32.

gemm.hip::gemm_impl picks one of about ten routes from the shapes alone; tests/_gemm_routes.py replays that choice in plain Python and
holds the case table (tests/test_gemm_routes.py checks the table on the CPU).  Each case here

  * asserts the route counters it moved (rlhip_path_count 0, 1, 26 .. 32) against the replay, so a changed gate cannot silently move the
    case to another kernel;
  * exact cases (the bulk): small-integer operands, alpha = 2, beta in {0, 1, -1/2} -- the float64 reference is representable in the type
    of the call and every order of summation gives its bits, so the WHOLE parent of C is compared bit for bit with what it must hold: a
    dropped, duplicated or misplaced term anywhere fails;
  * rounded cases (a few per route): Gaussian operands against the componentwise bound
        |C - ref| <= gamma_(k+2) (|alpha| |A| |B| + |beta| |C0|),   gamma_n = n u / (1 - n u),
    which holds for every order of summation in arithmetic of unit round-off u (k products, k - 1 additions, alpha, beta and the last
    addition), against a reference in higher precision (float64 for fp32, the 64-bit significand of long double for fp64); run twice,
    bit-identical;
  * poisoned padding: leading dimensions larger than the row counts with NaN in the guard rows of A, B and C, NaN columns behind A and B
    (and C), NaN in C where beta = 0, NaN in the strictly lower triangle of a syrk: the result must be finite and everything that is not
    the result bit-identical afterwards."""
import ctypes as C

import numpy as np
import pytest

import _gemm_routes as gr

pytestmark = pytest.mark.gpu

UINT = {"f64": np.uint64, "f32": np.uint32}


def _tdt(prec):
    import torch

    return torch.float64 if prec == "f64" else torch.float32


def _parent(M, ld, guard_cols, off, dt):
    """M (rows x cols, what the kernel may read) inside a column-major parent of NaN: leading dimension ld, guard_cols more columns,
    the base `off` elements into the allocation -> flat array"""
    rows, cols = M.shape
    assert ld > rows or rows == 0
    buf = np.full(off + ld * (cols + guard_cols), np.nan, dtype=dt)
    buf[off:].reshape(cols + guard_cols, ld)[:cols, :rows] = M.T
    return buf


def _upload(buf, off):
    import torch

    t = torch.from_numpy(buf).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t[off:]


def _counters(ctx):
    return {w: ctx.path_count(w) for w in gr.COUNTERS}


def _call(ctx, c, Ad, lda, Bd, ldb, Cd, ldc):
    if c.op == "syrk":
        return ctx.syrk("U", c.ta, c.n, c.k, c.alpha, Ad, lda, c.beta, Cd, ldc)
    return ctx.gemm(c.ta, c.tb, c.m, c.n, c.k, c.alpha, Ad, lda, Bd, ldb, c.beta, Cd, ldc)


def _reference(c, A, B, C0):
    if c.alpha == 0.0 or c.k == 0:                                  # BLAS: C = beta C, A and B are not referenced
        return c.beta * C0 if c.beta != 0.0 else np.zeros_like(C0)
    if c.kind == "exact" or c.prec == "f32":
        return c.alpha * (A @ B) + (c.beta * C0 if c.beta != 0.0 else 0.0)
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "the fp64 rounded cases need a reference above fp64"
    L = np.longdouble
    return L(c.alpha) * (A.astype(L) @ B.astype(L)) + L(c.beta) * C0.astype(L)


def _run(ctx, c):
    dt, off = gr.NPDT[c.prec], {"vec": 0, "odd": 0, "off": 1}
    m, n, k = c.m, c.n, c.k
    A, B, C0 = c.operands()
    lda, ldb, ldc = c.ld("a"), c.ld("b"), c.ldc()
    Ast = A.T if c.ta == "T" else A
    a_keep, Ad = _upload(_parent(Ast, lda, c.guard_cols(), off[c.amode], dt), off[c.amode])
    if c.same:
        b_keep, Bd = a_keep, Ad
    else:
        Bst = B.T if c.tb == "T" else B
        b_keep, Bd = _upload(_parent(Bst, ldb, c.guard_cols(), off[c.bmode], dt), off[c.bmode])
    upper = np.triu(np.ones((m, n), dtype=bool)) if c.tri else np.ones((m, n), dtype=bool)
    Cin = C0.copy()
    if c.beta == 0.0:
        Cin[:] = np.nan                                             # beta = 0: C is not read
    Cin[~upper] = np.nan                                            # syrk: the strictly lower triangle is neither read nor written
    cbuf = _parent(Cin, ldc, 1, 0, dt)
    want = c.route()
    assert want.sig == c.sig

    def once():
        c_keep, Cd = _upload(cbuf.copy(), 0)
        before = _counters(ctx)
        keep = ctx.lib.rlhip_avoid_persistent(ctx.h, 1) if c.avoid else None
        try:
            assert _call(ctx, c, Ad, lda, Bd, ldb, Cd, ldc) == 0
        finally:
            if c.avoid:
                ctx.lib.rlhip_avoid_persistent(ctx.h, keep)
        after = _counters(ctx)
        delta = {w: after[w] - before[w] for w in gr.COUNTERS if after[w] != before[w]}
        return c_keep.cpu().numpy(), delta

    got, delta = once()
    print(f"{c.name}: {c.sig}  counters {delta}  (replay {want.counts}, gate margin {want.margin:.3g})")
    assert delta == want.counts, f"route taken {delta}, replay says {want.counts} ({c.sig})"
    if c.avoid:
        assert 0 not in delta and 1 not in delta

    ref = _reference(c, A, B, C0)
    expect = cbuf.reshape(n + 1, ldc).copy()
    gotm = got.reshape(n + 1, ldc)
    U = UINT[c.prec]
    if c.kind == "exact":
        expect[:n, :m][upper.T] = ref.T[upper.T].astype(dt)
        # the result by value (np.array_equal's sense: no tolerance), the poison around it by its bits
        bad = np.argwhere(np.where(np.isnan(expect), expect.view(U) != gotm.view(U), expect != gotm))
        print(f"  exact: {len(bad)} of {expect.size} words of C's parent differ")
        if len(bad):
            j, i = bad[0]
            print(f"  first at row {i} column {j}: got {gotm[j, i]!r}, expected {expect[j, i]!r}; last at row {bad[-1][1]} column {bad[-1][0]}")
        assert len(bad) == 0
    else:
        res = gotm[:n, :m].T.astype(np.float64)
        assert np.all(np.isfinite(res[upper]))
        bound = gr.gamma(k + 2, c.prec) * (abs(c.alpha) * (np.abs(A) @ np.abs(B)) + abs(c.beta) * np.abs(C0))
        err = np.abs((res.astype(ref.dtype) - ref).astype(np.float64))
        ratio = float(np.max(err[upper] / bound[upper]))
        print(f"  rounded: max |C - ref| / bound = {ratio:.3g}")
        assert ratio <= 1.0
        outside = expect.copy()
        outside[:n, :m][upper.T] = 0
        inside = gotm.copy()
        inside[:n, :m][upper.T] = 0
        assert np.array_equal(outside.view(U), inside.view(U)), "guard rows, guard column or the lower triangle of C changed"
        again, _ = once()
        assert np.array_equal(again.view(U), got.view(U)), "not bitwise reproducible run to run"


@pytest.mark.parametrize("name", [c.name for c in gr.CASES])
def test_product(ctx, name):
    _run(ctx, gr.BY_NAME[name])


@pytest.mark.parametrize("ta", "NT")
def test_gemm_norma_on_a_shape_the_persistent_kernel_declines(ctx, ta):
    """the norm does not come out of the product there (fused == 0): a separate pass, still ||A||_F.  'N': the small kernel; 'T': a
    narrow tall product with a k remainder, which a fused-norm request keeps away from the narrow-panel kernel and from the k-remainder
    peel -- the tiled kernel with split-K."""
    import torch

    m, n, k = (300, 64, 200) if ta == "N" else (48, 64, 8192 + 5)
    rng = np.random.default_rng(5)
    A = rng.integers(-4, 5, (m, k)).astype(np.float64)
    B = rng.integers(-4, 5, (k, n)).astype(np.float64)
    Ast = A.T if ta == "T" else A
    lda, ldb, ldc = Ast.shape[0] + 4, k + 4, m + 4
    _, Ad = _upload(_parent(Ast, lda, 2, 0, np.float64), 0)
    _, Bd = _upload(_parent(B, ldb, 2, 0, np.float64), 0)
    cbuf = _parent(np.full((m, n), np.nan), ldc, 1, 0, np.float64)
    c_keep, Cd = _upload(cbuf.copy(), 0)
    want = gr.replay("f64", ta == "T", 0, m, n, k, 0, lda, ldb, norma=True)
    before = _counters(ctx)
    nrm, fused = ctx.gemm_norma(ta, "N", m, n, k, 2.0, Ad, lda, Bd, ldb, 0.0, Cd, ldc)
    after = _counters(ctx)
    delta = {w: after[w] - before[w] for w in gr.COUNTERS if after[w] != before[w]}
    print(ta, want.sig, delta, nrm, np.linalg.norm(A))
    assert delta == want.counts and gr.SK["f64"] not in delta and gr.SKINNY not in delta and gr.CUT not in delta
    assert fused == 0
    exact = np.sqrt(float(np.sum(A.astype(np.int64) ** 2)))       # (the separate pass is a scaled sum of squares: not exact to the bit)
    assert abs(nrm - exact) <= 1e-13 * exact
    expect = cbuf.reshape(n + 1, ldc).copy()
    expect[:n, :m] = (2.0 * (A @ B)).T
    assert np.array_equal(expect.view(np.uint64), c_keep.cpu().numpy().reshape(n + 1, ldc).view(np.uint64))
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", gr.PRECS)
def test_argument_codes(ctx, prec):
    """LAPACK-style argument numbers; nothing is written by a refused call, nor by one with m == 0 or n == 0"""
    import torch

    T = C.c_double if prec == "f64" else C.c_float
    gemm, syrk = getattr(ctx.lib, f"rlhip_gemm_{prec}"), getattr(ctx.lib, f"rlhip_syrk_{prec}")
    A = torch.ones(64 * 64, dtype=_tdt(prec), device="cuda")
    Cm = torch.full((64 * 64,), float("nan"), dtype=_tdt(prec), device="cuda")
    c0 = Cm.cpu().numpy().view(UINT[prec]).copy()
    a, b, c = A.data_ptr(), A.data_ptr(), Cm.data_ptr()

    def g(ta=b"N", tb=b"N", m=8, n=9, k=10, lda=None, ldb=None, ldc=None):
        lda = lda if lda is not None else (k if ta in b"Tt" else m)
        ldb = ldb if ldb is not None else (n if tb in b"Tt" else k)
        return gemm(ctx.h, ta, tb, m, n, k, T(2.0), a, lda, b, ldb, T(0.0), c, ldc if ldc is not None else m)

    before = _counters(ctx)
    assert g(ta=b"X") == -2 and g(tb=b"Q") == -3
    assert g(m=-1) == -3 and g(n=-1) == -4 and g(k=-1) == -5
    assert g(lda=7) == -8 and g(ta=b"T", lda=9) == -8
    assert g(ldb=9) == -10 and g(tb=b"T", ldb=8) == -10
    assert g(ldc=7) == -13
    assert g(m=0) == 0 and g(n=0) == 0 and g(m=0, ldc=1, lda=1) == 0
    s = lambda uplo=b"U", tr=b"T", n=8, k=10, lda=None, ldc=8: syrk(ctx.h, uplo, tr, n, k, T(2.0), a, lda if lda is not None else (k if tr in b"Tt" else n),
                                                                    T(0.0), c, ldc)
    assert s(uplo=b"L") == -2 and s(uplo=b"X") == -2 and s(tr=b"X") == -3
    assert s(n=-1) == -3                                            # (gemm_impl's own numbering from here on: m, n, k, lda, ldb, ldc)
    assert s(k=-1) == -5
    assert s(lda=9) == -8 and s(tr=b"N", lda=7) == -8 and s(ldc=7) == -13
    assert s(n=0) == 0
    assert _counters(ctx) == before, "a refused or empty call took a route"
    assert np.array_equal(Cm.cpu().numpy().view(UINT[prec]), c0)
    assert g() == 0 and g(ta=b"t", tb=b"c") == 0 and s(uplo=b"u", tr=b"n") == 0      # lower case and 'C' are accepted
    assert np.all(np.isfinite(Cm.cpu().numpy()[:8]))
