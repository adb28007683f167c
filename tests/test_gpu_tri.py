"""Every route of the triangular layer (tri.hip: rlhip_trsm_*, rlhip_trsm_gather_*, rlhip_trsm_gather_range_*, rlhip_trmm_*) in fp64 and fp32.

tests/_tri_cases.py holds the case tables, the input builders, the bound and a plain-Python replay of the host-side route decisions
(tests/test_tri_cases.py checks them on the CPU).  Every case here

  * sits inside column-major parents of NaN-payload poison, one guard column behind each matrix, the first element 3 words into the
    allocation: B with ldb = m + 7 (every word outside the m x n matrix must come back bit-identical), the triangle A with lda = n + 5 and
    the source of an out-of-place solve with ldsrc = m + 9, both read-only (the whole parent bit-identical, compared on the device);
    the strictly lower triangle of A is poison too, and so is the diagonal of a Diag::Unit case;
  * 1. returns the code the replay says;
  * 2. moves the route counters 2, 3, 4 and 67 .. 73 exactly as the replay says, the guard's verdicts replayed in float64 from the input;
  * 3. family E: the result is alpha X bit for bit (every route must return the exact answer);
       family R: |X U - alpha B| stays within the entrywise bound of _tri_cases.py, the ratio printed per route;
  * 4. fused cases run a second time with ldb = m (out of place: ldb = m and ldsrc = m), the layout the drivers use: bitwise the first
       result."""
import numpy as np
import pytest

import _tri_cases as tc

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _poison(n, prec):
    buf = np.empty(n, dtype=tc.UINT[prec])
    buf[:] = tc.POISON[prec]
    return buf.view(tc.NPDT[prec])


def _parent(M, ld, prec, off=0, guard_cols=1):
    """M (rows x cols) inside a column-major parent of poison: leading dimension ld, guard_cols more columns, the first element `off` elements
    into the allocation -> flat array"""
    rows, cols = M.shape
    assert ld >= max(rows, 1)
    buf = _poison(off + ld * (cols + guard_cols), prec)
    buf[off:].reshape(cols + guard_cols, ld)[:cols, :rows] = M.T
    return buf


def _poison_parent(rows, cols, ld, prec, off=0, guard_cols=1):
    return _poison(off + ld * (cols + guard_cols), prec)


def _upload(buf, off=0):
    t = _torch().from_numpy(buf).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off * buf.itemsize


def _inside(buf, rows, cols, ld, off):
    """view of the rows x cols matrix inside a parent (transposed: [column, row])"""
    return buf[off:].reshape(-1, ld)[:cols, :rows]


def _assert_guards(before, after, rows, cols, ld, off, prec, what):
    """every word of the parent outside the rows x cols matrix is bit-identical"""
    U = tc.UINT[prec]
    a, b = before.view(U).copy(), after.view(U).copy()
    _inside(a, rows, cols, ld, off)[:] = 0
    _inside(b, rows, cols, ld, off)[:] = 0
    bad = np.flatnonzero(a != b)
    if len(bad):
        print(f"  {what}: {len(bad)} guard words changed; first at flat index {bad[0]} (row {(bad[0] - off) % ld}, column {(bad[0] - off) // ld}), "
              f"last at {bad[-1]}")
    assert len(bad) == 0, what


def _bits(t):
    torch = _torch()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _assert_untouched(t, keep, what):
    assert _torch().equal(_bits(t), _bits(keep)), f"{what} was written"


def _assert_bitwise(got, expect, prec, what):
    """got, expect: rows x cols; on a mismatch print where (which rows, which columns modulo 16, 32 and 256)"""
    U = tc.UINT[prec]
    diff = np.ascontiguousarray(got).view(U) != np.ascontiguousarray(expect).view(U)
    if diff.any():
        r, c = np.nonzero(diff)
        print(f"  {what}: {len(r)} of {diff.size} entries differ; rows {r.min()} .. {r.max()} ({len(set(r))} distinct, mod 16: {sorted(set(r % 16))}), "
              f"columns {c.min()} .. {c.max()} (mod 32: {sorted(set(c % 32))}, 256-blocks {sorted(set(c // 256))}); first ({r[0]}, {c[0]}): "
              f"got {got[r[0], c[0]]!r}, expected {expect[r[0], c[0]]!r}")
    assert not diff.any(), what


def _counters(ctx):
    out = {w: ctx.path_count(w) for w in (tc.FUSED, tc.SUBST, tc.OOP)}
    out.update({w: ctx.tri_path_count(w) for w in range(67, 74)})
    return out


def _delta(ctx, before):
    after = _counters(ctx)
    return {w: after[w] - before[w] for w in after if after[w] != before[w]}


def _num_cu():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


def test_tri_counter_range(ctx):
    assert ctx.tri_path_count(66) == -1 and ctx.tri_path_count(74) == -1 and ctx.tri_path_count(2) == -1
    assert all(ctx.tri_path_count(w) >= 0 for w in range(67, 74))
    assert ctx.path_count(67) == -1 and ctx.lu_path_count(67) == -1


# ---------------------------------------------------------------------------------------------------------------- trsm in place
class _A:
    """the triangle of a case on the device, inside its parent, with a copy to compare with afterwards"""

    def __init__(self, A, prec):
        self.n = A.shape[0]
        self.lda = self.n + tc.PAD_A
        self.t, self.ptr = _upload(_parent(A, self.lda, prec, tc.OFF), tc.OFF)
        self.keep = self.t.clone()

    def check(self):
        _assert_untouched(self.t, self.keep, "the triangle A (read-only)")


def _trsm(ctx, case, prec, inp, pad, A=None):
    """-> (X as m x n, counter deltas); asserts the return code, the guards and the read-only triangle"""
    m, n = case.m, case.n
    A = A or _A(inp.A, prec)
    ldb, off = m + pad, tc.off_of(pad)
    buf = _parent(inp.B, ldb, prec, off)
    Bt, Bptr = _upload(buf, off)
    before = _counters(ctx)
    rc = getattr(ctx.lib, f"rlhip_trsm_{prec}")(ctx.h, b"R", b"U", b"N", b"U" if case.unit else b"N", m, n, inp.alpha, A.ptr, A.lda, Bptr, ldb)
    ctx.sync()
    delta = _delta(ctx, before)
    assert rc == 0
    got = Bt.cpu().numpy()
    _assert_guards(buf, got, m, n, ldb, off, prec, f"trsm wrote outside B (ldb = m + {pad})")
    A.check()
    return _inside(got, m, n, ldb, off).T, delta


def _check_values(case, fam, prec, inp, X, what):
    if fam == "E":
        _assert_bitwise(X, inp.expect, prec, what)
        return
    assert not np.isnan(X).any()
    rows = tc.residual_rows(case.m)
    ratio = tc.residual_ratio(inp.U, inp.B[rows], inp.alpha, X[rows], prec, tc.routes_of(case))
    print(f"  {what}: max |R| / bound per route {ratio}")
    assert all(r <= 1.0 for r in ratio.values()), ratio


@pytest.mark.parametrize("case,fam,prec", tc.trsm_ids(), ids=[tc.id_of(t) for t in tc.trsm_ids()])
def test_trsm(ctx, case, fam, prec):
    ncu = _num_cu()
    if case.needs_cu and ncu != case.needs_cu:
        pytest.skip(f"the twelve-wavefront choice of this shape is stated for {case.needs_cu} compute units, the device has {ncu}")
    inp = tc.trsm_input(case, fam, prec)
    bad = tc.guard_verdicts(inp.U, case.unit) if case.n <= 2048 else case.bad
    assert bad == case.bad
    A = _A(inp.A, prec)
    first = None
    for pad in ((tc.PAD_B, 0) if case.fused else (tc.PAD_B,)):
        replay = tc.trsm_replay(prec, case.m, case.n, case.m + pad, bad, ncu)
        X, delta = _trsm(ctx, case, prec, inp, pad, A)
        print(f"{case.name} {fam} {prec} ldb m + {pad}: {replay.sig}: counters {delta} (replay {replay.counts})")
        assert delta == replay.counts, f"route taken {delta}, replay says {replay.counts} ({replay.sig})"
        assert replay.sig == case.sig
        _check_values(case, fam, prec, inp, X, f"{case.name} {replay.sig} ldb m + {pad}")
        if first is None:
            first = X.copy()
        else:
            _assert_bitwise(X, first, prec, "ldb = m against ldb = m + 7")


@pytest.mark.parametrize("prec", tc.PRECS)
@pytest.mark.parametrize("name", tc.XASM_CASES)
def test_trsm_xasm_option(ctx, name, prec):
    """the X-operand loads issued from inline asm or left to the compiler: the same bits, and the exact answer"""
    case = tc.trsm_case(name)
    inp = tc.trsm_input(case, "E", prec)
    replay = tc.trsm_replay(prec, case.m, case.n, case.m + tc.PAD_B, case.bad, _num_cu())
    out = []
    for xasm in (0, 1):
        with ctx.options(trsm_xasm=xasm):
            X, delta = _trsm(ctx, case, prec, inp, tc.PAD_B)
        assert delta == replay.counts
        _assert_bitwise(X, inp.expect, prec, f"{name} trsm_xasm = {xasm}")
        out.append(X.copy())
    _assert_bitwise(out[0], out[1], prec, "trsm_xasm 0 against 1")


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_nan_in_the_triangle_goes_to_substitution(ctx, prec):
    """one NaN strictly above the diagonal of a sub-block: the guard flags the block (no 67), substitution leaves the columns before the
    NaN's finite and within the bound and makes every later column NaN, as the float64 substitution does"""
    case = tc.NAN_CASE
    inp = tc.trsm_input(case, "R", prec)
    X, delta = _trsm(ctx, case, prec, inp, tc.PAD_B)
    replay = tc.trsm_replay(prec, case.m, case.n, case.m + tc.PAD_B, case.bad, _num_cu())
    print(f"nan {prec}: counters {delta} (replay {replay.counts})")
    assert delta == replay.counts == {tc.SUBST: 8}
    j = tc.NAN_AT[1]
    assert np.isfinite(X[:, :j]).all()
    assert np.isnan(X[:, j:]).all() and np.isnan(inp.expect[:, j:]).all()
    ratio = tc.residual_ratio(inp.U[:j, :j], inp.B[:, :j], inp.alpha, X[:, :j], prec, "S")
    print(f"  columns < {j}: max |R| / bound per route {ratio}")
    assert ratio["S"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------- out of place
class _Gather:
    """operands of an out-of-place solve on the device"""

    def __init__(self, prec, inp, Bsrc, perm, pad=tc.PAD_B, pad_src=tc.PAD_SRC):
        torch = _torch()
        self.prec, self.inp = prec, inp
        self.m, self.n = inp.B.shape
        self.nsrc = Bsrc.shape[1]
        self.A = _A(inp.A, prec)
        self.ldsrc, self.off_src = self.m + pad_src, tc.off_of(pad_src)
        self.src, self.src_ptr = _upload(_parent(Bsrc, self.ldsrc, prec, self.off_src), self.off_src)
        self.src_keep = self.src.clone()
        self.perm = None if perm is None else torch.from_numpy(perm).to("cuda")
        self.perm_keep = None if perm is None else self.perm.clone()
        self.ldb, self.off = self.m + pad, tc.off_of(pad)
        self.buf = _poison_parent(self.m, self.n, self.ldb, prec, self.off)
        self.B, self.B_ptr = _upload(self.buf, self.off)

    def call(self, ctx, rng=None, perm_ptr=None, nsrc=None, alias=False):
        """-> (rc, counter deltas); rng = (col0, col1): the range form"""
        pp = perm_ptr if perm_ptr is not None else (self.perm.data_ptr() if self.perm is not None else None)
        dst, ldb = (self.src_ptr, self.ldsrc) if alias else (self.B_ptr, self.ldb)
        before = _counters(ctx)
        if rng is None:
            rc = getattr(ctx.lib, f"rlhip_trsm_gather_{self.prec}")(ctx.h, b"N", self.m, self.n, self.inp.alpha, self.A.ptr, self.A.lda, self.src_ptr,
                                                                  self.ldsrc, pp, dst, ldb)
        else:
            rc = getattr(ctx.lib, f"rlhip_trsm_gather_range_{self.prec}")(ctx.h, b"N", self.m, nsrc or self.nsrc, self.inp.alpha, self.A.ptr, self.A.lda,
                                                                        self.src_ptr, self.ldsrc, pp, dst, ldb, rng[0], rng[1])
        ctx.sync()
        return rc, _delta(ctx, before)

    def result(self):
        got = self.B.cpu().numpy()
        _assert_guards(self.buf, got, self.m, self.n, self.ldb, self.off, self.prec, "the out-of-place solve wrote outside B")
        return _inside(got, self.m, self.n, self.ldb, self.off).T

    def check_read_only(self):
        self.A.check()
        _assert_untouched(self.src, self.src_keep, "the source (read-only)")
        if self.perm is not None:
            assert _torch().equal(self.perm, self.perm_keep)

    def assert_B_unchanged(self, what):
        U = tc.UINT[self.prec]
        assert np.array_equal(self.B.cpu().numpy().view(U), self.buf.view(U)), what


@pytest.mark.parametrize("prec", tc.PRECS)
@pytest.mark.parametrize("case", tc.GATHER_CASES, ids=lambda c: c.name)
def test_trsm_gather(ctx, case, prec):
    inp, Bsrc, perm = tc.gather_input(case.m, case.n, case.bad, prec, case.name, case.perm)
    assert tc.guard_verdicts(inp.U) == case.bad
    g = _Gather(prec, inp, Bsrc, perm)
    replay = tc.gather_replay(prec, case.m, case.n, g.ldb, g.ldsrc, case.bad, case.perm, num_cu=_num_cu())
    rc, delta = g.call(ctx)
    print(f"{case.name} {prec}: rc {rc}, counters {delta} (replay {replay.counts})")
    assert rc == replay.rc == 0
    assert delta == replay.counts == dict(case.counts)
    first = g.result()
    _assert_bitwise(first, inp.expect, prec, case.name)
    g.check_read_only()
    if tc.GATHER in replay.counts:
        return
    # the fused twins a second time in the layout the drivers use, ldb = m and ldsrc = m: the same route, the same bits
    g = _Gather(prec, inp, Bsrc, perm, pad=0, pad_src=0)
    assert (g.ldb, g.ldsrc) == (case.m, case.m)
    replay = tc.gather_replay(prec, case.m, case.n, g.ldb, g.ldsrc, case.bad, case.perm, num_cu=_num_cu())
    rc, delta = g.call(ctx)
    print(f"{case.name} {prec} ldb = ldsrc = m: rc {rc}, counters {delta} (replay {replay.counts})")
    assert rc == replay.rc == 0
    assert delta == replay.counts == dict(case.counts)
    _assert_bitwise(g.result(), first, prec, f"{case.name}: ldb = ldsrc = m against the padded layout")
    g.check_read_only()


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_gather_identity_twin_is_the_in_place_fused_solve(ctx, prec):
    """family R: the identity twin (OOP = 2) returns the bits of the in-place fused solve of a copy"""
    case = tc.trsm_case("fused-ragged-rows")
    inp = tc.trsm_input(case, "R", prec)
    g = _Gather(prec, inp, inp.B, None)
    rc, delta = g.call(ctx)
    assert rc == 0 and delta == {tc.OOP: 1, tc.IDENT: 1}
    X, d2 = _trsm(ctx, case, prec, inp, tc.PAD_B)
    assert d2 == {tc.FUSED: 1}
    got = g.result()
    _assert_bitwise(got, X, prec, "identity twin against the in-place fused solve")
    _check_values(case, "R", prec, inp, got, "identity twin")
    g.check_read_only()


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_gather_aliased(ctx, prec):
    """B == Bsrc: the in-place solver without a pivot vector, -14 with one"""
    case = tc.trsm_case("blk-ragged")
    inp, Bsrc, perm = tc.gather_input(case.m, case.n, case.bad, prec, case.name, True)
    g = _Gather(prec, inp, Bsrc, perm)
    rc, delta = g.call(ctx, alias=True)
    assert rc == -14 and delta == {}
    g.check_read_only()
    g.assert_B_unchanged("-14")
    inp, Bsrc, _ = tc.gather_input(case.m, case.n, case.bad, prec, case.name, False)
    g = _Gather(prec, inp, Bsrc, None)
    replay = tc.gather_replay(prec, case.m, case.n, g.ldsrc, g.ldsrc, case.bad, False, aliased=True)
    rc, delta = g.call(ctx, alias=True)
    assert rc == 0 and delta == replay.counts == {tc.BLK1: 2}
    got = g.src.cpu().numpy()
    _assert_guards(g.src_keep.cpu().numpy(), got, g.m, g.n, g.ldsrc, g.off_src, prec, "the aliased solve wrote outside the matrix")
    _assert_bitwise(_inside(got, g.m, g.n, g.ldsrc, g.off_src).T, inp.expect, prec, "aliased")
    g.A.check()
    g.assert_B_unchanged("the separate B of an aliased call")


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_gather_range_pieces_are_the_whole_solve(ctx, prec):
    """range(0, 256) then range(256, 512) into one poisoned B: bitwise the whole rlhip_trsm_gather result, which is the exact answer"""
    m, n = tc.RANGE_M, tc.RANGE_N
    inp, Bsrc, perm = tc.gather_input(m, n, (False, False), prec, "range-split", True)
    g = _Gather(prec, inp, Bsrc, perm)
    for rng in ((0, 256), (256, 512)):
        replay = tc.range_replay(m, n, g.ldb, (False, False), *rng)
        rc, delta = g.call(ctx, rng=rng)
        print(f"range {rng} {prec}: rc {rc}, counters {delta}")
        assert rc == replay.rc == 0 and delta == replay.counts == {tc.OOP: 1}
        if rng == (0, 256):
            U = tc.UINT[prec]
            part = g.B.cpu().numpy()
            assert np.all(_inside(part, m, n, g.ldb, g.off)[256:].view(U) == tc.POISON[prec]), "range(0, 256) wrote right of column 256"
    pieces = g.result()
    g.check_read_only()
    whole = _Gather(prec, inp, Bsrc, perm)
    rc, delta = whole.call(ctx)
    assert rc == 0 and delta == {tc.OOP: 1}
    _assert_bitwise(pieces, whole.result(), prec, "the pieces of a split solve against the whole solve")
    _assert_bitwise(pieces, inp.expect, prec, "split solve")


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_gather_range_pivots_into_a_wider_source(ctx, prec):
    """nsrc = 600 > col1 = 512: the pivots are a prefix of a permutation of 1 .. 600"""
    m, n, nsrc = tc.RANGE_M, tc.RANGE_N, tc.RANGE_NSRC_WIDE
    inp, Bsrc, perm = tc.gather_input(m, n, (False, False), prec, "range-wide", True, nsrc=nsrc, alpha=2.0)
    assert perm.max() > n
    g = _Gather(prec, inp, Bsrc, perm)
    rc, delta = g.call(ctx, rng=(0, n))
    assert rc == 0 and delta == {tc.OOP: 1}
    _assert_bitwise(g.result(), inp.expect, prec, "range with nsrc > col1")
    g.check_read_only()


@pytest.mark.parametrize("prec", tc.PRECS)
def test_trsm_gather_range_not_taken_and_errors_leave_B_alone(ctx, prec):
    torch = _torch()
    n = tc.RANGE_N
    # not taken: (a) too few rows, (b) a refused block
    for what, m, bad in (("m = 16000", 16000, (False, False)), ("refused block", tc.RANGE_M, (False, True))):
        inp, Bsrc, perm = tc.gather_input(m, n, bad, prec, "range-not-taken", True)
        assert tc.guard_verdicts(inp.U) == bad
        g = _Gather(prec, inp, Bsrc, perm)
        rc, delta = g.call(ctx, rng=(0, n))
        assert rc == tc.range_replay(m, n, g.ldb, bad, 0, n).rc == 1 and delta == {}, what
        g.assert_B_unchanged(what)
        g.check_read_only()
    # errors
    m = tc.RANGE_M
    inp, Bsrc, perm = tc.gather_input(m, n, (False, False), prec, "range-errors", True)
    g = _Gather(prec, inp, Bsrc, perm)
    twice = perm.copy()
    twice[300] = twice[7]
    twice_dev = torch.from_numpy(twice).to("cuda")
    for what, want, kw in (("col1 % 256 != 0", -7, dict(rng=(0, 300))),
                           ("nsrc < col1", -7, dict(rng=(0, n), nsrc=500)),
                           ("a repeated pivot entry", -7, dict(rng=(0, n), perm_ptr=twice_dev.data_ptr())),
                           ("aliasing", -14, dict(rng=(0, n), alias=True))):
        rc, delta = g.call(ctx, **kw)
        print(f"range error {prec}: {what}: rc {rc}")
        assert rc == want and delta == {}, what
        g.assert_B_unchanged(what)
        g.check_read_only()
    assert tc.range_replay(m, n, g.ldb, (False, False), 0, 300).rc == -7 and tc.range_replay(m, 500, g.ldb, (False, False), 0, n).rc == -7
    assert tc.range_replay(m, n, g.ldb, (False, False), 0, n, aliased=True).rc == -14


# ---------------------------------------------------------------------------------------------------------------- trmm
@pytest.mark.parametrize("side,trans,m,n,diag,prec", tc.trmm_ids(), ids=lambda v: str(v))
def test_trmm(ctx, side, trans, m, n, diag, prec):
    U, Astore, B, C = tc.trmm_input(side, trans, m, n, diag, prec)
    A = _A(Astore, prec)
    ldb, off = m + tc.PAD_B, tc.OFF
    buf = _parent(B, ldb, prec, off)
    Bt, Bptr = _upload(buf, off)
    before = _counters(ctx)
    rc = getattr(ctx.lib, f"rlhip_trmm_{prec}")(ctx.h, side.encode(), b"U", trans.encode(), diag.encode(), m, n, tc.TRMM_ALPHA, A.ptr, A.lda, Bptr, ldb)
    ctx.sync()
    delta = _delta(ctx, before)
    assert rc == 0
    assert delta == tc.trmm_replay(side, m, n)
    got = Bt.cpu().numpy()
    _assert_guards(buf, got, m, n, ldb, off, prec, "trmm wrote outside B")
    A.check()
    X = _inside(got, m, n, ldb, off).T
    assert not np.isnan(X).any()
    _assert_bitwise(X + tc.NPDT[prec](0), C + tc.NPDT[prec](0), prec, f"trmm side {side} trans {trans} diag {diag}")
