"""Every route of the row-pivoted LU (lu.hip, lu_f64.hip, lu_f32.hip: rlhip_getrf_*, rlhip_getrf_piv_*), of rlhip_laswp_* and of
rlhip_luqrcp_piv, in fp64 and fp32.

tests/_lu_cases.py holds the case tables, the input builders and a plain-Python replay of the host-side route decisions
(tests/test_lu_cases.py checks the tables and the reference on the CPU).  Each getrf case here

  * sits inside a column-major parent of NaN-payload poison: lda = m + pad, one guard column behind the matrix, the first element 3 words
    into the allocation when pad = 7; every word outside the m x n matrix must come back bit-identical;
  * 1. info and ipiv equal LAPACK's ({d,s}getrf of scipy on the same data) exactly;
  * 2. independently of LAPACK's pivots, the device's interchanges obey the first-maximum rule on the duplicate-row groups (current
       positions, not original indices);
  * 3. |P A - L U| <= gamma_(k+2) (|L| |U|) entrywise, k = min(i, j) + 1, gamma_t = t u / (1 - t u), in float64 (doubled for fp64 data,
       whose evaluation obeys the same bound): Higham's Theorem 9.3, +2 for the multiply by the pivot's reciprocal;
  * 4. |L| <= 1;
  * 5. rlhip_getrf_piv_* in the same precision: ipiv bitwise the full call's, the upper triangle of the first min(m, n) rows bitwise the
       full call's U, the same guards;
  * 6. moved the route counters 60 .. 64 and 7 exactly as the replay says.

rlhip_laswp_* and rlhip_luqrcp_piv move data only: bitwise against a serial NumPy loop."""
import numpy as np
import pytest

import _lu_cases as lc

pytestmark = pytest.mark.gpu

POISON = {"f64": 0x7FF80000DEADBEEF, "f32": 0x7FC0BEEF}


def _torch():
    import torch

    return torch


def _poison(n, prec):
    buf = np.empty(n, dtype=lc.UINT[prec])
    buf[:] = POISON[prec]
    return buf.view(lc.NPDT[prec])


def _parent(M, ld, prec, off=0, guard_cols=1):
    """M (rows x cols) inside a column-major parent of poison: leading dimension ld, guard_cols more columns, the first element `off` elements
    into the allocation -> flat array"""
    rows, cols = M.shape
    assert ld >= max(rows, 1)
    buf = _poison(off + ld * (cols + guard_cols), prec)
    buf[off:].reshape(cols + guard_cols, ld)[:cols, :rows] = M.T
    return buf


def _upload(buf, off=0):
    t = _torch().from_numpy(buf).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off * buf.itemsize


def _inside(buf, rows, cols, ld, off):
    """view of the rows x cols matrix inside a parent (transposed: [column, row])"""
    return buf[off:].reshape(-1, ld)[:cols, :rows]


def _assert_guards(before, after, rows, cols, ld, off, prec, what):
    """every word of the parent outside the rows x cols matrix is bit-identical"""
    U = lc.UINT[prec]
    a, b = before.view(U).copy(), after.view(U).copy()
    _inside(a, rows, cols, ld, off)[:] = 0
    _inside(b, rows, cols, ld, off)[:] = 0
    bad = np.flatnonzero(a != b)
    if len(bad):
        print(f"  {what}: {len(bad)} guard words changed; first at flat index {bad[0]} (row {(bad[0] - off) % ld}, column {(bad[0] - off) // ld}), "
              f"last at {bad[-1]}")
    assert len(bad) == 0, what


def _lu_counters(ctx):
    out = {w: ctx.lu_path_count(w) for w in range(60, 67)}
    out[lc.COLUMN] = ctx.path_count(lc.COLUMN)
    return out


def _delta(ctx, before):
    after = _lu_counters(ctx)
    return {w: after[w] - before[w] for w in after if after[w] != before[w]}


def test_lu_counter_range(ctx):
    assert ctx.lu_path_count(59) == -1 and ctx.lu_path_count(67) == -1 and ctx.lu_path_count(7) == -1
    assert all(ctx.lu_path_count(w) >= 0 for w in range(60, 67))
    assert ctx.path_count(60) == -1 and ctx.var_path_count(60) == -1


# ---------------------------------------------------------------------------------------------------------------- getrf
def _getrf(ctx, case, prec, pad, piv_only=False):
    """-> (rc, 0-based pivots, the parent before, the parent after, lda, off, counter deltas)"""
    torch = _torch()
    A = lc.getrf_input(case, prec)
    m, n = A.shape
    lda, off = m + pad, lc.off_of(pad)
    buf = _parent(A, lda, prec, off)
    keep, ptr = _upload(buf, off)
    ip = torch.full((min(m, n) + 2,), -77, dtype=torch.int64, device="cuda")           # two guard words behind the pivots
    before = _lu_counters(ctx)
    rc = getattr(ctx.lib, f"rlhip_getrf_{'piv_' if piv_only else ''}{prec}")(ctx.h, m, n, ptr, lda, ip.data_ptr())
    ctx.sync()
    delta = _delta(ctx, before)
    ipn = ip.cpu().numpy()
    assert np.all(ipn[min(m, n):] == -77), "pivot vector overrun"
    return rc, ipn[:min(m, n)] - 1, buf, keep.cpu().numpy(), lda, off, delta


def _check_getrf(ctx, case, prec, pad, expect_counts=None):
    A = lc.getrf_input(case, prec)
    m, n = A.shape
    k = min(m, n)
    replay = lc.getrf_replay(prec, m, n)
    lu_ref, piv_ref, info_ref = lc.lapack_getrf(A, prec)
    assert info_ref == (case.zero_col + 1 if case.zero_col >= 0 else 0)
    rc, piv, buf, got, lda, off, delta = _getrf(ctx, case, prec, pad)
    print(f"{case.name} {prec} pad {pad}: rc {rc}, {replay.sig}: counters {delta} (replay {replay.counts})")
    # 6. the route
    if expect_counts is None:
        assert delta == replay.counts, f"route taken {delta}, replay says {replay.counts} ({replay.sig})"
    else:
        expect_counts(delta, replay)
    # guards
    _assert_guards(buf, got, m, n, lda, off, prec, "getrf wrote outside the matrix")
    # 1. LAPACK's info and pivots
    assert rc == info_ref
    wrong = np.flatnonzero(piv != piv_ref)
    if len(wrong):
        j = wrong[0]
        print(f"  {len(wrong)} pivots differ from LAPACK's; first in column {j}: device {piv[j]}, LAPACK {piv_ref[j]}")
    assert len(wrong) == 0
    # 2. first maximum among exact ties, from the device's interchanges alone
    assert np.all((piv >= np.arange(k)) & (piv < m))
    bad = lc.first_maximum_violations(m, piv, case.groups(prec))
    assert not bad, f"(column, chosen position, earlier position of a tying row, that row): {bad}"
    # 3. backward error, 4. |L| <= 1
    LU = _inside(got, m, n, lda, off).T
    assert not np.isnan(LU).any()
    ratio, lmax = lc.backward_ratio(A, LU, piv, prec)
    print(f"  residual / bound {ratio:.3f}, max |L| {lmax:.6f}")
    assert ratio <= 1.0
    assert lmax <= 1.0
    # 5. pivots only
    rc2, piv2, buf2, got2, _, _, delta2 = _getrf(ctx, case, prec, pad, piv_only=True)
    assert rc2 == rc
    if expect_counts is None:
        assert delta2 == replay.counts
    else:
        expect_counts(delta2, replay)
    _assert_guards(buf2, got2, m, n, lda, off, prec, "getrf_piv wrote outside the matrix")
    assert np.array_equal(piv2, piv)
    U = lc.UINT[prec]
    iu = np.triu_indices(k, 0, n)
    LU2 = _inside(got2, m, n, lda, off).T
    same = LU[:k][iu].view(U) == LU2[:k][iu].view(U)
    assert same.all(), f"U of getrf_piv differs from getrf's in {np.count_nonzero(~same)} words"


@pytest.mark.parametrize("case,prec,pad", lc.getrf_ids(), ids=[lc.id_of(t) for t in lc.getrf_ids()])
def test_getrf(ctx, case, prec, pad):
    _check_getrf(ctx, case, prec, pad)


def test_getrf_column_at_a_time_leaves_guard_rows(ctx):
    """the column-at-a-time panel (test_gpu_kernels.py::test_getrf_very_tall_panels_match_lapack keeps the lda = m cases) with lda = m + 7 in
    fp32: taken above the resident capacity, an occupancy query, hence asserted through counter 7 alone"""
    case = lc.COLUMN_CASE

    def expect(delta, replay):
        assert delta.get(lc.COLUMN, 0) > 0
        assert sum(delta.get(w, 0) for w in (lc.COLUMN, lc.LDS, lc.FAST, lc.GENERAL)) == len(replay.panels)
        assert lc.OUTER not in delta and lc.SOLVE not in delta

    _check_getrf(ctx, case, "f32", case.pads[0], expect_counts=expect)


@pytest.mark.parametrize("prec", lc.PRECS)
def test_getrf_repeats_on_one_context(ctx, prec):
    """the tagged-word buffer and the barrier counter belong to the context: a fast-step call, an LDS call, then the first again, nothing but
    the calls in between; the third result is bitwise the first"""
    fast = next(c for c in lc.GETRF if (c.m, c.n) == (4096, 96))
    lds = next(c for c in lc.GETRF if (c.m, c.n) == (257, 33))
    ops = []
    for case in (fast, lds, fast):
        A = lc.getrf_input(case, prec)
        t, ptr = _upload(_parent(A, case.m + 7, prec, 3), 3)
        ip = _torch().zeros(min(A.shape), dtype=_torch().int64, device="cuda")
        ops.append((case, t, ptr, ip))
    rcs = [getattr(ctx.lib, f"rlhip_getrf_{prec}")(ctx.h, c.m, c.n, ptr, c.m + 7, ip.data_ptr()) for c, t, ptr, ip in ops]
    ctx.sync()
    assert rcs == [0, 0, 0]
    U = lc.UINT[prec]
    assert np.array_equal(ops[0][1].cpu().numpy().view(U), ops[2][1].cpu().numpy().view(U))
    assert np.array_equal(ops[0][3].cpu().numpy(), ops[2][3].cpu().numpy())
    for c, t, ptr, ip in ops[:2]:
        assert np.array_equal(ip.cpu().numpy() - 1, lc.lapack_getrf(lc.getrf_input(c, prec), prec)[1])


# ---------------------------------------------------------------------------------------------------------------- laswp
@pytest.mark.parametrize("pattern", lc.LASWP_PATTERNS)
@pytest.mark.parametrize("n", lc.LASWP_NS)
@pytest.mark.parametrize("prec", lc.PRECS)
def test_laswp(ctx, prec, n, pattern):
    torch = _torch()
    rows, lda, off = lc.LASWP_ROWS, lc.LASWP_ROWS + lc.LASWP_PAD, 1
    M = lc.laswp_matrix(n, prec)
    buf = _parent(M, lda, prec, off)
    pristine, _ = _upload(buf, off)
    U = lc.UINT[prec]
    for k1, k2 in lc.LASWP_RANGES:
        ipiv = lc.laswp_ipiv(pattern, k1, k2)
        work = pristine.clone()
        ip = torch.from_numpy(ipiv).to("cuda")
        rc = getattr(ctx.lib, f"rlhip_laswp_{prec}")(ctx.h, n, work.data_ptr() + off * buf.itemsize, lda, k1, k2, ip.data_ptr())
        ctx.sync()
        assert rc == 0
        expect = buf.copy()
        _inside(expect, rows, n, lda, off)[:] = lc.laswp_reference(M, k1, k2, ipiv).T
        got = work.cpu().numpy()
        bad = np.flatnonzero(expect.view(U) != got.view(U))
        if len(bad):
            i = bad[0]
            print(f"  {pattern} k1 {k1} k2 {k2}: {len(bad)} words differ; first at row {(i - off) % lda}, column {(i - off) // lda}: got {got[i]!r}, "
                  f"expected {expect[i]!r}")
        assert len(bad) == 0, (pattern, k1, k2)
        assert np.array_equal(ip.cpu().numpy(), ipiv)


# ---------------------------------------------------------------------------------------------------------------- luqrcp_piv
def _luqrcp(ctx, sd, cols, ipiv, route):
    torch = _torch()
    ip = torch.from_numpy(ipiv).to("cuda")
    J = torch.full((cols + 3,), -5, dtype=torch.int64, device="cuda")
    before = _lu_counters(ctx)
    rc = ctx.lib.rlhip_luqrcp_piv(ctx.h, sd, cols, ip.data_ptr(), J.data_ptr())
    ctx.sync()
    delta = _delta(ctx, before)
    assert rc == 0
    assert delta == lc.luqrcp_replay(sd, cols) == {lc.WALK if route == "walk" else lc.SERIAL: 1}
    Jn = J.cpu().numpy()
    assert np.all(Jn[cols:] == -5), "J overrun"
    ref = lc.luqrcp_reference(sd, cols, ipiv)
    bad = np.flatnonzero(Jn[:cols] != ref)
    if len(bad):
        print(f"  sd {sd} cols {cols}: {len(bad)} entries differ; first at {bad[0]}: got {Jn[bad[0]]}, expected {ref[bad[0]]}")
    assert len(bad) == 0
    assert np.array_equal(ip.cpu().numpy(), ipiv)


@pytest.mark.parametrize("sd,cols", lc.LUQRCP_SHAPES)
def test_luqrcp_piv_shapes(ctx, sd, cols):
    _luqrcp(ctx, sd, cols, lc.luqrcp_random_ipiv(sd, cols), lc.LUQRCP_ROUTE[(sd, cols)])


@pytest.mark.parametrize("kind", ["chain", "wrap"])
def test_luqrcp_piv_hash_collisions(ctx, kind):
    sd, cols, ipiv = lc.luqrcp_adversarial(kind)
    _luqrcp(ctx, sd, cols, ipiv, "walk")
