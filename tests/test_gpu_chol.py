"""Every route of the Cholesky layer (chol.hip: rlhip_potrf_*, and potrf_upper_enqueue through rlhip_cholqrq_*) in fp64 and fp32.

tests/_chol_cases.py holds the sizes, the input builders, the bounds and a replay of the route (tests/test_chol_cases.py checks them, and
a plain NumPy Cholesky against every limit used here, on the CPU).  Every potrf case here

  * sits in a column-major parent of NaN-payload poison: lda = n + 5, one guard column, the first element 3 words into the allocation,
    the strictly lower triangle of A poison as well.  Every word outside the upper triangle of the n x n matrix must come back
    bit-identical (guard rows, guard column, offset words, lower triangle), and the upper triangle finite: no poison reached the factor;
  * family E: the factor is the integer U, bit for bit in fp32, within tol_E in fp64 (the number of entries that are not bitwise U is
    printed, not asserted);
    family R: |A - R^T R| within the entrywise bound, the ratio printed per case and route; diag(R) > 0;
    both run a second time with lda = n and no offset, the layout the drivers use, the symmetric values below the diagonal: bitwise
    the first result, and the lower triangle bit-identical again (a quiet NaN may come back with its payload from `old - update`, so
    poison alone need not show an update that reaches below the diagonal; a finite value does);
  * family F: the return value is the failing position; rows above the pivot equal U through the columns of its 32-panel; the pivot
    entry is <= 0 (NaN for a NaN pivot, exactly 0 for a zero column)."""
import ctypes as C

import numpy as np
import pytest

import _chol_cases as cc

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _parent(M, ld, prec, off):
    """M (n x n) inside a column-major parent of poison: leading dimension ld, one guard column, the first element `off` elements into
    the allocation -> flat array"""
    n = M.shape[0]
    assert ld >= max(n, 1)
    buf = np.empty(off + ld * (n + 1), dtype=cc.UINT[prec])
    buf[:] = cc.POISON[prec]
    buf = buf.view(cc.NPDT[prec])
    buf[off:].reshape(n + 1, ld)[:n, :n] = M.T
    return buf


def _inside(buf, n, ld, off):
    """view of the n x n matrix inside a parent (transposed: [column, row])"""
    return buf[off:].reshape(-1, ld)[:n, :n]


def _assert_outside_upper_untouched(before, after, n, ld, off, prec, what):
    """every word of the parent outside the upper triangle of the n x n matrix is bit-identical"""
    U = cc.UINT[prec]
    a, b = before.view(U).copy(), after.view(U).copy()
    upper = np.tri(n, dtype=bool)                                             # [column, row]: row <= column
    _inside(a, n, ld, off)[upper] = 0
    _inside(b, n, ld, off)[upper] = 0
    bad = np.flatnonzero(a != b)
    if len(bad):
        r, c = (bad - off) % ld, (bad - off) // ld
        print(f"  {what}: {len(bad)} words outside the upper triangle changed; first at flat index {bad[0]} (row {r[0]}, column {c[0]}), last at "
              f"{bad[-1]} (row {r[-1]}, column {c[-1]}); {np.count_nonzero((r < n) & (c < n))} of them in the lower triangle, "
              f"{np.count_nonzero(r >= n)} in guard rows")
    assert len(bad) == 0, what


def _assert_bitwise(got, expect, prec, what):
    """got, expect: matrices of one shape; on a mismatch print where (rows modulo 16, columns modulo 32, the 256-blocks)"""
    U = cc.UINT[prec]
    diff = np.ascontiguousarray(got).view(U) != np.ascontiguousarray(expect).view(U)
    if diff.any():
        r, c = np.nonzero(diff)
        print(f"  {what}: {len(r)} of {diff.size} entries differ; rows {r.min()} .. {r.max()} ({len(set(r))} distinct, mod 16: {sorted(set(r % 16))}, "
              f"256-blocks {sorted(set(r // 256))}), columns {c.min()} .. {c.max()} (mod 32: {sorted(set(c % 32))}, 256-blocks {sorted(set(c // 256))}); "
              f"first ({r[0]}, {c[0]}): got {got[r[0], c[0]]!r}, expected {expect[r[0], c[0]]!r}")
    assert not diff.any(), what


def _assert_close(got, expect, tol, what):
    """max |got - expect| <= tol (NaN fails); on a miss print where, as _assert_bitwise does"""
    with np.errstate(invalid="ignore"):
        miss = ~(np.abs(got - expect) <= tol)
    if miss.any():
        r, c = np.nonzero(miss)
        print(f"  {what}: {len(r)} of {miss.size} entries off by more than {tol:.3g}; rows {r.min()} .. {r.max()} (mod 16: {sorted(set(r % 16))}, "
              f"256-blocks {sorted(set(r // 256))}), columns {c.min()} .. {c.max()} (mod 32: {sorted(set(c % 32))}, 256-blocks {sorted(set(c // 256))}); "
              f"first ({r[0]}, {c[0]}): got {got[r[0], c[0]]!r}, expected {expect[r[0], c[0]]!r}")
    assert not miss.any(), what


def _potrf(ctx, A, prec, pad=cc.PAD_A, off=cc.OFF, uplo=b"U", n=None, lda=None, untouched=False, symmetric=False):
    """A: symmetric float64 n x n.  Stores it (poison below the diagonal; the symmetric values with symmetric = True) in a poison parent,
    calls rlhip_potrf and checks every word outside the upper triangle (the whole parent with untouched = True)
    -> (return value, the n x n matrix as it came back)"""
    st = np.array(A, dtype=cc.NPDT[prec], order="C") if symmetric else cc.stored(A, prec)
    n0 = st.shape[0]
    ld = n0 + pad
    buf = _parent(st, ld, prec, off)
    t = _torch().from_numpy(buf).to("cuda")
    assert t.data_ptr() % 16 == 0
    rc = getattr(ctx.lib, f"rlhip_potrf_{prec}")(ctx.h, uplo, n0 if n is None else n, t.data_ptr() + off * buf.itemsize, ld if lda is None else lda)
    ctx.sync()
    got = t.cpu().numpy()
    what = f"potrf {prec} n = {n0} lda = n + {pad} offset {off}"
    if untouched:
        U = cc.UINT[prec]
        assert np.array_equal(got.view(U), buf.view(U)), f"{what}: the parent was written"
    else:
        _assert_outside_upper_untouched(buf, got, n0, ld, off, prec, what)
    return rc, _inside(got, n0, ld, off).T.copy()


def _check_e(e, R, prec, what):
    n = e.n
    up = np.triu_indices(n)
    assert np.isfinite(R[up]).all(), f"{what}: the upper triangle is not finite"
    Ru = np.triu(R)
    if prec == "f32":
        _assert_bitwise(Ru, e.U.astype(np.float32), prec, what)
    else:
        print(f"  {what}: {int(np.count_nonzero(Ru[up] != e.U[up]))} of {len(up[0])} entries are not bitwise U; max |R - U| = "
              f"{np.abs(Ru - e.U).max():.3g}, tol_E = {e.tol:.3g}")
        _assert_close(Ru, e.U, e.tol, what)


# ---------------------------------------------------------------------------------------------------------------- families E and R
@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n", sorted(cc.SIZES))
def test_potrf_family_e(ctx, n, prec):
    e = cc.family_e(n)
    r = cc.route(n)
    print(f"E n = {n} {prec}: {r.kind} {r.steps} ({cc.SIZES[n]})")
    rc, R = _potrf(ctx, e.A, prec)
    assert rc == 0
    _check_e(e, R, prec, f"E n = {n} {prec} {r.kind}")
    rc, R2 = _potrf(ctx, e.A, prec, pad=0, off=0, symmetric=True)
    assert rc == 0
    _assert_bitwise(np.triu(R2), np.triu(R), prec, "lda = n, offset 0, symmetric input against lda = n + 5, offset 3, poison below the diagonal")


@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n", sorted(cc.SIZES))
def test_potrf_family_r(ctx, n, prec):
    A = cc.family_r(n, prec)
    r = cc.route(n)
    rc, R = _potrf(ctx, A, prec)
    assert rc == 0
    assert np.isfinite(R[np.triu_indices(n)]).all(), "the upper triangle is not finite"
    ratio = cc.residual_ratio(A, R, prec)
    print(f"R n = {n} {prec} {r.kind}: max |A - R^T R| / bound = {ratio:.4g}")
    assert ratio <= 1.0
    assert (np.diag(R) > 0).all()
    rc, R2 = _potrf(ctx, A, prec, pad=0, off=0, symmetric=True)
    assert rc == 0
    _assert_bitwise(np.triu(R2), np.triu(R), prec, "lda = n, offset 0, symmetric input against lda = n + 5, offset 3, poison below the diagonal")


# ---------------------------------------------------------------------------------------------------------------- family F
def _check_f(n, pos, kind, prec, rc, R, U, tol):
    k = pos - 1
    assert rc == pos, f"potrf returned {rc}, the first pivot that is not positive is {pos}"
    cols = cc.checked_columns(n, k)
    got, want = np.triu(R)[:k, :cols], np.triu(U)[:k, :cols]
    what = f"F n = {n} position {pos} {kind} {prec}: rows 0 .. {k - 1}, columns 0 .. {cols - 1}"
    if prec == "f32":
        _assert_bitwise(got, want.astype(np.float32), prec, what)
    else:
        _assert_close(got, want, tol, what)
    if kind == "nan":
        assert np.isnan(R[k, k])
    elif kind == "zero":
        assert R[k, k] == 0.0
    else:
        assert R[k, k] <= 0.0


@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n,pos,kind", cc.f_ids(), ids=lambda v: str(v))
def test_potrf_family_f(ctx, n, pos, kind, prec):
    A, U, tol = cc.family_f(n, pos, kind)
    rc, R = _potrf(ctx, A, prec)
    print(f"F n = {n} position {pos} {kind} {prec} {cc.route(n).kind}: returned {rc}, pivot entry {R[pos - 1, pos - 1]!r}")
    _check_f(n, pos, kind, prec, rc, R, U, tol)


@pytest.mark.parametrize("prec", cc.PRECS)
def test_potrf_a_failure_does_not_leak_into_later_calls(ctx, prec):
    """the info word of a failed call stays in the mailbox: a small and a two-level success on the same context must not see it"""
    (n, pos, kind), small, two = cc.REPEAT
    A, U, tol = cc.family_f(n, pos, kind)
    rc, R = _potrf(ctx, A, prec)
    _check_f(n, pos, kind, prec, rc, R, U, tol)
    for m in (small, two):
        e = cc.family_e(m)
        rc, R = _potrf(ctx, e.A, prec)
        assert rc == 0, f"n = {m} after a failed call returned {rc}"
        _check_e(e, R, prec, f"E n = {m} {prec} after a failed call")


# ---------------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("prec", cc.PRECS)
def test_potrf_arguments(ctx, prec):
    """uplo = 'L' -> -2, n < 0 and lda < n -> negative, n = 0 -> 0; no word of the parent is written in any of them"""
    A = cc.family_e(33).A
    rc, _ = _potrf(ctx, A, prec, uplo=b"L", untouched=True)
    assert rc == -2
    rc, _ = _potrf(ctx, A, prec, n=-1, untouched=True)
    assert rc < 0
    rc, _ = _potrf(ctx, A, prec, lda=32, untouched=True)
    assert rc < 0
    rc, _ = _potrf(ctx, A, prec, n=0, untouched=True)
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------- potrf_upper_enqueue
def _cholqrq(ctx, prec, U):
    """A = [U; 0] (m x k, lda = m), R = a k x k buffer of poison -> (rc, info, A before, A after, R as k x k)"""
    torch = _torch()
    m, k = cc.CHOLQRQ_M, cc.CHOLQRQ_K
    T = cc.NPDT[prec]
    A = np.zeros((k, m), dtype=T)                                            # [column, row]
    A[:, :k] = U.T
    At = torch.from_numpy(A).to("cuda")
    keep = At.clone()
    Rbuf = np.empty(k * k, dtype=cc.UINT[prec])
    Rbuf[:] = cc.POISON[prec]
    Rt = torch.from_numpy(Rbuf.view(T)).to("cuda")
    info = C.c_int(-1)
    with ctx.options(cholqrq_one_stream=1):
        rc = getattr(ctx.lib, f"rlhip_cholqrq_{prec}")(ctx.h, m, k, At.data_ptr(), m, Rt.data_ptr(), 0, C.byref(info))
        ctx.sync()
    if rc == 1:
        pytest.skip(f"rlhip_cholqrq_{prec} does not serve {m} x {k} on this context (returned 1): potrf_upper_enqueue is not reached")
    return rc, int(info.value), keep, At, Rt.cpu().numpy().reshape(k, k).T


@pytest.mark.parametrize("prec", cc.PRECS)
def test_cholqrq_enqueued_potrf_success(ctx, prec):
    """A = [U; 0]: A^T A = U^T U exactly, the factor left in R by potrf_upper_enqueue is U"""
    e = cc.family_e(cc.CHOLQRQ_K)
    rc, info, _, _, R = _cholqrq(ctx, prec, e.U)
    assert rc == 0 and info == 0
    _check_e(e, R, prec, f"cholqrq {prec}: R")
    low = np.tril(R, -1)
    assert not np.isnan(R).any() and not low.any(), "the strictly lower part of R is not zero"


@pytest.mark.parametrize("prec", cc.PRECS)
def test_cholqrq_enqueued_potrf_failure(ctx, prec):
    """column 100 of A zero: the pivot is exactly zero, info = 101 comes back from the device word and A is left alone"""
    torch = _torch()
    U = cc.family_e(cc.CHOLQRQ_K).U.copy()
    U[:, cc.CHOLQRQ_ZERO_COLUMN] = 0.0
    rc, info, keep, At, _ = _cholqrq(ctx, prec, U)
    assert rc == 0
    assert info == cc.CHOLQRQ_ZERO_COLUMN + 1
    bits = torch.int64 if prec == "f64" else torch.int32
    assert torch.equal(At.view(bits), keep.view(bits)), "A was written although the factorization failed"
