"""Every route of the sparse-sign sketching operator (sketch.hip: rlhip_saso_*) and of the CSR kernels (sparse.hip: rlhip_csr_*) in fp64 and
fp32, bit for bit.

tests/_sketch_sparse_cases.py holds the case tables and a plain-Python replay of the host-side route decisions (tests/test_sketch_sparse_cases.py
checks the tables on the CPU).  Each case here

  * asserts the route counters it moved (rlhip_path_count 14, 33 .. 42) against the replay, so a changed gate cannot silently move the case
    to another kernel;
  * takes S from the oracle's independent restatement of the stream (oracle.saso_dense), never from the device's own dense copy;
  * compares with np.array_equal's sense (no tolerance) against a float64 reference cast to the type of the call: operands hold integers
    |x| <= 8, alpha = 2, beta = -1/2 (and beta = 0 over a result full of NaN), the entries of S are +-1, so every order of summation gives
    the reference's bits in both precisions;
  * fills the guard rows of every padded operand (lda > m, ldb > d, ldc > m, ldo > m) and a guard column behind it with a NaN of a payload no
    arithmetic produces, and requires them back bit-identical;
  * one Gaussian fp32 case per family against the derived entrywise bound (L + 3) 2^-24 (|alpha| sum |terms| + |beta c0|), L = nonzeros of
    that sketch row / CSR row."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _sketch_sparse_cases as sc

pytestmark = pytest.mark.gpu

POISON = {"f64": 0x7FF80000DEADBEEF, "f32": 0x7FC0BEEF}


def _torch():
    import torch

    return torch


def _u32(v):
    return (C.c_uint32 * len(v))(*v)


def _poison(n, prec):
    buf = np.empty(n, dtype=sc.UINT[prec])
    buf[:] = POISON[prec]
    return buf.view(sc.NPDT[prec])


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


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda")


def _differences(expect, got, prec):
    """words that differ: results by value, poison by its bits"""
    U = sc.UINT[prec]
    return np.argwhere(np.where(np.isnan(expect), expect.view(U) != got.view(U), expect != got))


def _assert_same(expect, got, prec, what):
    bad = _differences(expect, got, prec)
    if len(bad):
        i = tuple(bad[0])
        print(f"  {what}: {len(bad)} of {expect.size} words differ; first at {i}: got {got[i]!r}, expected {expect[i]!r}; last at {tuple(bad[-1])}")
    assert len(bad) == 0, what


def _counters(ctx):
    return {w: ctx.path_count(w) for w in sc.COUNTERS}


def _delta(ctx, before):
    after = _counters(ctx)
    return {w: after[w] - before[w] for w in sc.COUNTERS if after[w] != before[w]}


def _create(ctx, d, m, nnz, mode):
    S, nxt = C.c_void_p(), (C.c_uint32 * 4)()
    rc = ctx.lib.rlhip_saso_create_mode(ctx.h, d, m, nnz, mode, _u32(sc.CTR), _u32(sc.KEY), nxt, C.byref(S))
    return rc, S, tuple(nxt)


# ---------------------------------------------------------------------------------------------------------------- SASO generation
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", [g.name for g in sc.GEN])
def test_saso_generation(ctx, orc, name, mode):
    g = sc.GEN_BY_NAME[name]
    _, counts, _ = sc.build_replay(g.d, g.m, g.nnz, mode)
    So, nxt_o = sc.sketch_operator(g.d, g.m, g.nnz, mode)
    before = _counters(ctx)
    rc, S, nxt = _create(ctx, g.d, g.m, g.nnz, mode)
    assert rc == 0
    try:
        delta = _delta(ctx, before)
        print(name, mode, delta, counts)
        assert delta == counts
        assert nxt == nxt_o                                                   # the state after the operator: integer-exact
        if g.m:
            assert set(np.diff(So.tocsc().indptr)) == {g.nnz}                 # (the oracle's operator: nnz distinct rows per column)
        dense = So.toarray()
        for prec in sc.PRECS:
            buf = _poison(g.d * g.m + 8, prec)
            keep, ptr = _upload(buf)
            assert getattr(ctx.lib, f"rlhip_saso_dense_{prec}")(ctx.h, S, ptr) == 0
            got = keep.cpu().numpy()
            expect = buf.copy()
            expect[:g.d * g.m] = dense.T.reshape(-1)
            _assert_same(expect, got, prec, f"dense copy {prec}")
    finally:
        ctx.lib.rlhip_saso_destroy(ctx.h, S)


# ---------------------------------------------------------------------------------------------------------------- SASO apply
def _apply_once(ctx, c, S, So, A, B0, r0, r1, beta, whole_entry):
    prec, dt = c.prec, sc.NPDT[c.prec]
    d, n, mloc = c.d, c.n, r1 - r0
    lda, ldb = c.lda(mloc), c.ldb()
    Aloc = A[r0:r1]
    abuf = _parent(Aloc, lda, prec, c.a_off)
    a_keep, a_ptr = _upload(abuf, c.a_off)
    Bin = B0 if beta != 0.0 else _poison(d * n, prec).reshape(d, n)
    bbuf = _parent(Bin, ldb, prec)
    b_keep, b_ptr = _upload(bbuf)
    want = c.route(r0, r1)
    before = _counters(ctx)
    if whole_entry:
        rc = getattr(ctx.lib, f"rlhip_saso_apply_{prec}")(ctx.h, S, n, sc.ALPHA, a_ptr, lda, beta, b_ptr, ldb)
    else:
        rc = getattr(ctx.lib, f"rlhip_saso_apply_rows_{prec}")(ctx.h, S, n, sc.ALPHA, a_ptr, lda, r0, mloc, beta, b_ptr, ldb)
    ctx.sync()
    delta = _delta(ctx, before)
    print(f"  rows [{r0}, {r1}) beta {beta}: rc {rc}, {want.sig}: counters {delta} (replay {want.counts}; CT {want.CT} NR {want.NR} x {want.passes} NJ {want.NJ})")
    assert rc == want.rc
    assert delta == want.counts, f"route taken {delta}, replay says {want.counts} ({want.sig})"
    got = b_keep.cpu().numpy()
    _assert_same(abuf, a_keep.cpu().numpy(), prec, "the operand changed")
    if rc != 0:
        _assert_same(bbuf, got, prec, "a refused call wrote")
        return
    Sl = So[:, r0:r1]
    ref = sc.ALPHA * (Sl @ Aloc) + (beta * B0 if beta != 0.0 else 0.0)
    expect = bbuf.copy().reshape(n + 1, ldb)
    gotm = got.reshape(n + 1, ldb)
    if c.kind == "exact":
        expect[:n, :d] = ref.T.astype(dt)
        _assert_same(expect, gotm, prec, "S A")
        return
    res = gotm[:n, :d].T.astype(np.float64)
    assert np.all(np.isfinite(res))
    L = np.diff(Sl.tocsr().indptr)[:, None]
    bound = sc.rounded_bound(L, sc.ALPHA, abs(Sl) @ np.abs(Aloc), beta, B0)
    ratio = float(np.max(np.abs(res - ref) / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"  rounded: max |B - ref| / bound = {ratio:.3g}")
    assert ratio <= 1.0
    expect[:n, :d] = gotm[:n, :d]
    _assert_same(expect, gotm, prec, "guard rows of B")


@pytest.mark.parametrize("name", [c.name for c in sc.APPLY])
def test_saso_apply(ctx, orc, name):
    c = sc.APPLY_BY_NAME[name]
    assert c.route().sig == c.sig
    So, _ = sc.sketch_operator(c.d, c.m, c.nnz, c.mode)
    A, B0 = c.operands()
    rc, S, _ = _create(ctx, c.d, c.m, c.nnz, c.mode)
    assert rc == 0
    print(name, c.sig)
    try:
        for beta in (sc.BETA, 0.0):
            if c.whole:
                _apply_once(ctx, c, S, So, A, B0, 0, c.m, beta, True)
            for r0, r1 in zip(c.cuts[:-1], c.cuts[1:]):
                _apply_once(ctx, c, S, So, A, B0, r0, r1, beta, False)
    finally:
        ctx.lib.rlhip_saso_destroy(ctx.h, S)


# ---------------------------------------------------------------------------------------------------------------- S * (sparse A)
@pytest.mark.parametrize("name", [c.name for c in sc.APPLY_CSR])
def test_saso_apply_csr(ctx, orc, name):
    c = sc.APPLY_CSR_BY_NAME[name]
    prec, dt, d, m, n = c.prec, sc.NPDT[c.prec], c.d, c.m, c.n
    fn = getattr(ctx.lib, f"rlhip_saso_apply_csr_{prec}")
    rowptr, colidx, vals, A = c.matrix()
    B0 = c.b0()
    ldb = d + c.ldb_pad
    So, _ = sc.sketch_operator(d, m, c.nnz, c.mode)
    rc, S, _ = _create(ctx, d, m, c.nnz, c.mode)
    assert rc == 0

    def run(rp, ci, v, row0, beta, ncols=n):
        """-> (return code, d x n result); the guard rows and the guard column of B must come back as they were"""
        Bin = B0 if beta != 0.0 else _poison(d * n, prec).reshape(d, n)
        bbuf = _parent(Bin, ldb, prec)
        b_keep, b_ptr = _upload(bbuf)
        rpd, cid, vd = _dev(rp.astype(np.int64)), _dev(np.concatenate((ci, [0])).astype(np.int64)), _dev(np.concatenate((v, [0.0])).astype(dt))
        r = fn(ctx.h, S, ncols, sc.ALPHA, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), beta, b_ptr, ldb, row0)
        ctx.sync()
        got = b_keep.cpu().numpy()
        if r != 0 or ncols == 0:
            _assert_same(bbuf, got, prec, "a refused or empty call wrote")
            return r, None
        gotm = got.reshape(n + 1, ldb)
        expect = bbuf.copy().reshape(n + 1, ldb)
        expect[:n, :d] = gotm[:n, :d]
        _assert_same(expect, gotm, prec, "guard rows of B")
        return r, gotm[:n, :d].T.copy()

    try:
        assert run(rowptr, colidx, vals, 0, sc.BETA, ncols=0)[0] == 0         # n == 0: nothing to do, nothing touched
        r, got = run(rowptr, colidx, vals, 0, sc.BETA)
        assert r == c.rc
        if c.rc != 0:
            return
        SA = So @ A
        assert np.array_equal(got, (sc.ALPHA * SA + sc.BETA * B0).astype(dt)), "whole operand"
        _, whole0 = run(rowptr, colidx, vals, 0, 0.0)
        assert np.array_equal(whole0, (sc.ALPHA * SA).astype(dt)), "whole operand, beta = 0 over NaN"
        # two row shards with local row indices and row0 = their offset
        cut = m // 2 + 1
        parts = []
        for r0, r1 in ((0, cut), (cut, m)):
            loc = sp.csc_matrix(A[r0:r1])
            loc.sort_indices()
            _, part = run(loc.indptr, loc.indices, loc.data, r0, 0.0)
            assert np.array_equal(part, (sc.ALPHA * (So[:, r0:r1] @ A[r0:r1])).astype(dt)), f"rows [{r0}, {r1})"
            parts.append(part)
        assert np.array_equal(parts[0] + parts[1], whole0)
        # the dense path on the same A: the same bits
        a_keep, a_ptr = _upload(_parent(A, m + 2, prec))
        b_keep, b_ptr = _upload(_parent(B0, ldb, prec))
        assert getattr(ctx.lib, f"rlhip_saso_apply_{prec}")(ctx.h, S, n, sc.ALPHA, a_ptr, m + 2, sc.BETA, b_ptr, ldb) == 0
        ctx.sync()
        assert np.array_equal(b_keep.cpu().numpy().reshape(n + 1, ldb)[:n, :d].T, got)
    finally:
        ctx.lib.rlhip_saso_destroy(ctx.h, S)


# ---------------------------------------------------------------------------------------------------------------- CSR products
@pytest.mark.parametrize("name", [c.name for c in sc.SPMM])
def test_csr_spmm(ctx, name):
    c = sc.SPMM_BY_NAME[name]
    prec, dt, nc = c.prec, sc.NPDT[c.prec], c.nc
    m, k, rowptr, colidx, vals = c.matrix()
    B, C0 = c.operands(m, k)
    sig, counts = sc.spmm_replay(c.layout, m, nc)
    assert sig == c.sig
    rpd, cid, vd = _dev(rowptr), _dev(np.concatenate((colidx, [0]))), _dev(np.concatenate((vals, [0.0])).astype(dt))
    Ad = sc.csr_dense(m, k, rowptr, colidx, vals)
    fn = getattr(ctx.lib, f"rlhip_csr_spmm_{prec}")
    for beta in (sc.BETA, 0.0):
        Cin = C0 if beta != 0.0 else _poison(m * nc, prec).reshape(m, nc)
        if c.layout == "C":
            ldb, ldc = k + 3, m + 5
            bbuf, cbuf = _parent(B, ldb, prec), _parent(Cin, ldc, prec)
        else:                                                                 # row-major: the column-major image of the transpose
            ldb, ldc = nc + 3, nc + 2
            bbuf, cbuf = _parent(B.T, ldb, prec), _parent(Cin.T, ldc, prec)
        b_keep, b_ptr = _upload(bbuf)
        c_keep, c_ptr = _upload(cbuf)
        before = _counters(ctx)
        assert fn(ctx.h, c.layout.encode(), m, nc, k, sc.ALPHA, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), b_ptr, ldb, beta, c_ptr, ldc) == 0
        ctx.sync()
        delta = _delta(ctx, before)
        print(f"{name} beta {beta}: {sig}, counters {delta}")
        assert delta == counts
        _assert_same(bbuf, b_keep.cpu().numpy(), prec, "the operand changed")
        ref = sc.ALPHA * (Ad @ B) + (beta * C0 if beta != 0.0 else 0.0)
        got = c_keep.cpu().numpy().reshape(-1, ldc)
        expect = cbuf.copy().reshape(-1, ldc)
        rt = ref.T if c.layout == "C" else ref
        if c.kind == "exact":
            expect[:rt.shape[0], :rt.shape[1]] = rt.astype(dt)
            _assert_same(expect, got, prec, "A B")
            continue
        res = got[:rt.shape[0], :rt.shape[1]].astype(np.float64)
        assert np.all(np.isfinite(res))
        bound = sc.rounded_bound(np.diff(rowptr)[:, None], sc.ALPHA, sc.csr_dense(m, k, rowptr, colidx, np.abs(vals)) @ np.abs(B), beta, C0)
        bt = bound.T if c.layout == "C" else bound
        ratio = float(np.max(np.abs(res - rt) / np.maximum(bt, np.finfo(np.float64).tiny)))
        print(f"  rounded: max |C - ref| / bound = {ratio:.3g}")
        assert ratio <= 1.0
        expect[:rt.shape[0], :rt.shape[1]] = got[:rt.shape[0], :rt.shape[1]]
        _assert_same(expect, got, prec, "guard rows of C")


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("c0,b", [(0, 12), (2, 9), (3, 1)])
def test_csr_densify_cols(ctx, prec, c0, b):
    """columns c0 .. c0 + b - 1 as a dense block: empty columns are zeroed, duplicate entries sum (integers: exactly, in any order)"""
    rowptr, colidx, vals, m = sc.densify_matrix()
    dense = sc.csr_dense(len(rowptr) - 1, m, rowptr, colidx, vals).T          # m x 12
    ldo = m + 3
    obuf = _parent(_poison(m * b, prec).reshape(m, b), ldo, prec)
    o_keep, o_ptr = _upload(obuf)
    rpd, cid, vd = _dev(rowptr), _dev(colidx), _dev(vals.astype(sc.NPDT[prec]))
    assert getattr(ctx.lib, f"rlhip_csr_densify_cols_{prec}")(ctx.h, m, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), c0, b, o_ptr, ldo) == 0
    ctx.sync()
    expect = obuf.copy().reshape(b + 1, ldo)
    expect[:b, :m] = dense[:, c0:c0 + b].T
    _assert_same(expect, o_keep.cpu().numpy().reshape(b + 1, ldo), prec, "dense block")


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", [t.name for t in sc.TRANSPOSE])
def test_csr_transpose(ctx, name, prec):
    torch = _torch()
    t = sc.TRANSPOSE_BY_NAME[name]
    dt = sc.NPDT[prec]
    rowptr, colidx, vals = t.matrix()
    nnz = len(colidx)
    route, counts, longest = sc.transpose_replay(t.k, colidx)
    assert route == t.route
    ref = sp.csr_matrix((vals, colidx, rowptr), shape=(t.m, t.k)).T.tocsr()    # a stable sort by column: duplicates kept, in source-entry order
    rpd, cid, vd = _dev(rowptr), _dev(colidx), _dev(vals.astype(dt))
    fn = getattr(ctx.lib, f"rlhip_csr_transpose_{prec}")
    outs = []
    for rep in range(2):
        rpt = torch.full((t.k + 3,), -7, dtype=torch.int64, device="cuda")
        cit = torch.full((nnz + 2,), -7, dtype=torch.int64, device="cuda")
        v_keep, v_ptr = _upload(_poison(nnz + 2, prec))
        before = _counters(ctx)
        assert fn(ctx.h, t.m, t.k, rpd.data_ptr(), cid.data_ptr(), vd.data_ptr(), rpt.data_ptr(), cit.data_ptr(), v_ptr) == 0
        ctx.sync()
        delta = _delta(ctx, before)
        print(f"{name} {prec}: {route}, longest transposed row {longest}, counters {delta}")
        assert delta == counts
        outs.append((rpt.cpu().numpy(), cit.cpu().numpy(), v_keep.cpu().numpy()))
    rp, ci, v = outs[0]
    assert np.array_equal(rp[:t.k + 1], ref.indptr) and np.all(rp[t.k + 1:] == -7)
    assert np.array_equal(ci[:nnz], ref.indices) and np.all(ci[nnz:] == -7)  # source rows ascending inside every transposed row
    assert np.array_equal(v[:nnz], ref.data.astype(dt))                       # distinct values: duplicates in source-entry order
    assert np.array_equal(v[nnz:].view(sc.UINT[prec]), _poison(2, prec).view(sc.UINT[prec]))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "not bitwise reproducible run to run"
