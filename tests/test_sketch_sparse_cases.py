"""CPU half of test_gpu_sketch_sparse.py: every case of tests/_sketch_sparse_cases.py is replayed through the plain-Python copy of the
host-side route decisions of sketch.hip / sparse.hip and must land on the route it is listed under; the exact cases must be exact on the
reference alone: |alpha| (|S| |A|) + |beta| |B0| (resp. |alpha| (|A_csr| |B|) + |beta| |C0|) in float64 stays below 2^24 for the fp32
cases and below 2^53 for the fp64 ones, so every order of summation gives the reference's bits."""
import numpy as np
import pytest
import scipy.sparse as sp

import _sketch_sparse_cases as sc


def _fits(bound, prec):
    top = float(np.max(bound)) if np.size(bound) else 0.0
    print(f"largest |alpha| sum |terms| + |beta c0| = {top:g} (2^{np.log2(max(top, 1)):.1f}), {sc.BITS[prec]} bits")
    assert top < 2.0 ** sc.BITS[prec]
    assert 2 * top < 2.0 ** sc.BITS[prec], "results are multiples of 1/2: one more bit"


def test_scalars_are_the_agreed_ones():
    assert sc.ALPHA in sc.ALPHAS and sc.BETA in sc.BETAS and 0.0 in sc.BETAS and sc.ENTRY_MAX == 8


# ---------------------------------------------------------------------------------------------------------------- generation
@pytest.mark.parametrize("name", [g.name for g in sc.GEN])
def test_generation_case_is_listed_under_its_route(name):
    g = sc.GEN_BY_NAME[name]
    route, counts, has16 = sc.build_replay(g.d, g.m, g.nnz, 1)
    assert route == g.route
    assert sc.build_replay(g.d, g.m, g.nnz, 0) == ("affine", {}, False)
    assert has16 == (g.d <= 32768)


def test_generation_gates_are_hit_on_both_sides():
    r = lambda d, m, nnz: sc.build_replay(d, m, nnz, 1)[0]
    assert r(64, 300, 8) == "lds" and r(64, 300, 9) == "chain:128"
    assert r(3351, 3401, 4) == "lds" and r(3352, 3402, 4) == "chain:8"
    assert 4 * 3351 * 11 <= 144 * 1024 < 4 * 3352 * 11
    assert r(64, 0, 4) == "none"
    listed = {g.route for g in sc.GEN}
    assert listed == {"lds", "chain:8", "chain:128", "none"}
    assert not sc.build_replay(40960, 37, 2, 1)[2] and sc.build_replay(32768, 37, 2, 1)[2]


# ---------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("name", [c.name for c in sc.APPLY])
def test_apply_case_is_listed_under_its_route(name):
    c = sc.APPLY_BY_NAME[name]
    r = c.route()
    print(name, r)
    assert r.sig == c.sig
    assert len(c.shard_sigs) == max(len(c.cuts) - 1, 0)
    for (r0, r1), sig in zip(zip(c.cuts[:-1], c.cuts[1:]), c.shard_sigs):
        s = c.route(r0, r1)
        print("  shard", r0, r1, s)
        assert s.sig == sig
    if len(c.cuts) == 4:                                                     # cuts lie inside blocks
        assert all(x % c.d for x in c.cuts[1:-1])
    assert (r.rc == -2) == (c.sig == "refused")


@pytest.mark.parametrize("name", [c.name for c in sc.APPLY if c.kind == "exact" and c.sig != "refused"])
def test_apply_case_is_exact_on_the_reference(name):
    c = sc.APPLY_BY_NAME[name]
    S, _ = sc.sketch_operator(c.d, c.m, c.nnz, c.mode)
    A, B0 = c.operands()
    assert np.abs(A).max(initial=0) <= sc.ENTRY_MAX and np.abs(B0).max() <= sc.ENTRY_MAX and np.array_equal(A, np.round(A))
    assert S.shape == (c.d, c.m) and (S.nnz == 0 or set(np.unique(np.abs(S.data))) == {1.0})
    _fits(sc.ALPHA * (abs(S) @ np.abs(A)) + abs(sc.BETA) * np.abs(B0), c.prec)


def test_apply_routes_counters_and_adjacent_gates():
    by = {}
    for c in sc.APPLY:
        r = c.route()
        by.setdefault(c.prec, {}).setdefault(c.sig, []).append(c.name)
        for (r0, r1), sig in zip(zip(c.cuts[:-1], c.cuts[1:]), c.shard_sigs):
            by[c.prec].setdefault("shard " + sig, []).append(c.name)
    for p in sc.PRECS:
        print(p, {k: len(v) for k, v in by[p].items()})
        e = 1 if p == "f64" else 2
        for ct, passes in ((4, _p(5120 * e)), (2, _p(5120 * e + 1)), (2, _p(10240 * e)), (1, _p(10240 * e + 1)), (1, _p(20480 * e))):
            assert f"staged:ct{ct}:nr8x{passes}" in by[p]
        for sig in ("refused", "empty", "staged:ct4:nr5x1", "staged:ct4:nr8x2", "dma:5", "dma:5+tail", "shard dma:5+head+tail"):
            assert sig in by[p], sig
    assert "dma:10+tail" in by["f64"] and "dma:1280+tail" in by["f64"] and "dma:10+tail" not in by["f32"]
    # the LDS-DMA route's gates, each missed alone next to a shape that passes them all
    R = sc.apply_replay
    for p, d in (("f64", 640), ("f32", 44)):
        m, lda = 9 * d + 6, 9 * d + 8
        assert R(p, 1, d, m, 4, lda=lda).counts == {sc.DMA: 1, sc.STAGED: 1}
        assert R(p, 1, d, m, 6, lda=lda).counts == {sc.STAGED: 1}                                   # n % 4
        assert R(p, 1, d, 7 * d, 4, lda=7 * d + 4).counts == {sc.STAGED: 1}                         # nfb >= 8
        assert R(p, 1, d, 8 * d, 4, lda=8 * d + 4).counts == {sc.DMA: 1}
        assert R(p, 1, d, m, 4, lda=lda, a_off=1).counts == {sc.STAGED: 1}                          # the pointer
        assert R(p, 1, d, m, 4, lda=lda - 1).counts == {sc.STAGED: 1}                               # lda
        assert R(p, 0, d, m, 4, lda=lda).counts == {sc.STAGED: 1}                                   # the operator's structure
    assert R("f64", 1, 641, 9 * 641 + 6, 4, lda=9 * 641 + 8).counts == {sc.STAGED: 1}               # d: 16-byte columns
    assert R("f64", 1, 1280, 9 * 1280 + 6, 4, lda=9 * 1280 + 8).NJ == "1280" and R("f64", 1, 1282, 9 * 1282 + 6, 4, lda=9 * 1282 + 8).counts == {sc.STAGED: 1}
    assert R("f64", 1, 640, 5766, 4, 1, 5765, 5768).counts == {sc.STAGED: 1} and R("f64", 1, 640, 5766, 4, 2, 5764, 5766).counts == {sc.DMA: 1, sc.STAGED: 1}
    # NJ: five pieces per wave up to 20 chunks of 64 pieces, ten beyond
    assert [R("f64", 1, d, 9 * d + 6, 4, lda=9 * d + 8).NJ for d in (640, 642, 1278, 1280)] == [5, 10, 10, "1280"]
    assert [R("f32", 1, d, 9 * d + 6, 4, lda=9 * d + 6 + 2).NJ for d in (44, 1276, 1280)] == [5, 5, 5]
    # slabs
    assert [R("f64", 0, d, 37, 5).CT for d in (5120, 5121, 10240, 10241, 20480)] == [4, 2, 2, 1, 1] and R("f64", 0, 20481, 37, 5).rc == -2
    assert [R("f32", 1, d, 37, 5).CT for d in (10240, 10241, 20480, 20481, 40960)] == [4, 2, 2, 1, 1] and R("f32", 1, 40961, 37, 5).rc == -2
    assert R("f64", 1, 2600, 3 * 2600 + 11, 5).NR == 8 and R("f64", 1, 2600, 3 * 2600 + 11, 5).passes == 2 and R("f64", 1, 1280, 5000, 5).NR == 5


def _p(d):
    return -(-d // 2048)


# ---------------------------------------------------------------------------------------------------------------- S * (sparse A)
@pytest.mark.parametrize("name", [c.name for c in sc.APPLY_CSR])
def test_apply_csr_case(name):
    c = sc.APPLY_CSR_BY_NAME[name]
    assert sc.apply_csr_replay(c.d, c.m, c.n, 0, c.d + c.ldb_pad) == c.rc
    rowptr, colidx, vals, A = c.matrix()
    lens = np.diff(rowptr)
    assert len(rowptr) == c.n + 1 and np.count_nonzero(A) == len(vals) and np.array_equal(vals, np.round(vals)) and np.abs(vals).max() <= sc.ENTRY_MAX
    if c.m >= 300:
        assert np.count_nonzero(lens == 0) == 3 and lens.max() == 300
    if c.rc == 0:
        S, _ = sc.sketch_operator(c.d, c.m, c.nnz, c.mode)
        _fits(sc.ALPHA * (abs(S) @ np.abs(A)) + abs(sc.BETA) * np.abs(c.b0()), c.prec)
    assert sc.apply_csr_replay(19200, 37, 3) == 0 and sc.apply_csr_replay(19201, 37, 3) == -2 and sc.apply_csr_replay(19201, 37, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- CSR products
@pytest.mark.parametrize("name", [c.name for c in sc.SPMM])
def test_spmm_case(name):
    c = sc.SPMM_BY_NAME[name]
    m, k, rowptr, colidx, vals = c.matrix()
    sig, counts = sc.spmm_replay(c.layout, m, c.nc)
    assert sig == c.sig and len(counts) == 1
    lens = np.diff(rowptr)
    if c.shape in ("std", "k1"):
        assert tuple(lens[:14]) == sc.ROW_LENGTHS and tuple(lens[-14:]) == sc.ROW_LENGTHS[::-1] and m == 150
        long_row = colidx[rowptr[13]:rowptr[14]]
        assert len(np.unique(long_row)) < len(long_row), "no duplicate column index in the 200-entry row"
        assert k == 1 or np.any(np.diff(colidx[rowptr[7]:rowptr[8]]) < 0), "sorted columns"
    if c.shape == "nnz0":
        assert len(vals) == 0
    if c.shape == "tall":
        assert m == 70001 and np.all(lens == 1) and m > 4 * 256 * 64, "the wide kernel's grid covers every row in one sweep"
    if c.kind == "exact":
        B, C0 = c.operands(m, k)
        _fits(sc.ALPHA * (sc.csr_dense(m, k, rowptr, colidx, np.abs(vals)) @ np.abs(B)) + abs(sc.BETA) * np.abs(C0), c.prec)


def test_spmm_routes_and_adjacent_widths():
    for p in sc.PRECS:
        got = {(c.layout, c.sig) for c in sc.SPMM if c.prec == p and c.kind == "exact"}
        assert got == {("C", "narrow-cm:16"), ("C", "narrow-cm:32"), ("R", "narrow-rm:16"), ("R", "narrow-rm:32")} | {(lay, f"wide:{w}") for lay in "CR" for w in (1, 2, 4)}
    r = lambda lay, nc: sc.spmm_replay(lay, 150, nc)[1]
    assert r("C", 32) == {sc.SPMM_NARROW_CM: 1} and r("C", 33) == {sc.SPMM_WIDE: 1} and r("R", 32) == {sc.SPMM_NARROW_RM: 1} and r("R", 33) == {sc.SPMM_WIDE: 1}
    assert sc.spmm_replay("R", 0, 5) == ("nothing", {}) and sc.spmm_replay("C", 5, 0) == ("nothing", {})


# ---------------------------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize("name", [t.name for t in sc.TRANSPOSE])
def test_transpose_case(name):
    t = sc.TRANSPOSE_BY_NAME[name]
    rowptr, colidx, vals = t.matrix()
    route, counts, longest = sc.transpose_replay(t.k, colidx)
    print(name, route, longest, len(colidx))
    assert route == t.route and (longest <= 512) == (route == "sort")
    clen = np.bincount(colidx, minlength=t.k)
    for j, L in t.long_cols.items():
        assert clen[j] == L
    assert len(np.unique(vals)) == len(vals) and len(vals) < 2 ** 24
    if t.m > 1 and t.k > 1:
        assert any(np.any(np.diff(colidx[a:b]) < 0) for a, b in zip(rowptr[:-1], rowptr[1:])), "column indices are sorted inside every row"
    if t.name == "m1":
        assert 4000 <= len(colidx) <= 6000 and clen.max() > 1
    # the reference of the GPU test is scipy's transpose; it is the stable sort by column (duplicates kept, in source-entry order)
    ref = sp.csr_matrix((vals, colidx, rowptr), shape=(t.m, t.k)).T.tocsr()
    rpt, cit, vt = sc.transpose_reference(t.m, t.k, rowptr, colidx, vals)
    assert np.array_equal(ref.indptr, rpt) and np.array_equal(ref.indices, cit) and np.array_equal(ref.data, vt)
    assert all(np.all(np.diff(cit[a:b]) >= 0) for a, b in zip(rpt[:-1], rpt[1:]))
    dup = [(a, b) for a, b in zip(rpt[:-1], rpt[1:]) if np.any(np.diff(cit[a:b]) == 0)]
    if t.name in ("m1", "m1-long", "rows-16-17", "row-512", "row-513", "k1"):
        assert dup, "no duplicate (row, column) pair"
    for a, b in dup:                                                          # equal source rows: ascending entry numbers (= values)
        same = np.diff(cit[a:b]) == 0
        assert np.all(np.diff(vt[a:b])[same] > 0)


def test_transpose_routes_and_the_512_boundary():
    assert {t.route for t in sc.TRANSPOSE} == {"sort", "count"}
    assert sc.transpose_replay(3, np.array([1] * 512 + [0]))[0] == "sort" and sc.transpose_replay(3, np.array([1] * 513))[0] == "count"
    assert sc.transpose_replay(3, np.zeros(0, dtype=np.int64))[0] == "nothing"
    lens = {L for t in sc.TRANSPOSE for L in t.long_cols.values()}
    assert {16, 17, 512, 513} <= lens


def test_densify_matrix_has_empty_long_and_duplicate_columns():
    rowptr, colidx, vals, m = sc.densify_matrix()
    lens = np.diff(rowptr)
    assert np.count_nonzero(lens == 0) >= 3 and lens.max() > 256
    assert any(len(np.unique(colidx[a:b])) < b - a for a, b in zip(rowptr[:-1], rowptr[1:]))
    _fits(np.abs(sc.csr_dense(len(lens), m, rowptr, colidx, np.abs(vals))), "f32")


def test_rounded_bound():
    assert sc.rounded_bound(5, 2.0, 3.0, -0.5, np.array(4.0)) == 8 * 2.0 ** -24 * 8.0
