"""CPU half of test_gpu_tri.py: every case of tests/_tri_cases.py is replayed through the plain-Python copy of tri.hip's host-side route
decisions and must land on the signature it is listed under; every counter 2, 3, 4 and 67 .. 73 is moved by a listed case in each
precision it exists for; the conditioning margins of both input families hold; family E is exactly representable in fp32 and an emulation
of the device's algorithm in the working precision returns its exact answer; the same emulation stays within the entrywise bound on
family R.  The 32-bit offset gate of the fused kernel (4 ld + m >= 2^28: a parent above 60 GB) is checked here, in the replay, only."""
import numpy as np
import pytest

import _tri_cases as tc

EMU_ROWS = 96                     # rows are independent: the emulation runs on the first and last EMU_ROWS / 2 rows of a tall case


def _rows(m):
    return np.arange(m) if m <= 2 * EMU_ROWS else np.r_[0:EMU_ROWS // 2, m - EMU_ROWS // 2:m]


ALL = tc.trsm_ids() + [(tc.NAN_CASE, "R", p) for p in tc.PRECS]


# ---------------------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("case", tc.TRSM + [tc.NAN_CASE], ids=lambda c: c.name)
def test_trsm_case_is_listed_under_its_route(case):
    for prec in case.precs:
        for fam in case.fams:
            if case.n > 2048 and prec == "f64":
                continue                                                       # (the 8224-column triangle: one precision is enough here)
            inp = tc.trsm_input(case, fam, prec)
            bad = tc.guard_verdicts(inp.U, case.unit)
            assert bad == case.bad, (fam, prec, bad)
            for ldb in (case.m, case.m + tc.PAD_B):
                r = tc.trsm_replay(prec, case.m, case.n, ldb, bad)
                print(f"{case.name} {fam} {prec} ldb {ldb}: {r.sig} {r.counts}")
                assert r.rc == 0 and r.sig == case.sig
    assert len(case.sig.split("+")[0]) == case.nblk
    if case.needs_cu:
        # 304 compute units hold the 257 workgroups of 128 rows in one round; 384 workgroups stay two rounds
        assert tc.trsm_replay("f32", case.m, case.n, case.m, case.bad, num_cu=304).sig == ("F+12" if case.m == 49152 else "F")
        assert tc.trsm_replay("f64", case.m, case.n, case.m, case.bad).sig == "F"


def test_every_counter_is_moved_in_each_precision():
    for prec in tc.PRECS:
        moved = set()
        for c, fam, p in tc.trsm_ids():
            if p == prec:
                moved |= set(tc.trsm_replay(prec, c.m, c.n, c.m + tc.PAD_B, c.bad).counts)
        for g in tc.GATHER_CASES:
            r = tc.gather_replay(prec, g.m, g.n, g.m + tc.PAD_B, g.m + tc.PAD_SRC, g.bad, g.perm)
            assert tuple(sorted(r.counts.items())) == g.counts, g.name
            moved |= set(r.counts)
        for side, trans in tc.TRMM_FORMS:
            moved |= set(tc.trmm_replay(side, 7, 7))
        want = set(tc.COUNTERS) - ({tc.TWELVE} if prec == "f64" else set())
        assert moved == want, (prec, sorted(want - moved), sorted(moved - want))
    assert all(not tc.twelve_wavefronts("f64", m) for m in (32805, 49152))


def test_gates_on_both_sides():
    G = (False,)
    assert tc.trsm_replay("f64", 15, 128, 15, G).counts == {tc.SUBST: 4} and tc.trsm_replay("f64", 16, 128, 16, G).counts == {tc.BLK1: 1}
    assert tc.trsm_replay("f64", 300, 127, 300, G).counts == {tc.SUBST: 4}
    assert tc.trsm_replay("f64", 16383, 256, 16383, G).counts == {tc.BLK1: 1} and tc.trsm_replay("f64", 16384, 256, 16384, G).counts == {tc.FUSED: 1}
    assert tc.trsm_replay("f64", 16384, 255, 16384, G).counts == {tc.BLK1: 1}
    assert tc.trsm_replay("f64", 65535, 160, 65535, G).counts == {tc.BLK1: 1} and tc.trsm_replay("f64", 65536, 160, 65536, G).counts == {tc.BLK2: 1}
    # the block-count gate: 32 blocks may use the guard, 33 may not
    assert tc.trsm_replay("f32", 40, 8192, 40, (False,) * 32).counts == {tc.BLK1: 32}
    assert tc.trsm_replay("f32", 40, 8224, 40, (False,) * 33).counts == {tc.SUBST: 257}
    # the 32-bit lane offsets: 4 ld + m < 2^28
    m = 2 ** 28 // 5
    assert tc.tf_offsets_fit(m, m) and not tc.tf_offsets_fit(m + 1, m + 1)
    assert tc.trsm_replay("f64", m, 256, m, G).counts == {tc.FUSED: 1} and tc.trsm_replay("f64", m + 1, 256, m + 1, G).counts == {tc.BLK2: 1}
    assert tc.gather_replay("f64", m + 1, 256, m + 1, m + 1, G, False).counts == {tc.GATHER: 1, tc.BLK2: 1}
    big = 2 ** 26
    assert tc.gather_replay("f64", 16421, 256, 16421, big, G, False).counts == {tc.OOP: 1}            # the source's offsets only choose the twin
    assert tc.gather_replay("f64", 16421, 256, 16421, 16421, G, False).counts == {tc.OOP: 1, tc.IDENT: 1}
    # mixed verdicts: runs, hand-overs
    B_, G_ = True, False
    assert tc.trsm_replay("f64", 16421, 768, 16421, (G_, B_, G_)).counts == {tc.FUSED: 2, tc.SUBST: 8}
    assert tc.trsm_replay("f64", 16421, 582, 16421, (G_, G_, G_)).counts == {tc.FUSED: 1, tc.BLK1: 1}
    assert tc.trsm_replay("f64", 16421, 582, 16421, (B_, B_, G_)).counts == {tc.SUBST: 16, tc.BLK1: 1}
    assert tc.trsm_replay("f64", 65557, 288, 65557, (G_, G_)).counts == {tc.FUSED: 1, tc.BLK2: 1}
    # twelve wavefronts: 257 workgroups of 128 rows are two rounds on 256 compute units, 171 of 192 rows one
    assert tc.twelve_wavefronts("f32", 32805) and not tc.twelve_wavefronts("f32", 32768) and tc.twelve_wavefronts("f32", 49152)
    assert not tc.twelve_wavefronts("f32", 49153) and not tc.twelve_wavefronts("f32", 65557)
    # out of place
    assert tc.gather_replay("f64", 300, 300, 300, 300, (G_, G_), True, aliased=True).rc == -14
    assert tc.gather_replay("f64", 333, 300, 333, 333, (G_, G_), False, aliased=True).counts == {tc.BLK1: 2}
    assert tc.range_replay(16421, 512, 16421, (G_, G_), 256, 512).counts == {tc.OOP: 1}
    assert tc.range_replay(16000, 512, 16000, (G_, G_), 0, 512).rc == 1 and tc.range_replay(16421, 512, 16421, (G_, B_), 0, 512).rc == 1
    assert tc.range_replay(16421, 512, 16421, (G_, G_), 0, 300).rc == -7 and tc.range_replay(16421, 500, 16421, (G_, G_), 0, 512).rc == -7
    assert tc.range_replay(16421, 512, 16421, (G_, G_), 0, 512, aliased=True).rc == -14


# ---------------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("case,fam,prec", ALL, ids=[tc.id_of(t) for t in ALL])
def test_conditioning_margins(case, fam, prec):
    if case is tc.NAN_CASE:
        inp = tc.trsm_input(case, fam, prec)
        k2 = tc.sub_block_kappa2(inp.U)
        i, j = tc.NAN_AT
        assert i < j and i // tc.SB == j // tc.SB and np.isnan(inp.U[i, j]) and np.count_nonzero(np.isnan(inp.U)) == 1
        assert np.isinf(k2[i // tc.SB]) and np.all(k2[np.arange(len(k2)) != i // tc.SB] <= tc.KAPPA2_GOOD)
        return
    inp = tc.trsm_input(case, fam, prec)
    k2 = tc.sub_block_kappa2(inp.U, case.unit)
    graded = {r0 // tc.SB for r0, _ in tc._grading(case.bad, case.n)}
    good = np.array([s not in graded for s in range(len(k2))])
    print(f"{case.name} {fam} {prec}: good kappa_F^2 <= {k2[good].max():.3g}" + (f", bad >= {k2[~good].min():.3g}" if graded else ""))
    assert np.all(k2[good] <= tc.KAPPA2_GOOD)
    assert np.all(k2[~good] >= tc.KAPPA2_BAD)
    assert len(graded) == sum(case.bad)


@pytest.mark.parametrize("w", (1, 2, 17, 31))
def test_a_ragged_block_without_a_full_sub_block_can_be_refused(w):
    """the device pads a ragged sub-block with the identity before it takes the norms, so even one column fails the guard when it is
    small enough: (31 + u^2) (31 + 1 / u^2) for a 1 x 1 block holding u.  Both families grade such a block past the margin, and family E
    stays exact through substitution."""
    n, bad = tc.BW + w, (False, True)
    assert tc._grading(bad, n) == [(tc.BW, w)]
    for prec in tc.PRECS:
        e = tc.family_e(40, n, bad, prec, False, -0.5, 7)
        r = tc.family_r(40, n, bad, prec, False, 7)
        for inp in (e, r):
            k2 = tc.sub_block_kappa2(inp.U)
            assert np.all(k2[:-1] <= tc.KAPPA2_GOOD) and k2[-1] >= tc.KAPPA2_BAD
            assert tc.guard_verdicts(inp.U) == bad
        got = tc.emulate_trsm(e.U, e.B, e.alpha, prec, (True, False))
        assert np.array_equal(got.view(tc.UINT[prec]), e.expect.view(tc.UINT[prec]))
    u = 2.0 ** -tc.RAGGED_GRADING_START
    k2 = tc.sub_block_kappa2(tc.family_e(1, tc.BW + 1, bad, "f64", False, -0.5, 7).U)[-1]
    assert k2 == pytest.approx((31 + u * u) * (31 + 1 / (u * u)), rel=1e-12) and 5.2e8 < k2 < 5.3e8


# ---------------------------------------------------------------------------------------------------------------- family E
@pytest.mark.parametrize("case", [c for c in tc.TRSM if c.n <= 2048], ids=lambda c: c.name)
def test_family_e_is_exact_in_fp32(case):
    a, b = tc.trsm_input(case, "E", "f64"), tc.trsm_input(case, "E", "f32")
    for x, y in ((a.U, b.U), (a.B, b.B), (a.expect, b.expect)):
        assert np.array_equal(x, y.astype(np.float64))
    # the float64 build is what it claims: X U = B, alpha X expected, small integers on the right-hand side, no zero in the solution
    X = a.expect / a.alpha
    rows = _rows(case.m)
    assert np.array_equal(X[rows] @ a.U, a.B[rows])
    assert np.array_equal(a.B, np.rint(a.B)) and np.abs(a.B).max() <= 3 * (2 + 16 + 1)
    assert np.all(a.expect != 0)
    n = case.n
    low = np.tri(n, k=0 if case.unit else -1, dtype=bool)
    assert np.all(a.A.view(np.uint64)[low] == tc.POISON["f64"]) and np.array_equal(a.A[~low], a.U[~low])
    assert np.all(b.A.view(np.uint32)[low] == tc.POISON["f32"])
    assert a.alpha in (-0.5, 2.0)


@pytest.mark.parametrize("case,prec", [(c, p) for c in tc.TRSM for p in c.precs if not (c.n > 2048 and p == "f64")],
                         ids=lambda v: getattr(v, "name", v))
def test_emulation_returns_the_exact_answer_on_family_e(case, prec):
    inp = tc.trsm_input(case, "E", prec)
    rows = _rows(case.m)
    got = tc.emulate_trsm(inp.U, inp.B[rows], inp.alpha, prec, tc.inverse_blocks_of(case))
    U = tc.UINT[prec]
    assert got.dtype == tc.NPDT[prec]
    assert np.array_equal(got.view(U), np.ascontiguousarray(inp.expect[rows]).view(U))
    # and on the other route of every block
    other = tuple(not b and not bad for b, bad in zip(tc.inverse_blocks_of(case), case.bad))
    if case.n <= 1024:
        got = tc.emulate_trsm(inp.U, inp.B[rows], inp.alpha, prec, other)
        assert np.array_equal(got.view(U), np.ascontiguousarray(inp.expect[rows]).view(U))


# ---------------------------------------------------------------------------------------------------------------- family R
R_IDS = [(c, p) for c in tc.TRSM for p in c.precs if "R" in c.fams]


@pytest.mark.parametrize("case,prec", R_IDS, ids=lambda v: getattr(v, "name", v))
def test_emulation_stays_within_the_bound_on_family_r(case, prec):
    inp = tc.trsm_input(case, "R", prec)
    rows = _rows(case.m)
    inv = tc.inverse_blocks_of(case)
    X = tc.emulate_trsm(inp.U, inp.B[rows], inp.alpha, prec, inv)
    ratio = tc.residual_ratio(inp.U, inp.B[rows], inp.alpha, X, prec, tc.routes_of(case))
    print(f"{case.name} {prec}: emulation residual / bound {ratio}")
    assert all(r <= 1.0 for r in ratio.values())
    assert set(ratio) == set(tc.routes_of(case))
    # the bound is not vacuous: one entry (the largest of a middle column) off by 1e-9 (fp64) / 1e-2 (fp32) relative is seen
    Xw = X.copy()
    Xw[np.argmax(np.abs(X[:, case.n // 2])), case.n // 2] *= 1 + (1e-9 if prec == "f64" else 1e-2)
    assert max(tc.residual_ratio(inp.U, inp.B[rows], inp.alpha, Xw, prec, tc.routes_of(case)).values()) > 1.0


def test_reference_agrees_with_scipy():
    from scipy.linalg import solve_triangular

    inp = tc.trsm_input(tc.trsm_case("ragged-sub"), "R", "f64")
    X = tc.solve_reference(inp.U, inp.B, inp.alpha)
    ref = solve_triangular(inp.U, inp.alpha * inp.B.T, trans="T", lower=False).T
    assert np.abs(X - ref).max() <= 1e-13 * np.abs(ref).max()
    D = tc.inverse_by_columns(inp.U[:32, :32].copy())
    assert np.allclose(D @ inp.U[:32, :32], np.eye(32), atol=1e-13)


def test_nan_reference():
    inp = tc.trsm_input(tc.NAN_CASE, "R", "f64")
    j = tc.NAN_AT[1]
    assert np.isfinite(inp.expect[:, :j]).all() and np.isnan(inp.expect[:, j:]).all()
    assert tc.guard_verdicts(inp.U) == (True,)


# ---------------------------------------------------------------------------------------------------------------- out of place, trmm
@pytest.mark.parametrize("prec", tc.PRECS)
def test_gather_inputs(prec):
    inp, Bsrc, p = tc.gather_input(300, 256, (False,), prec, "t", True, nsrc=300)
    assert Bsrc.shape == (300, 300) and len(set(p)) == 256 and p.min() >= 1 and p.max() <= 300
    assert np.array_equal(Bsrc[:, p - 1], inp.B)
    assert np.count_nonzero(np.isnan(Bsrc).all(axis=0)) == 44
    inp, Bsrc, p = tc.gather_input(300, 256, (False,), prec, "t", False)
    assert p is None and Bsrc is inp.B


def test_trmm_inputs_are_exact():
    for side, trans, m, n, diag, prec in tc.trmm_ids():
        U, A, B, C = tc.trmm_input(side, trans, m, n, diag, prec)
        assert U.dtype == tc.NPDT[prec] and np.array_equal(C, np.rint(2 * C) / 2)
        U64, B64 = U.astype(np.float64), B.astype(np.float64)
        ref = tc.TRMM_ALPHA * (B64 @ U64 if side == "R" else (U64.T if trans == "T" else U64) @ B64)
        assert np.array_equal(C.astype(np.float64), ref)
        assert tc.trmm_replay(side, m, n) == {tc.TRMM_R if side == "R" else tc.TRMM_L: 1}


# ---------------------------------------------------------------------------------------------------------------- the export
def test_tri_path_count_is_exported():
    from randlapack_amd import _lib

    assert "rlhip_tri_path_count" in _lib.SIGNATURES
    lib = _lib.load()
    for which in (66, 67, 73, 74, 2, -1):
        assert lib.rlhip_tri_path_count(None, which) == -1
