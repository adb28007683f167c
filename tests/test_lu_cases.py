"""CPU half of test_gpu_lu.py: every case of tests/_lu_cases.py is replayed through the plain-Python copy of rlhip::getrf's host-side route
decisions and must land on the route it is listed under; every gate is hit on both sides by a listed case; and the reference alone (LAPACK
on the same data) satisfies every condition the GPU test puts on the device: the expected info, fp32 pivots that do not depend on the
working precision, the first-maximum rule on the duplicate-row groups, the entrywise backward-error bound and |L| <= 1."""
import numpy as np
import pytest

import _lu_cases as lc


# ---------------------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("case,prec", [(c, p) for c in lc.GETRF + [lc.COLUMN_CASE] for p in c.precs], ids=lambda v: getattr(v, "name", v))
def test_getrf_case_is_listed_under_its_route(case, prec):
    r = lc.getrf_replay(prec, case.m, case.n)
    print(f"{case.name} {prec}: {r.sig}  counters {r.counts}  nbo {r.nbo}  panels (j0, pb, rows, G_reg, route, workgroups): {r.panels}")
    assert r.sig == case.sig
    if case is lc.COLUMN_CASE:
        assert all(p[3] > lc.REG_CAP_MIN for p in r.panels)                   # asserted through counter 7 on the device
        return
    # the route does not depend on the run-time occupancy query: no panel of a listed case comes near the resident capacity
    assert all(p[3] <= 64 or p[3] <= lc.REG_CAP_MIN // 2 for p in r.panels)
    assert lc.getrf_replay(prec, case.m, case.n, reg_cap=4 * lc.REG_CAP_MIN).counts == r.counts
    assert sum(r.counts.get(w, 0) for w in (lc.LDS, lc.FAST, lc.GENERAL)) == len(r.panels) == lc._cdiv(min(case.m, case.n), lc.PB)
    assert (lc.OUTER in r.counts) == ("+outer" in case.sig) == (case.m >= 49152 and case.n >= 256)
    assert (lc.SOLVE in r.counts) <= (lc.OUTER in r.counts)
    if case.zero_col >= 0:
        # the zero column sits in the second panel, and that panel runs on the kernel the case is listed under
        j0, pb, rows, G_reg, route, G = r.panels[1]
        assert j0 <= case.zero_col < j0 + pb and route == case.sig


def test_both_pads_and_both_offsets_are_listed():
    for prec in lc.PRECS:
        for sig in ("lds", "fast", "fast>lds", "general>fast"):
            pads = {pad for c, p, pad in lc.getrf_ids() if p == prec and c.sig == sig and c.zero_col < 0}
            assert pads == {0, 7}, (prec, sig, pads)
        outer = {pad for c, p, pad in lc.getrf_ids() if p == prec and "+outer" in c.sig}
        assert outer == {0, 7}
    assert lc.off_of(0) == 0 and lc.off_of(7) % 4 != 0                       # pad 7: columns and the first element off 16 bytes in fp32


def test_getrf_gates_are_hit_on_both_sides():
    listed = [(c, p) for c in lc.GETRF for p in c.precs]
    panels = {p: [] for p in lc.PRECS}
    for c, p in listed:
        panels[p] += [(q[2], q[4]) for q in lc.getrf_replay(p, c.m, c.n).panels]
    for p in lc.PRECS:
        assert (1023, "lds") in panels[p] and (1024, "fast") in panels[p]
    assert (32768, "fast") in panels["f64"] and (32769, "general") in panels["f64"]
    assert (65536, "fast") in panels["f32"] and (65537, "general") in panels["f32"]
    for p in lc.PRECS:
        shapes = {(c.m, c.n): lc.getrf_replay(p, c.m, c.n).nbo for c, q in listed if q == p}
        assert shapes[(49151, 256)] == 32 and shapes[(49152, 256)] == 128 and shapes[(49152, 255)] == 32
        sigs = {c.sig for c, q in listed if q == p}
        assert {"lds", "fast", "fast>lds", "general>fast"} <= sigs
        zero = {c.sig for c, q in listed if q == p and c.zero_col == 40}
        assert zero == {"lds", "fast", "general"}
    # the kernels under the outer block, the ragged last block and the solve launches
    r = lc.getrf_replay("f64", 49152, 300)
    assert r.counts == {lc.GENERAL: 10, lc.OUTER: 1, lc.SOLVE: 8} and r.panels[-1][1] == 12 and r.right_launches == 2
    assert lc.getrf_replay("f32", 49152, 256).counts == {lc.FAST: 8, lc.OUTER: 1, lc.SOLVE: 4}
    r = lc.getrf_replay("f32", 66000, 256)
    assert r.counts == {lc.GENERAL: 8, lc.OUTER: 1, lc.SOLVE: 4}                 # 66000 - 224 = 65776 rows in the last panel
    # route changes inside one call
    assert lc.getrf_replay("f64", 1040, 64).counts == {lc.FAST: 1, lc.LDS: 1}
    assert lc.getrf_replay("f64", 1100, 1300).counts == {lc.FAST: 3, lc.LDS: 32} and lc.getrf_replay("f64", 1100, 1300).one_panel
    assert lc.getrf_replay("f64", 32790, 64).counts == {lc.GENERAL: 1, lc.FAST: 1}
    assert lc.getrf_replay("f32", 65560, 64).counts == {lc.GENERAL: 1, lc.FAST: 1}
    # the resident capacity: the parameter of the replay
    assert lc.getrf_replay("f32", 300000, 40, reg_cap=256).counts == {lc.COLUMN: 2}
    assert lc.getrf_replay("f32", 300000, 40, reg_cap=512).counts == {lc.GENERAL: 2}


def test_luqrcp_routes_and_gate():
    for (sd, cols), route in lc.LUQRCP_ROUTE.items():
        assert lc.luqrcp_replay(sd, cols) == {lc.WALK if route == "walk" else lc.SERIAL: 1}
    assert set(lc.LUQRCP_SHAPES) == set(lc.LUQRCP_ROUTE)
    mins = {min(s) for s in lc.LUQRCP_SHAPES}
    assert {2048, 2049} <= mins
    assert lc.luqrcp_replay(5, 0) == {}


# ---------------------------------------------------------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("case,prec", [(c, p) for c in lc.GETRF + [lc.COLUMN_CASE] for p in c.precs], ids=lambda v: getattr(v, "name", v))
def test_reference_satisfies_every_condition(case, prec):
    A = lc.getrf_input(case, prec)
    m, n = A.shape
    assert A.dtype == lc.NPDT[prec]
    groups = case.groups(prec)
    for g in groups:                                                          # exact duplicates up to sign
        for r, s in zip(g.rows, g.signs):
            assert np.array_equal(A[r], s * A[g.rows[0]])
        assert len(set(g.signs)) == 2
    lu, piv, info = lc.lapack_getrf(A, prec)
    assert info == (case.zero_col + 1 if case.zero_col >= 0 else 0)
    if case.zero_col >= 0:
        where = lc.positions_after(piv, m, case.zero_col)
        assert np.all(A[:, case.zero_col] == 0) and np.signbit(A[where[case.zero_col], case.zero_col])
        assert np.count_nonzero(np.signbit(A[:, case.zero_col])) == 1
    if prec == "f32":                                                        # condition of check 1
        _, piv64, info64 = lc.lapack_getrf(A.astype(np.float64), "f64")
        assert np.array_equal(piv, piv64) and info == info64
    bad = lc.first_maximum_violations(m, piv, groups)
    assert not bad, bad
    # every group takes part in a pivot decision while all its members still tie
    where = lc.positions_after(piv, m)
    for g in groups:
        first = min(int(np.flatnonzero(where == r)[0]) for r in g.rows)
        assert first < min(m, n), f"group of column {g.col} never wins"
    ratio, lmax = lc.backward_ratio(A, lu, piv, prec)
    print(f"{case.name} {prec}: {lc.getrf_replay(prec, m, n).sig}; LAPACK: residual / bound {ratio:.3f}, max |L| {lmax:.6f}, groups {groups}")
    assert ratio <= 1.0
    assert lmax <= 1.0


def test_first_maximum_check_sees_a_wrong_tie():
    """the check of the pivot order must fail when a later member of a group is chosen"""
    case = next(c for c in lc.GETRF if (c.m, c.n) == (1025, 33))
    A = lc.getrf_input(case, "f64")
    groups = case.groups("f64")
    _, piv, _ = lc.lapack_getrf(A, "f64")
    assert piv[0] == groups[0].rows[0]
    wrong = piv.copy()
    wrong[0] = groups[0].rows[1]
    assert lc.first_maximum_violations(case.m, wrong, groups)


# ---------------------------------------------------------------------------------------------------------------- laswp
def _net_moved(k1, k2, ip, q0, cnt):
    """rows whose content changes under the interchanges q0 .. q0 + cnt - 1 (one launch of the kernel)"""
    rows = np.arange(lc.LASWP_ROWS)
    for i in range(q0, q0 + cnt):
        p = int(ip[i]) - 1
        rows[i], rows[p] = rows[p], rows[i]
    return int(np.count_nonzero(rows != np.arange(lc.LASWP_ROWS)))


def test_laswp_patterns_are_what_they_claim():
    assert np.array_equal(lc.laswp_ipiv("identity", 1, 100), np.arange(1, 101))
    assert _net_moved(1, 32, lc.laswp_ipiv("distinct_far", 1, 32), 0, 32) == 64            # every lane of the composing wave holds a moved row
    assert _net_moved(1, 32, lc.laswp_ipiv("same_far", 1, 32), 0, 32) == 33
    assert _net_moved(1, 32, lc.laswp_ipiv("rotate", 1, 32), 0, 32) == 34
    ip = lc.laswp_ipiv("far_again", 1, 32)
    assert np.count_nonzero(ip[:32] == 131) == 11 and np.count_nonzero(ip[:32] == np.arange(1, 33)) == 11
    for pattern in lc.LASWP_PATTERNS:
        for k1, k2 in lc.LASWP_RANGES:
            ip = lc.laswp_ipiv(pattern, k1, k2)
            M = lc.laswp_matrix(5, "f32")
            out = lc.laswp_reference(M, k1, k2, ip)
            assert sorted(out[:, 0]) == sorted(M[:, 0])
            if pattern == "identity" or k2 < k1:
                assert np.array_equal(out, M)
    assert 70000 > 4 * 16384 and lc.laswp_matrix(70000, "f32").max() < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------- luqrcp_piv
def test_hash_restatement():
    for a in (0, 1, 2048, 65535, 399999, 2 ** 31 - 1):
        assert int(lc.lq_hash(a)) == ((a * 2654435761) % 2 ** 32) >> 20
    assert int(lc.lq_hash(np.array([5, 7]))[1]) == ((7 * 2654435761) % 2 ** 32) >> 20


def test_adversarial_pivots_reach_the_chain_and_the_wrap():
    sd, cols, ip = lc.luqrcp_adversarial("chain")
    assert lc.luqrcp_replay(sd, cols) == {lc.WALK: 1}
    far = ip[ip > sd] - 1
    assert len(set(far)) >= 40 and len(set(lc.lq_hash(far).tolist())) == 1
    longest, wraps, deep = lc.lds_walk_probes(sd, cols, ip)
    print("chain: longest probe", longest, "wraps", wraps, "keys found 40 or more deep", deep)
    assert longest >= 40 and deep >= 8
    sd, cols, ip = lc.luqrcp_adversarial("wrap")
    assert lc.luqrcp_replay(sd, cols) == {lc.WALK: 1}
    far = ip[ip > sd] - 1
    assert {4094, 4095, 0} == set(lc.lq_hash(far).tolist())
    longest, wraps, deep = lc.lds_walk_probes(sd, cols, ip)
    print("wrap: longest probe", longest, "wraps", wraps)
    assert wraps >= 4 and longest >= 6
    assert np.all(ip >= np.arange(1, sd + 1)) and ip.max() <= cols
