"""CPU half of test_gpu_chol.py: the route replay of tests/_chol_cases.py agrees with the constants of chol.hip and lands every listed size
on the edge the table states; the conditions of family E hold for every listed n; and a plain NumPy right-looking Cholesky in the
precision under test meets, by a wide margin, every limit the device is held to: family E bit for bit in fp32 (and within tol_E in fp64),
family R's entrywise ratio <= 1, family F's info, leading rows and pivot entry.  The reference alone therefore stays inside every asserted
limit."""
import re
from pathlib import Path

import numpy as np
import pytest

import _chol_cases as cc

CHOL_HIP = Path(__file__).resolve().parent.parent / "randlapack_amd" / "csrc" / "chol.hip"
NS = sorted(cc.SIZES)


# ---------------------------------------------------------------------------------------------------------------- routes
def test_route_constants_are_those_of_chol_hip():
    src = CHOL_HIP.read_text()

    def const(name):
        m = re.findall(rf"constexpr\s+(?:int|int64_t)\s+{name}\s*=\s*(\d+)\s*;", src)
        assert len(set(m)) == 1, (name, m)
        return int(m[0])

    assert (const("PS_MAXN"), const("BS"), const("NB")) == (cc.PS_MAXN, cc.BS, cc.NB) == (448, 256, 32)
    assert "if (n <= PS_MAXN)" in src and "if (n <= 0 || n > PS_MAXN || lda < n) return 1;" in src
    assert cc.CHOLQRQ_K <= cc.PS_MAXN                                            # potrf_upper_enqueue serves the CholQR Gram matrix


def test_every_listed_size_hits_the_edge_it_is_listed_for():
    r = {n: cc.route(n) for n in NS}
    for n in NS:
        print(f"n = {n:4d} ({cc.SIZES[n]}): {r[n].kind} {r[n].steps}; panels of the last block {r[n].blocks[-1][3][-3:]}")
    assert all(r[n].kind == "small" for n in NS if n <= 448) and all(r[n].kind == "two-level" for n in NS if n > 448)
    assert all(sum(jb for _, jb, _ in r[n].steps) == n for n in NS)
    assert r[31].blocks[0][3] == ((31, 0),) and r[32].blocks[0][3] == ((32, 0),) and r[33].blocks[0][3] == ((32, 1), (1, 0))
    assert r[47].blocks[0][3] == ((32, 15), (15, 0)) and cc.padded_columns(15) == 1 and cc.padded_columns(1) == 15
    assert r[48].blocks[0][3][0] == (32, 16) and cc.padded_columns(16) == 0
    assert r[49].blocks[0][3][0] == (32, 17) and cc.padded_columns(17) == 15
    assert r[64].blocks[0][3] == ((32, 32), (32, 0)) and r[65].blocks[0][3] == ((32, 33), (32, 1), (1, 0))
    assert r[255].blocks[0][3][-1] == (31, 0) and r[256].blocks[0][3][-1] == (32, 0) and r[257].blocks[0][3][-1] == (1, 0)
    assert len(r[448].blocks[0][3]) == 14 and r[448].blocks[0][3][0] == (32, 416) and r[447].blocks[0][3][-1] == (31, 0)
    assert r[449].steps == ((0, 256, 193), (256, 193, 0))
    assert r[511].steps[-1] == (256, 255, 0) and r[512].steps[-1] == (256, 256, 0) and r[513].steps == ((0, 256, 257), (256, 256, 1), (512, 1, 0))
    assert r[705].steps == ((0, 256, 449), (256, 256, 193), (512, 193, 0)) and r[705].blocks[-1][3][-1] == (1, 0)     # ragged in both levels
    assert r[768].steps == ((0, 256, 512), (256, 256, 256), (512, 256, 0))
    # the padding of the MFMA tiles: none, one zero column and fifteen are met; and a block row exists only right of a full block
    met = {cc.padded_columns(rest) for n in NS for b in r[n].blocks for _, rest in b[3] if rest}
    assert met == {0, 1, 15}
    assert all(jb == cc.BS for n in NS if n > 448 for _, jb, rest in r[n].steps if rest > 0)


def test_checked_columns():
    assert cc.checked_columns(40, 0) == 32 and cc.checked_columns(40, 31) == 32 and cc.checked_columns(40, 32) == 40
    assert cc.checked_columns(300, 96) == 128 and cc.checked_columns(300, 255) == 256 and cc.checked_columns(300, 299) == 300
    assert cc.checked_columns(449, 448) == 449 and cc.checked_columns(449, 255) == 256 and cc.checked_columns(449, 256) == 288
    assert cc.checked_columns(705, 2) == 32 and cc.checked_columns(705, 511) == 512 and cc.checked_columns(705, 704) == 705
    for n, ps in cc.F_POSITIONS.items():
        assert n in (40, 300) or n in cc.SIZES
        assert all(1 <= p <= n and p <= cc.checked_columns(n, p - 1) <= n for p in ps)
    (n, pos, kind), small, two = cc.REPEAT
    assert pos in cc.F_POSITIONS[n] and kind in cc.F_KINDS and cc.route(n).kind == "two-level"
    assert cc.route(small).kind == "small" and cc.route(two).kind == "two-level" and {small, two} <= set(cc.SIZES)


# ---------------------------------------------------------------------------------------------------------------- family E
@pytest.mark.parametrize("n", NS + [40, 300])
def test_family_e_conditions(n):
    e = cc.family_e(n)
    print(f"n = {n}: level {cc.E_LEVEL.get(n, 0)}, kappa_2(U) = {e.kappa_u:.3g}, kappa_2(A) eps = {e.kappa_eps:.3g}, tol_E = {e.tol:.3g}, "
          f"max |A| = {np.abs(e.A).max():g}")
    assert cc.conditions_hold(e)
    assert e.kappa_eps <= 0.5 and e.tol <= 2.0 ** -6 and np.abs(e.A).max() < 2 ** 24          # the conditions, spelled out
    for lower in range(cc.E_LEVEL.get(n, 0)):                                                  # thinned only where it has to be
        assert not cc.conditions_hold(cc.family_e(n, lower))
    U, A = e.U, e.A
    assert np.array_equal(U, np.rint(U)) and np.array_equal(U, np.triu(U)) and np.array_equal(A, A.T)
    d = np.diag(U)
    assert set(d) <= {1.0, 2.0, 4.0} and np.count_nonzero(np.triu(U, 1), axis=0).max(initial=0) <= 3
    assert np.abs(np.triu(U, 1)).max(initial=0) <= 2 and np.abs(A).max() <= 28
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A)                          # exact in fp32
    k = n // 2                                                                                  # a Schur complement is of the same kind
    S = A[k:, k:] - U[:k, k:].T @ U[:k, k:]
    assert np.array_equal(S, U[k:, k:].T @ U[k:, k:]) and np.abs(S).max() <= 28
    for prec in cc.PRECS:
        st = cc.stored(A, prec)
        low = np.tri(n, k=-1, dtype=bool)
        assert st.dtype == cc.NPDT[prec] and np.all(st.view(cc.UINT[prec])[low] == cc.POISON[prec]) and np.array_equal(st[~low], A[~low])


@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n", NS)
def test_plain_cholesky_returns_u_on_family_e(n, prec):
    e = cc.family_e(n)
    R, info = cc.potrf_plain(cc.stored(e.A, prec), prec)
    assert info == 0 and R.dtype == cc.NPDT[prec]
    differ = int(np.count_nonzero(R.astype(np.float64) != e.U))
    print(f"n = {n} {prec}: {differ} entries are not U; max |R - U| = {np.abs(R - e.U).max():.3g} (tol_E = {e.tol:.3g})")
    if prec == "f32":
        assert np.array_equal(R.view(np.uint32), e.U.astype(np.float32).view(np.uint32))
    assert np.abs(R - e.U).max() <= e.tol
    # one integer of A off by one is seen: some entry of the factor moves by 1 / 4 and more, far above tol_E
    if n >= 2:
        A = e.A.copy()
        A[n // 3, n - 1] += 1.0
        A[n - 1, n // 3] += 1.0
        Rw, _ = cc.potrf_plain(A, "f64")
        with np.errstate(invalid="ignore"):
            assert not np.abs(Rw - e.U).max() <= 0.25 - e.tol


# ---------------------------------------------------------------------------------------------------------------- family R
@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n", NS)
def test_plain_cholesky_stays_within_the_bound_on_family_r(n, prec):
    A = cc.family_r(n, prec)
    assert np.array_equal(A, A.T) and np.array_equal(A.astype(cc.NPDT[prec]).astype(np.float64), A)
    R, info = cc.potrf_plain(cc.stored(A, prec), prec)
    ratio = cc.residual_ratio(A, R, prec)
    print(f"n = {n} {prec} {cc.route(n).kind}: plain Cholesky residual / bound {ratio:.3g}")
    assert info == 0 and (np.diag(R) > 0).all()
    assert ratio <= 1.0
    # the bound is not vacuous: the largest entry of a middle column off by 1e-9 (fp64) / 1e-2 (fp32) relative is seen
    if n >= 2:
        Rw = R.astype(np.float64)
        j = n // 2
        Rw[np.argmax(np.abs(Rw[:j + 1, j])), j] *= 1 + (1e-9 if prec == "f64" else 1e-2)
        assert cc.residual_ratio(A, Rw, prec) > 1.0


# ---------------------------------------------------------------------------------------------------------------- family F
@pytest.mark.parametrize("prec", cc.PRECS)
@pytest.mark.parametrize("n,pos,kind", cc.f_ids(), ids=lambda v: str(v))
def test_plain_cholesky_reports_the_position_on_family_f(n, pos, kind, prec):
    A, U, tol = cc.family_f(n, pos, kind)
    k = pos - 1
    assert np.array_equal(np.isnan(A), np.isnan(A).T) and np.count_nonzero(np.isnan(A)) == (kind == "nan")
    R, info = cc.potrf_plain(cc.stored(A, prec), prec)
    assert info == pos
    cols = cc.checked_columns(n, k)
    assert pos <= cols <= n
    if prec == "f32":
        assert np.array_equal(R[:k, :cols], np.triu(U)[:k, :cols].astype(np.float32))
    else:
        assert np.abs(R[:k, :cols] - np.triu(U)[:k, :cols]).max(initial=0) <= tol
    if kind == "neg":
        assert R[k, k] == -1.0                                                  # exact here; the device is held to <= 0
    elif kind == "nan":
        assert np.isnan(R[k, k])
    else:
        assert R[k, k] == 0.0 and not R[:k, k].any()
