"""Device block / lockstep PCG, the spectral preconditioner and KRILL (randlapack_amd/csrc/pcg.hip, include/RandLAPACK_amd/rl_determiter.hh,
rl_krill.hh) in fp64 and fp32: the four kernels on their own (exactly where the inputs allow it), the solver step by step against the numpy
model (tests/_pcg_model.py), convergence by the reference's own check (test/drivers/test_krill.cc:60-65), the edges, and the KRILL driver."""
import functools

import numpy as np
import pytest

import _pcg_model as pm

pytestmark = pytest.mark.gpu

DT = {"f64": np.float64, "f32": np.float32}


def _t(a, T):
    """(m, n) numpy -> column-major device tensor (n, m) of dtype T"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=T).T)).to("cuda:0")


def _np(t):
    return t.detach().cpu().numpy().T.copy()


# ---------------------------------------------------------------------------------------------------
# 1. posm_square
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("diag_only", [False, True])
@pytest.mark.parametrize("s", [1, 3, 8, 33, 64, 65])
def test_posm_square_exact_on_powers_of_four(ctx, s, diag_only, prec):
    """LHS = diag(4^j): sqrt, the two divisions and every product with a zero are exact, so the result is RHS / 4^j bit for bit
    (s = 65 takes the composed route)"""
    from randlapack_amd import device as dev

    T = DT[prec]
    d = 4.0 ** (np.arange(s) % 6)
    B = np.random.default_rng(s).integers(-3, 4, size=(s, s)).astype(T)
    L, R = _t(np.diag(d), T), _t(B, T)
    assert dev.posm_square(ctx, L, R, diag_only=diag_only) == s
    want = (np.diag(np.diag(B)) if diag_only else B) / d[:, None].astype(T)
    got = _np(R)
    assert np.array_equal(got, want.astype(T))
    assert not np.any(np.signbit(got[want == 0]))
    assert np.array_equal(_np(L), np.diag(d).astype(T))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("s", [1, 3, 8, 33, 64, 65])
def test_posm_square_tridiagonal(ctx, s, prec):
    """tridiag(-1, 4, -1): condition number below 3, so a backward-stable solve is within a small multiple of s eps of the solution"""
    from randlapack_amd import device as dev

    T = DT[prec]
    A = 4.0 * np.eye(s) - np.eye(s, k=1) - np.eye(s, k=-1)
    B = np.random.default_rng(100 + s).integers(-3, 4, size=(s, s)).astype(np.float64)
    R = _t(B, T)
    Lh = np.tril(A) + np.triu(np.full((s, s), 77.0), 1)              # the strictly upper triangle is never read
    assert dev.posm_square(ctx, _t(Lh, T), R) == s
    ref = np.linalg.solve(A, B)
    err = np.max(np.abs(_np(R) - ref))
    print(f"s={s} {prec}: err={err:.3g} bound={100 * s * np.finfo(T).eps * max(1.0, np.max(np.abs(ref))):.3g}")
    assert err <= 100 * s * np.finfo(T).eps * max(1.0, np.max(np.abs(ref)))


def _failing():
    sing = np.eye(5)
    sing[:2, :2] = 1.0
    return {"singular": (sing, 4), "indefinite": (np.diag([1.0, -1.0]), -3), "zero": (np.zeros((4, 4)), -6)}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["singular", "indefinite", "zero"])
def test_posm_square_failure_path(ctx, name, prec):
    """the device attempt reports -1 and writes nothing; the C++ posm_square then returns the reference's rank / codes from the host fallback"""
    from randlapack_amd import device as dev

    T = DT[prec]
    A, want = _failing()[name]
    s = A.shape[0]
    B = np.random.default_rng(5).integers(-3, 4, size=(s, s)).astype(np.float64)
    L, R = _t(A, T), _t(B, T)
    assert dev.posm_square(ctx, L, R) == -1
    assert np.array_equal(_np(L), A.astype(T)) and np.array_equal(_np(R), B.astype(T))
    assert dev.posm_square(ctx, L, R, host_fallback=True) == want
    assert np.array_equal(_np(L), A.astype(T))
    if want < 0:
        assert np.array_equal(_np(R), B.astype(T))
    else:
        ref = np.linalg.pinv(A) @ B
        assert np.max(np.abs(_np(R) - ref)) <= 100 * s * np.finfo(T).eps * max(1.0, np.max(np.abs(ref)))
    # a NaN pivot fails as a non-positive one does
    An = np.eye(3)
    An[1, 1] = np.nan
    assert dev.posm_square(ctx, _t(An, T), _t(np.eye(3), T)) == -1


# ---------------------------------------------------------------------------------------------------
# 2. the update kernels, exactly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("s", [1, 3, 8, 33, 64, 100])
def test_update_kernels_exact(ctx, s, prec):
    """small integers: every product and sum is exact in either precision (|entries| <= 3 + 6 s < 2^24), whatever the order of summation"""
    import torch

    from randlapack_amd import device as dev

    T = DT[prec]
    for n in (1, 63, 64, 65, 300, 4099):
        rng = np.random.default_rng(1000 * s + n)
        ld = n + 5
        blocks = {}
        for name in ("P", "GP", "X", "R", "NR"):
            full = np.full((ld, s), 99.0)
            full[:n] = rng.integers(-3, 4, size=(n, s))
            blocks[name] = full
        alpha = rng.integers(-2, 3, size=(s, s)).astype(np.float64)
        beta = rng.integers(-2, 3, size=(s, s)).astype(np.float64)
        d = {k: _t(v, T) for k, v in blocks.items()}
        before = [ctx.pcg_path_count(i) for i in (43, 44, 45)]
        cn = dev.pcg_update_xr(ctx, n, s, _t(alpha, T), d["P"], d["GP"], d["X"], d["R"])
        Xw = blocks["X"][:n] + blocks["P"][:n] @ alpha
        Rw = blocks["R"][:n] - blocks["GP"][:n] @ alpha
        for name, want in (("X", Xw), ("R", Rw)):
            got = _np(d[name])
            assert np.array_equal(got[:n], want.astype(T)), (name, n)
            assert np.all(got[n:] == 99.0), (name, n)
        assert cn.dtype == torch.float64 and np.array_equal(cn.cpu().numpy(), np.sum(Rw * Rw, axis=0)), n
        for name in ("P", "GP"):
            assert np.array_equal(_np(d[name]), blocks[name].astype(T)), (name, n)
        # without the norms: the same X and R
        d2 = {k: _t(v, T) for k, v in blocks.items()}
        assert dev.pcg_update_xr(ctx, n, s, _t(alpha, T), d2["P"], d2["GP"], d2["X"], d2["R"], want_norms=False) is None
        assert torch.equal(d2["X"], d["X"]) and torch.equal(d2["R"], d["R"])
        dev.pcg_update_p(ctx, n, s, _t(beta, T), d["NR"], d["P"])
        got = _np(d["P"])
        assert np.array_equal(got[:n], (blocks["NR"][:n] + blocks["P"][:n] @ beta).astype(T)), n
        assert np.all(got[n:] == 99.0), n
        assert np.array_equal(_np(d["NR"]), blocks["NR"].astype(T)), n
        moved = [ctx.pcg_path_count(i) - b for i, b in zip((43, 44, 45), before)]
        assert moved == ([2, 1, 0] if s <= 64 else [0, 0, 3]), (n, moved)
    assert ctx.pcg_path_count(42) == -1 and ctx.pcg_path_count(46) == -1


# ---------------------------------------------------------------------------------------------------
# 3. the preconditioner against numpy
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 2.0)])
@pytest.mark.parametrize("num_ops", [1, 3])
def test_spectral_precond_apply(ctx, num_ops, alpha, beta, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    dim, dim_pre, n = 333, 64, 3
    rng = np.random.default_rng(17)
    V = np.linalg.qr(rng.standard_normal((dim, dim_pre)))[0].astype(T).astype(np.float64)
    ev = np.sort(rng.random(dim_pre) + 0.05)[::-1]
    mus = (1e-2, 1e-1, 1.0)[:num_ops]
    D = np.stack([(ev[-1] + mu) / (ev + mu) - 1.0 for mu in mus], axis=1).astype(T).astype(np.float64)
    ldb, ldc = dim + 3, dim + 8
    Bf, Cf = np.full((ldb, n), np.nan), np.full((ldc, n), 55.0)
    Bf[:dim] = rng.standard_normal((dim, n))
    Cf[:dim] = rng.standard_normal((dim, n))
    if beta == 0.0:
        Cf[:dim] = np.nan                                              # beta == 0 must not read C
    Bf, Cf = Bf.astype(T).astype(np.float64), Cf.astype(T).astype(np.float64)
    Cd = _t(Cf, T)
    got, cn = dev.spectral_precond_apply(ctx, _t(V, T), _t(D, T), _t(Bf, T), dim, n, alpha=alpha, beta=beta, C_=Cd)
    B = Bf[:dim]
    W = (V.T @ B) * (D if num_ops != 1 else D[:, :1])
    want = alpha * (B + V @ W) + (beta * Cf[:dim] if beta != 0.0 else 0.0)
    tol = 1e-11 if T is np.float64 else 2e-4
    out = _np(got)
    np.testing.assert_allclose(out[:dim], want, atol=tol, rtol=tol)
    assert np.all(out[dim:] == 55.0)
    np.testing.assert_allclose(cn.cpu().numpy(), np.sum(want * want, axis=0), atol=tol, rtol=tol)
    # the norms are those of the block it wrote, bit for bit in double
    o64 = out[:dim].astype(np.float64)
    np.testing.assert_allclose(cn.cpu().numpy(), np.sum(o64 * o64, axis=0), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------
# 4.-6. the solver
# ---------------------------------------------------------------------------------------------------
CASES = ("dense300", "rbf333", "rbf1037")


@functools.lru_cache(maxsize=None)
def _case(name):
    c = {"dense300": lambda: pm.dense_case(), "rbf333": lambda: pm.rbf_case(333, 64), "rbf1037": lambda: pm.rbf_case(1037, 100)}[name]()
    c["V"], c["ev"] = pm.top_eigs(c["K"], c["k"])
    return c


def _device_pcg(ctx, c, mus, T, H, X0, tol, max_iters):
    """the device solver on case c: dense through rlhip_drv_pcg_dense_*, RBF through rlhip_drv_pcg_rbf_* (the kernel matrix is formed on the device)"""
    import torch

    from randlapack_amd import device as dev

    s = H.shape[1]
    V, ev = _t(c["V"], T), torch.from_numpy(c["ev"].astype(T)).to("cuda:0")
    Hd, Xd = _t(H, T), _t(X0, T)
    if c["kind"] == "dense":
        r = dev.pcg_dense(ctx, _t(c["K"], T), c["n"], list(mus), V, ev, Hd, Xd, s, tol, max_iters)
    else:
        r = dev.pcg_rbf(ctx, _t(c["pts"], T), c["pts"].shape[0], c["n"], c["h"], list(mus), V, ev, Hd, Xd, s, tol, max_iters)
    r["X"] = _np(r["X"])
    return r


def _problem(c, mode, s, T):
    mus = pm.mode_mus(c, mode)
    G = pm.reg_op(c["K"], mus, T)
    Xstar = np.random.default_rng(101).standard_normal((c["n"], s)).astype(T)
    return mus, G, Xstar, G(Xstar)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), np.finfo(np.float64).tiny))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", pm.MODES)
@pytest.mark.parametrize("name", CASES)
def test_three_steps_match_the_model(ctx, name, mode, s, prec):
    """tol = 0, three iterations: X and both norm histories against the model in the same precision.  The allowance is measured, not chosen:
    the model run again on the symmetrically permuted problem differs from itself by rounding alone, and the device's order of summation
    differs from the model's at least as much as a permutation does; 100 times that difference, never less than 1000 eps."""
    T = DT[prec]
    c = _case(name)
    mus, G, Xstar, H = _problem(c, mode, s, T)
    X0 = np.zeros_like(H)
    N = pm.SpectralPrecond(c["V"], c["ev"], mus, T)
    Xm, itm, nRm, nNRm = pm.pcg(G, H, 0.0, 3, N, X0, T)
    perm = np.random.default_rng(5).permutation(c["n"])
    Gp = pm.reg_op(c["K"][np.ix_(perm, perm)], mus, T)
    Np = pm.SpectralPrecond(c["V"][perm], c["ev"], mus, T)
    Xp, _, nRp, nNRp = pm.pcg(Gp, H[perm], 0.0, 3, Np, X0, T)
    Xp_back = np.empty_like(Xp)
    Xp_back[perm] = Xp
    self_diff = max(_rel(Xm, Xp_back), _rel(nRm, nRp), _rel(nNRm, nNRp))
    allowed = max(100.0 * self_diff, 1000.0 * float(np.finfo(T).eps))
    r = _device_pcg(ctx, c, mus, T, H, X0, 0.0, 3)
    dX, dR, dNR = _rel(Xm, r["X"]), _rel(nRm, r["normR"]), _rel(nNRm, r["normNR"])
    print(f"{name} {mode} s={s} {prec}: model self-difference {self_diff:.3g}, allowed {allowed:.3g}; device X {dX:.3g} normR {dR:.3g} normNR {dNR:.3g}")
    assert r["iters"] == itm == 3 and r["normR"].size == 4 and r["normNR"].size == 4
    assert dX <= allowed and dR <= allowed and dNR <= allowed


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", pm.MODES)
@pytest.mark.parametrize("name", CASES)
def test_convergence_by_the_reference_check(ctx, name, mode, s, prec):
    T = DT[prec]
    c = _case(name)
    mus, G, Xstar, H = _problem(c, mode, s, T)
    tol = 100 * float(np.finfo(T).eps)
    r = _device_pcg(ctx, c, mus, T, H, np.zeros_like(H), tol, 30)
    ratio = pm.reference_check(r["X"], Xstar, T)
    print(f"{name} {mode} s={s} {prec}: iters={r['iters']} error/allowed={ratio:.3g} last normNR={r['normNR'][-1]:.3g}")
    assert ratio <= 1.0
    assert r["iters"] <= 30 and r["normNR"].size == r["iters"] + 1
    assert r["normNR"][-1] < tol * (1.0 + r["normNR"][0])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", [("lockstep", 3), ("block", 8)])
def test_solver_edges(ctx, mode, s, prec):
    from randlapack_amd import _lib

    T = DT[prec]
    c = _case("rbf333")
    mus, G, Xstar, H = _problem(c, mode, s, T)
    Z = np.zeros_like(H)
    # H = 0, X0 = 0: P = 0, P^T G P = 0 fails on the device, the host fallback answers -(s + 2), the loop breaks in its first iteration
    r = _device_pcg(ctx, c, mus, T, Z, Z, 100 * float(np.finfo(T).eps), 30)
    assert r["iters"] == 1 and np.array_equal(r["X"], Z) and not np.any(np.signbit(r["X"]))
    assert r["normR"].tolist() == [0.0] and r["normNR"].tolist() == [0.0]
    # tol = 1: normNR < 1 + normNR0 after the first step
    r = _device_pcg(ctx, c, mus, T, H, Z, 1.0, 30)
    assert r["iters"] == 1 and r["normNR"].size == 2
    # the same call twice: the same bits
    a = _device_pcg(ctx, c, mus, T, H, Z, 0.0, 4)
    b = _device_pcg(ctx, c, mus, T, H, Z, 0.0, 4)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["normR"], b["normR"]) and np.array_equal(a["normNR"], b["normNR"])
    # lockstep needs one regularization parameter per column
    with pytest.raises(_lib.RlhipError):
        _device_pcg(ctx, c, (1e-2, 1e-1), T, H, Z, 0.0, 2)


# ---------------------------------------------------------------------------------------------------
# 7. KRILL
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mode,s", [("lockstep", 3), ("block", 4)])
def test_krill_full_rpchol_rbf(ctx, mode, s, prec):
    from randlapack_amd import device as dev

    T = DT[prec]
    n, rows_x, h, k, blk = 1000, 5, 3.0, 128, 16
    pts = np.random.default_rng(2).standard_normal((rows_x, n)).astype(T).astype(np.float64)
    mus = (1e-2, 1e-1, 1.0) if mode == "lockstep" else (1e-2,)
    G = pm.reg_op(pm.rbf_kernel(pts, h, np.float64), mus, np.float64)
    Xstar = np.random.default_rng(101).standard_normal((n, s)).astype(T)
    H = G(Xstar)
    tol = 100 * float(np.finfo(T).eps)
    Pd = _t(pts, T)
    key = (7, 0)
    r = dev.krill_full_rpchol_rbf(ctx, Pd, rows_x, n, h, list(mus), _t(H, T), _t(np.zeros_like(H), T), s, tol, 40, k=k, b=blk, key=key)
    ratio = pm.reference_check(_np(r["X"]), Xstar, T)
    print(f"krill {mode} s={s} {prec}: k={r['k']} iters={r['iters']} error/allowed={ratio:.3g}")
    assert ratio <= 1.0
    assert r["k"] == k and r["iters"] <= 40
    assert r["normNR"][-1] < tol * (1.0 + r["normNR"][0])
    pc = dev.rpchol_pc_data(ctx, Pd, rows_x, n, h, k, blk, key=key)
    assert r["next_ctr"] == pc["next_ctr"] and pc["k"] == k
