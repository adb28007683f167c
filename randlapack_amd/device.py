"""Thin Python handles over the rlhip C ABI for tests / bench / smoke.

A column-major m x n matrix is held as a torch tensor `t` of shape (n, m), contiguous, so that
element (i, j) is `t[j, i]` and the leading dimension is m.  `cm_from_numpy` / `cm_to_numpy` convert
from/to ordinary (m, n) numpy arrays.  Nothing in here computes: it forwards pointers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_TORCH_DT = None


def _torch():
    import torch

    return torch


def _suffix(t):
    torch = _torch()
    if t.dtype == torch.float64:
        return "f64", C.c_double
    if t.dtype == torch.float32:
        return "f32", C.c_float
    raise TypeError(f"unsupported dtype {t.dtype}")


def cm_from_numpy(a: np.ndarray, device="cuda:0"):
    """(m, n) numpy -> column-major device tensor of shape (n, m)."""
    torch = _torch()
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(device)


def cm_to_numpy(t) -> np.ndarray:
    """column-major device tensor (n, m) -> (m, n) numpy."""
    return t.detach().cpu().numpy().T.copy()


def cm_empty(m: int, n: int, dtype=None, device="cuda:0"):
    torch = _torch()
    return torch.empty((n, m), dtype=dtype or torch.float64, device=device)


def cm_zeros(m: int, n: int, dtype=None, device="cuda:0"):
    torch = _torch()
    return torch.zeros((n, m), dtype=dtype or torch.float64, device=device)


class Context:
    """One rlhip context bound to torch's CURRENT HIP stream on `device` (so torch.cuda.Event timing and
    torch allocations are ordered with the kernels)."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("randlapack_amd needs a HIP device (torch.cuda.is_available() is False)")
        self.lib = _lib.load()
        self.device = device
        torch.cuda.set_device(device)
        stream = torch.cuda.current_stream(device).cuda_stream if use_torch_stream else 0
        h = C.c_void_p()
        _lib.check(self.lib.rlhip_create(C.byref(h), device, C.c_void_p(stream), 0 if use_torch_stream else 1),
                   "rlhip_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.rlhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _lib.check(self.lib.rlhip_sync(self.h), "rlhip_sync")

    # ---- timing on the context stream
    def timer_start(self):
        _lib.check(self.lib.rlhip_timer_start(self.h), "timer_start")

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        _lib.check(self.lib.rlhip_timer_stop_ms(self.h, C.byref(ms)), "timer_stop")
        return float(ms.value)

    def reserve_workspace(self, nbytes: int):
        _lib.check(self.lib.rlhip_reserve_workspace(self.h, nbytes), "reserve_workspace")

    # ---- RNG
    @staticmethod
    def _u32(vals):
        arr = (C.c_uint32 * len(vals))(*[int(v) & 0xFFFFFFFF for v in vals])
        return arr

    def philox(self, nblocks: int, ctr, key):
        torch = _torch()
        out = torch.empty(4 * nblocks, dtype=torch.int32, device=f"cuda:{self.device}")
        _lib.check(
            self.lib.rlhip_philox4x32_10(self.h, nblocks, out.data_ptr(), self._u32(ctr), self._u32(key)), "philox"
        )
        return out.cpu().numpy().view(np.uint32)

    def fill_dense(self, buf, rows: int, cols: int, ctr=(0, 0, 0, 0), key=(0, 0), dist: int = 0):
        suf, _ = _suffix(buf)
        nxt = (C.c_uint32 * 4)()
        fn = getattr(self.lib, f"rlhip_fill_dense_{suf}")
        _lib.check(fn(self.h, dist, rows, cols, buf.data_ptr(), self._u32(ctr), self._u32(key), nxt), "fill_dense")
        return tuple(int(x) for x in nxt)

    # ---- BLAS-3 (column-major tensors, see module docstring)
    def gemm(self, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc):
        suf, T = _suffix(Cm)
        fn = getattr(self.lib, f"rlhip_gemm_{suf}")
        return _lib.check(
            fn(self.h, ta.encode(), tb.encode(), m, n, k, T(alpha), A.data_ptr(), lda, B.data_ptr(), ldb, T(beta),
               Cm.data_ptr(), ldc),
            "gemm",
        )

    def syrk(self, uplo, trans, n, k, alpha, A, lda, beta, Cm, ldc):
        suf, T = _suffix(Cm)
        fn = getattr(self.lib, f"rlhip_syrk_{suf}")
        return _lib.check(
            fn(self.h, uplo.encode(), trans.encode(), n, k, T(alpha), A.data_ptr(), lda, T(beta), Cm.data_ptr(), ldc),
            "syrk",
        )

    def trsm(self, m, n, alpha, A, lda, B, ldb, diag="N"):
        suf, T = _suffix(B)
        fn = getattr(self.lib, f"rlhip_trsm_{suf}")
        return _lib.check(
            fn(self.h, b"R", b"U", b"N", diag.encode(), m, n, T(alpha), A.data_ptr(), lda, B.data_ptr(), ldb), "trsm"
        )

    def trsm_gather(self, m, n, alpha, A, lda, Bsrc, ldsrc, jpvt, B, ldb, diag="N"):
        """B = alpha * Bsrc[:, jpvt - 1] * inv(A), out of place (rlhip_trsm_gather_*); jpvt: device int64 tensor (1-based) or None"""
        suf, T = _suffix(B)
        fn = getattr(self.lib, f"rlhip_trsm_gather_{suf}")
        return _lib.check(
            fn(self.h, diag.encode(), m, n, T(alpha), A.data_ptr(), lda, Bsrc.data_ptr(), ldsrc, jpvt.data_ptr() if jpvt is not None else None,
               B.data_ptr(), ldb), "trsm_gather")

    def trmm(self, m, n, alpha, A, lda, B, ldb, diag="N"):
        suf, T = _suffix(B)
        fn = getattr(self.lib, f"rlhip_trmm_{suf}")
        return _lib.check(
            fn(self.h, b"R", b"U", b"N", diag.encode(), m, n, T(alpha), A.data_ptr(), lda, B.data_ptr(), ldb), "trmm"
        )

    def potrf(self, n, A, lda) -> int:
        suf, _ = _suffix(A)
        fn = getattr(self.lib, f"rlhip_potrf_{suf}")
        return _lib.check(fn(self.h, b"U", n, A.data_ptr(), lda), "potrf")

    def lange_fro(self, m, n, A, lda) -> float:
        suf, T = _suffix(A)
        res = T()
        fn = getattr(self.lib, f"rlhip_lange_fro_{suf}")
        _lib.check(fn(self.h, m, n, A.data_ptr(), lda, C.byref(res)), "lange")
        return float(res.value)

    def lacpy(self, uplo, m, n, A, lda, B, ldb):
        suf, _ = _suffix(A)
        fn = getattr(self.lib, f"rlhip_lacpy_{suf}")
        return _lib.check(fn(self.h, uplo.encode(), m, n, A.data_ptr(), lda, B.data_ptr(), ldb), "lacpy")

    def laset(self, uplo, m, n, offd, diag, A, lda):
        suf, T = _suffix(A)
        fn = getattr(self.lib, f"rlhip_laset_{suf}")
        return _lib.check(fn(self.h, uplo.encode(), m, n, T(offd), T(diag), A.data_ptr(), lda), "laset")

    def gesvdj(self, m, n, A, lda, S, VT, ldvt):
        suf, _ = _suffix(A)
        sweeps = C.c_int()
        fn = getattr(self.lib, f"rlhip_gesvdj_{suf}")
        info = _lib.check(fn(self.h, m, n, A.data_ptr(), lda, S.data_ptr(), VT.data_ptr(), ldvt, C.byref(sweeps)),
                          "gesvdj")
        return info, int(sweeps.value)

    # ---- diagnostics
    def path_count(self, which: int) -> int:
        return int(self.lib.rlhip_path_count(self.h, which))

    def pcg_path_count(self, which: int) -> int:
        """routes of the PCG update kernels: 43 fused update_xr, 44 fused update_p, 45 composed (include/rlhip.h rlhip_pcg_path_count)"""
        return int(self.lib.rlhip_pcg_path_count(self.h, which))

    def lsq_path_count(self, which: int) -> int:
        """routes of the matrix-vector layer: 46 fused normal matvec, 47 composed, 48 gemv 'N', 49 gemv 'T' (include/rlhip.h rlhip_lsq_path_count)"""
        return int(self.lib.rlhip_lsq_path_count(self.h, which))

    def lsq_block_path_count(self, which: int) -> int:
        """routes of the block least-squares layer: 76 one-pass normal matmat, 77 composed, 78 pcg_saddle_block iterations (include/rlhip.h
        rlhip_lsq_block_path_count)"""
        return int(self.lib.rlhip_lsq_block_path_count(self.h, which))

    def normal_matmat_route(self, route: int = 1):
        """context manager: the route of rlhip_normal_matmat_* on this context (rlhip_normal_matmat_set_route): 1 the one-pass kernel where
        the shape allows, 0 always the composed route, -1 the default; the value found is put back"""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            was = int(self.lib.rlhip_normal_matmat_set_route(self.h, int(route)))
            try:
                yield self
            finally:
                self.lib.rlhip_normal_matmat_set_route(self.h, was)
        return _cm()

    def spmv_path_count(self, which: int) -> int:
        """routes of the sparse matrix-vector layer: 50 / 51 / 52 a product with 4 / 16 / 64 lanes per row, 53 the split long-row route,
        54 csr_normal_matvec calls (include/rlhip.h rlhip_spmv_path_count)"""
        return int(self.lib.rlhip_spmv_path_count(self.h, which))

    def rbf_path_count(self, which: int) -> int:
        """routes of the two-point-set RBF kernels: 55 fused cross apply, 56 composed cross apply, 57 sqexp_cross_submatrix calls
        (include/rlhip.h rlhip_rbf_path_count)"""
        return int(self.lib.rlhip_rbf_path_count(self.h, which))

    def rbf_split_count(self) -> int:
        """fused cross applies that ran split over X (options(rbf_fused=2); include/rlhip.h rlhip_rbf_split_count)"""
        return int(self.lib.rlhip_rbf_split_count(self.h))

    def var_path_count(self, which: int) -> int:
        """routes of rlhip_pdk_cross_var_*: 58 fused, 59 composed (include/rlhip.h rlhip_pdk_var_path_count)"""
        return int(self.lib.rlhip_pdk_var_path_count(self.h, which))

    def grad_path_count(self, which: int) -> int:
        """routes of rlhip_pdk_cross_grad_*: 74 fused, 75 composed (include/rlhip.h rlhip_pdk_grad_path_count)"""
        return int(self.lib.rlhip_pdk_grad_path_count(self.h, which))

    def grad_fused(self, on: bool = True):
        """context manager: rlhip_pdk_cross_grad_* on this context takes its fused kernel where the shape allows (rlhip_pdk_grad_set_fused);
        the value found is put back"""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            was = int(self.lib.rlhip_pdk_grad_set_fused(self.h, int(bool(on))))
            try:
                yield self
            finally:
                self.lib.rlhip_pdk_grad_set_fused(self.h, was)
        return _cm()

    def lu_path_count(self, which: int) -> int:
        """routes of the LU layer: a panel on 60 the LDS kernel, 61 the fast step, 62 the general register kernel; 63 getrf calls with an
        outer block wider than a panel, 64 unit_lower_solve_kernel launches; luqrcp_piv on 65 the LDS walk, 66 the serial kernel
        (include/rlhip.h rlhip_lu_path_count)"""
        return int(self.lib.rlhip_lu_path_count(self.h, which))

    def tri_path_count(self, which: int) -> int:
        """routes of the triangular layer: a 256-block of trsm on 67 the per-block MFMA kernel, 68 its two-row-tile form; 69 a fused launch
        with twelve wavefronts; 70 a fused out-of-place solve on the identity twin; 71 trsm_gather by gather-copy + the in-place solver;
        72 trmm side Right, 73 side Left (include/rlhip.h rlhip_tri_path_count)"""
        return int(self.lib.rlhip_tri_path_count(self.h, which))

    def var_fused(self, on: bool = True):
        """context manager: rlhip_pdk_cross_var_* on this context takes its fused kernel where the shape allows (rlhip_pdk_var_set_fused);
        the value found is put back"""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            was = int(self.lib.rlhip_pdk_var_set_fused(self.h, int(bool(on))))
            try:
                yield self
            finally:
                self.lib.rlhip_pdk_var_set_fused(self.h, was)
        return _cm()

    # ---- options (include/rlhip.h: enum rlhip_option; -1 restores the default)
    OPT = dict(cholqrq_one_stream=0, gesdd_gram=1, jacobi_persist=2, trsm_xasm=3, saso_mode=4, hqrrp_tall_panel=5,
               bqrrp_lookahead_min_elems=6, bqrrp_cholqr_fallback=7, cqrrpt_fold_pivoting=8, cqrrpt_split_qrcp=9, sparse_sketch_densify=10, jacobi_clock_holders=11,
               lsq_normal_fused=12, spmv_lanes=13, rbf_fused=14)

    def set_option(self, name: str, value: int) -> None:
        _lib.check(self.lib.rlhip_set_option(self.h, self.OPT[name], int(value)), "set_option")

    def get_option(self, name: str) -> int:
        return int(self.lib.rlhip_get_option(self.h, self.OPT[name]))

    def options(self, **kw):
        """context manager: set options for the duration of a block, then restore what was there"""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            old = {k: self.get_option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return _cm()

    def gemm_norma(self, ta, tb, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc):
        """gemm + ||A||_F in one pass (rlhip_gemm_norma_f64); returns (norm, fused flag)"""
        nrm, fused = C.c_double(), C.c_int()
        _lib.check(self.lib.rlhip_gemm_norma_f64(self.h, ta.encode(), tb.encode(), m, n, k, alpha, A.data_ptr(), lda, B.data_ptr(), ldb,
                                                 beta, Cm.data_ptr(), ldc, C.byref(nrm), C.byref(fused)), "gemm_norma")
        return float(nrm.value), int(fused.value)

    def mfma_peak(self, is_f64=True, iters=20000) -> float:
        tf = C.c_double()
        _lib.check(self.lib.rlhip_mfma_peak(self.h, 1 if is_f64 else 0, iters, C.byref(tf)), "mfma_peak")
        return float(tf.value)

    def hbm_read_peak(self, buf) -> float:
        g = C.c_double()
        nbytes = buf.numel() * buf.element_size()
        _lib.check(self.lib.rlhip_hbm_read_peak(self.h, buf.data_ptr(), nbytes, C.byref(g)), "hbm_read_peak")
        return float(g.value)


# ------------------------------------------------------------------------------------------------------
# driver-level entry points (include/rlhip_drivers.h): the C++ RS/RF/QB/RSVD objects behind a C ABI
# ------------------------------------------------------------------------------------------------------
def _state_arr(ctr, key):
    return (C.c_uint32 * 6)(*[int(v) & 0xFFFFFFFF for v in list(ctr) + list(key)])


class _Owned:
    """a callee-allocated device block (rlhip_malloc) exposed through __cuda_array_interface__; returned to the library's pool when the
    last tensor viewing it goes away (the reference's caller free()s these arrays: rl_rsvd.hh:139-143)"""

    def __init__(self, ctx: "Context", ptr: int, shape, typestr: str):
        self._ctx, self._ptr = ctx, ptr
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self._ptr and getattr(self._ctx, "h", None):
                self._ctx.lib.rlhip_free(self._ctx.h, C.c_void_p(self._ptr))
        except Exception:
            pass
        self._ptr = 0


def _adopt(ctx: "Context", ptr: C.c_void_p, rows: int, cols: int, dtype=None):
    """a callee-allocated column-major device block as a torch tensor of shape (cols, rows) WITHOUT a copy: the tensor views the block and
    the block goes back to the library's pool when the tensor dies"""
    torch = _torch()
    dtype = dtype or torch.float64
    if rows * cols <= 0 or not ptr.value:
        if ptr.value:
            _lib.check(ctx.lib.rlhip_free(ctx.h, ptr), "rlhip_free")
        return torch.empty((cols, rows), dtype=dtype, device=f"cuda:{ctx.device}")
    owner = _Owned(ctx, int(ptr.value), (cols, rows), "<f8" if dtype == torch.float64 else "<f4")
    return torch.as_tensor(owner, device=f"cuda:{ctx.device}")


def _drv_check(ctx, rc, what):
    if rc <= -100:
        raise _lib.RlhipError(f"{what}: {ctx.lib.rlhip_last_error().decode()} (code {rc})")
    return rc


def drv_stab(ctx: Context, kind: int, A, m: int, k: int, cond_check: bool = False):
    cf = C.c_int(0)
    rc = getattr(ctx.lib, f"rlhip_drv_stab_{_suffix(A)[0]}")(ctx.h, kind, int(cond_check), m, k, A.data_ptr(), C.byref(cf))
    return _drv_check(ctx, rc, "stab"), bool(cf.value)


def drv_rs(ctx: Context, A, m, n, k, p, q, stab_kind=0, ctr=(0, 0, 0, 0), key=(0, 0)):
    Om = cm_empty(n, k, device=f"cuda:{ctx.device}")
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_rs_f64(ctx.h, m, n, A.data_ptr(), k, p, q, stab_kind, Om.data_ptr(), st)
    return _drv_check(ctx, rc, "rs"), Om, tuple(int(x) for x in st[:4])


def drv_rf(ctx: Context, A, m, n, k, p, q, rs_stab=0, orth_kind=0, ctr=(0, 0, 0, 0), key=(0, 0)):
    Q = cm_empty(m, k, device=f"cuda:{ctx.device}")
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_rf_f64(ctx.h, m, n, A.data_ptr(), k, p, q, rs_stab, orth_kind, Q.data_ptr(), st)
    return _drv_check(ctx, rc, "rf"), Q, tuple(int(x) for x in st[:4])


def drv_qb(ctx: Context, A, m, n, k, b_sz, tol, p, q, rs_stab=0, rf_orth=0, qb_orth=0, orth_check=False,
           ctr=(0, 0, 0, 0), key=(0, 0)):
    kk = C.c_int64(k)
    Qp, Bp = C.c_void_p(), C.c_void_p()
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_qb_f64(ctx.h, m, n, A.data_ptr(), C.byref(kk), b_sz, tol, p, q, rs_stab, rf_orth, qb_orth,
                                  int(orth_check), C.byref(Qp), C.byref(Bp), st)
    _drv_check(ctx, rc, "qb")
    Q = _adopt(ctx, Qp, m, k)
    BT = _adopt(ctx, Bp, n, k)
    kf = int(kk.value)
    return rc, kf, Q[:kf], BT[:kf], tuple(int(x) for x in st[:4])


def drv_rsvd(ctx: Context, A, m, n, k, b_sz, tol, p, q, rs_stab=0, rf_orth=0, qb_orth=0, orth_check=False,
             ctr=(0, 0, 0, 0), key=(0, 0), keep_on_device=True):
    """RSVD::call.  Returns dict(rc, qb_rc, k, U, S, V, next_ctr); U/V are column-major tensors (k, m)/(k, n)."""
    kk = C.c_int64(k)
    Up, Sp, Vp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    qrc = C.c_int(0)
    st = _state_arr(ctr, key)
    suf, _ = _suffix(A)
    rc = getattr(ctx.lib, f"rlhip_drv_rsvd_{suf}")(ctx.h, m, n, A.data_ptr(), C.byref(kk), b_sz, tol, p, q, rs_stab, rf_orth, qb_orth,
                                                   int(orth_check), C.byref(Up), C.byref(Sp), C.byref(Vp), st, C.byref(qrc))
    _drv_check(ctx, rc, "rsvd")
    kf = int(kk.value)
    kal = max(kf, 1)
    U = _adopt(ctx, Up, m, kal, A.dtype)
    S = _adopt(ctx, Sp, kal, 1, A.dtype).reshape(-1)
    V = _adopt(ctx, Vp, n, kal, A.dtype)
    return dict(rc=rc, qb_rc=int(qrc.value), k=kf, U=U[:kf], S=S[:kf], V=V[:kf], next_ctr=tuple(int(x) for x in st[:4]))


def drv_cqrrt(ctx: Context, A, m, n, d_factor=1.25, nnz=2, eps=None, ctr=(0, 0, 0, 0), key=(0, 0), sketch_in=None, want_sketch=False):
    """CQRRT::call.  A (column-major tensor (n, m)) is overwritten by Q.  Returns dict(rc, R, next_ctr[, sketch])."""
    dev = f"cuda:{ctx.device}"
    if eps is None:
        eps = float(np.finfo(np.float64).eps ** 0.85)
    d = int(d_factor * n)
    R = cm_zeros(n, n, device=dev)
    sk_out = cm_empty(d, n, device=dev) if want_sketch else None
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_cqrrt_f64(ctx.h, m, n, A.data_ptr(), m, R.data_ptr(), n, d_factor, nnz, eps, st,
                                     sketch_in.data_ptr() if sketch_in is not None else None,
                                     sk_out.data_ptr() if sk_out is not None else None)
    _drv_check(ctx, rc, "cqrrt")
    out = dict(rc=rc, R=R, next_ctr=tuple(int(x) for x in st[:4]))
    if want_sketch:
        out["sketch"] = sk_out
    return out


def drv_abrik(ctx: Context, A, m, n, k, tol, max_krylov_iters=0, ctr=(0, 0, 0, 0), key=(0, 0), qr_exp=-1):
    """ABRIK::call on the dense operator A (column-major tensor (n, m), not modified).  Returns dict(rc, U, S, V, triplets, iters,
    norm_R_end, next_ctr); U/V are column-major tensors (triplets, m)/(triplets, n)."""
    Up, Sp, Vp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    trip, iters = C.c_int64(0), C.c_int64(0)
    nre = C.c_double(0)
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_abrik_f64(ctx.h, m, n, A.data_ptr(), m, k, tol, max_krylov_iters, C.byref(Up), C.byref(Sp), C.byref(Vp), st,
                                     C.byref(trip), C.byref(iters), C.byref(nre), qr_exp)
    _drv_check(ctx, rc, "abrik")
    t = int(trip.value)
    U = _adopt(ctx, Up, m, t)
    S = _adopt(ctx, Sp, t, 1).reshape(-1)
    V = _adopt(ctx, Vp, n, t)
    return dict(rc=rc, U=U, S=S, V=V, triplets=t, iters=int(iters.value), norm_R_end=float(nre.value),
                next_ctr=tuple(int(x) for x in st[:4]))


def drv_revd2(ctx: Context, A, m, k, tol, uplo="U", syps_passes=2, passes_per_stab=1, error_est_p=10, orth_kind=1, ctr=(0, 0, 0, 0),
              key=(0, 0)):
    """REVD2::call on the symmetric matrix whose `uplo` triangle is stored in A (column-major tensor (m, m)).
    Returns dict(rc, k, V, eigvals, err, next_ctr); V is a column-major tensor (k, m)."""
    Vp, Ep = C.c_void_p(), C.c_void_p()
    kk = C.c_int64(k)
    err = C.c_double(0)
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_revd2_f64(ctx.h, uplo.encode(), m, A.data_ptr(), C.byref(kk), tol, syps_passes, passes_per_stab, error_est_p,
                                     orth_kind, C.byref(Vp), C.byref(Ep), st, C.byref(err))
    _drv_check(ctx, rc, "revd2")
    kf = int(kk.value)
    return dict(rc=rc, k=kf, V=_adopt(ctx, Vp, m, kf), eigvals=_adopt(ctx, Ep, kf, 1).reshape(-1), err=float(err.value),
                next_ctr=tuple(int(x) for x in st[:4]))


def drv_syrf(ctx: Context, A, m, k, uplo="U", syps_passes=2, passes_per_stab=1, orth_kind=1, ctr=(0, 0, 0, 0), key=(0, 0)):
    """SYRF::call.  Returns dict(rc, Q, next_ctr) with Q a column-major tensor (k, m)."""
    Q = cm_zeros(m, k, device=f"cuda:{ctx.device}")
    st = _state_arr(ctr, key)
    rc = ctx.lib.rlhip_drv_syrf_f64(ctx.h, uplo.encode(), m, A.data_ptr(), k, syps_passes, passes_per_stab, orth_kind, Q.data_ptr(), st)
    _drv_check(ctx, rc, "syrf")
    return dict(rc=rc, Q=Q, next_ctr=tuple(int(x) for x in st[:4]))


MAT_TYPES = {"polynomial": 0, "exponential": 1, "gaussian": 2, "step": 3, "spiked": 4, "adverserial": 5, "bad_cholqr": 6, "kahan": 7}


def drv_mat_gen(ctx: Context, m_type, m, n, rank=None, cond_num=1.0, scaling=1.0, exponent=1.0, diag=False, theta=1.0, perturb=1.0,
                frac_spectrum_one=0.1, check_true_rank=False, ctr=(0, 0, 0, 0), key=(0, 0), dtype=None):
    """gen::mat_gen into HBM.  Returns dict(A, rank, next_ctr); A is a column-major tensor (n, m) ((rank, rank) when diag)."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    dtype = dtype or torch.float64
    rank = n if rank is None else rank
    A = cm_zeros(rank, rank, dtype=dtype, device=dev) if diag else cm_zeros(m, n, dtype=dtype, device=dev)
    st = _state_arr(ctr, key)
    r_out = C.c_int64(rank)
    suf = "f64" if dtype == torch.float64 else "f32"
    rc = getattr(ctx.lib, f"rlhip_drv_mat_gen_{suf}")(ctx.h, MAT_TYPES[m_type] if isinstance(m_type, str) else m_type, m, n, rank, cond_num,
                                                      scaling, exponent, 1 if diag else 0, theta, perturb, frac_spectrum_one,
                                                      1 if check_true_rank else 0, A.data_ptr(), st, C.byref(r_out))
    _drv_check(ctx, rc, "mat_gen")
    return dict(A=A, rank=int(r_out.value), next_ctr=tuple(int(x) for x in st[:4]))


class DenseOperator:
    """linops::DenseLinOp over a column-major device tensor (n, m) (rows m, cols n)."""

    def __init__(self, A, m, n):
        self.A, self.rows, self.cols = A, m, n
        self.dtype = A.dtype

    def desc(self):
        from ._lib import LinOpDesc
        return LinOpDesc(0, self.rows, self.cols, self.A.data_ptr(), self.rows, 0, None, None, None)


class CsrOperator:
    """linops::SparseLinOp over device CSR arrays (int64 rowptr / colidx).  Build from scipy with `from_scipy`."""

    def __init__(self, rows, cols, rowptr, colidx, vals):
        self.rows, self.cols = rows, cols
        self.rowptr, self.colidx, self.vals = rowptr, colidx, vals
        self.dtype = vals.dtype

    @classmethod
    def from_scipy(cls, sp, device="cuda:0", dtype=None):
        torch = _torch()
        csr = sp.tocsr()
        dt = dtype or torch.float64
        return cls(csr.shape[0], csr.shape[1], torch.as_tensor(csr.indptr.astype(np.int64), device=device),
                   torch.as_tensor(csr.indices.astype(np.int64), device=device),
                   torch.as_tensor(csr.data, device=device).to(dt))

    def desc(self):
        from ._lib import LinOpDesc
        return LinOpDesc(1, self.rows, self.cols, None, 0, int(self.vals.numel()), self.rowptr.data_ptr(), self.colidx.data_ptr(),
                         self.vals.data_ptr())


class CscOperator(CsrOperator):
    """linops::SparseLinOp::from_csc: the operator given by its columns (colptr, row indices, values)"""

    @classmethod
    def from_scipy(cls, sp, device="cuda:0", dtype=None):
        torch = _torch()
        csc = sp.tocsc()
        dt = dtype or torch.float64
        return cls(csc.shape[0], csc.shape[1], torch.as_tensor(csc.indptr.astype(np.int64), device=device),
                   torch.as_tensor(csc.indices.astype(np.int64), device=device), torch.as_tensor(csc.data, device=device).to(dt))

    def desc(self):
        from ._lib import LinOpDesc
        return LinOpDesc(2, self.rows, self.cols, None, 0, int(self.vals.numel()), self.rowptr.data_ptr(), self.colidx.data_ptr(), self.vals.data_ptr())


class CooOperator(CsrOperator):
    """linops::SparseLinOp::from_coo: (row, col, value) triplets in any order, duplicates summed"""

    @classmethod
    def from_triplets(cls, rows, cols, ri, ci, v, device="cuda:0", dtype=None):
        torch = _torch()
        dt = dtype or torch.float64
        return cls(rows, cols, torch.as_tensor(np.asarray(ri, dtype=np.int64), device=device), torch.as_tensor(np.asarray(ci, dtype=np.int64), device=device),
                   torch.as_tensor(np.asarray(v), device=device).to(dt))

    def desc(self):
        from ._lib import LinOpDesc
        return LinOpDesc(3, self.rows, self.cols, None, 0, int(self.vals.numel()), self.rowptr.data_ptr(), self.colidx.data_ptr(), self.vals.data_ptr())


def _op_descs(op):
    """op: DenseOperator | CsrOperator | (left, right) -> (left desc, right desc or None, rows, cols, dtype)"""
    if isinstance(op, tuple):
        left, right = op
        return left.desc(), right.desc(), left.rows, right.cols, left.dtype
    return op.desc(), None, op.rows, op.cols, op.dtype


QR_LINOPS_ALGS = {"cholqr": 0, "scholqr3": 1, "scholqr3_basic": 2, "cqrrt": 3}


def drv_qr_linops(ctx: Context, alg, op, block_size=0, want_Q=False, d_factor=2.0, nnz=2, use_dense_sketch=False, ctr=(0, 0, 0, 0),
                  key=(0, 0), sketch_in=None, want_sketch=False):
    """CholQR_linops / sCholQR3_linops / sCholQR3_linops_basic / CQRRT_linops ::call on a dense, CSR or composite (tuple) operator.
    Returns dict(rc, R[, Q][, sketch], next_ctr); R and Q are column-major tensors (n, n) / (n, m)."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    ld, rd, m, n, dtype = _op_descs(op)
    suf = "f64" if dtype == torch.float64 else "f32"
    R = cm_zeros(n, n, dtype=dtype, device=dev)
    d = int(d_factor * n)
    sk_out = cm_empty(d, n, dtype=dtype, device=dev) if want_sketch else None
    Qp = C.c_void_p()
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_qr_linops_{suf}")(
        ctx.h, QR_LINOPS_ALGS[alg] if isinstance(alg, str) else alg, C.byref(ld), C.byref(rd) if rd is not None else None, R.data_ptr(), n,
        block_size, C.byref(Qp) if want_Q else None, d_factor, nnz, 1 if use_dense_sketch else 0, st,
        sketch_in.data_ptr() if sketch_in is not None else None, sk_out.data_ptr() if sk_out is not None else None)
    _drv_check(ctx, rc, "qr_linops")
    out = dict(rc=rc, R=R, next_ctr=tuple(int(x) for x in st[:4]))
    if want_Q:
        out["Q"] = _adopt(ctx, Qp, m, n, dtype=dtype) if Qp.value else None
    if want_sketch:
        out["sketch"] = sk_out
    return out


ABRIK_TIMES = ("allocation", "get_factors", "ungqr", "reorth", "qr", "gemm_A", "main_loop", "sketching", "r_cpy", "s_cpy", "norm", "rest", "total")


def drv_abrik_linop(ctx: Context, op, k, tol, max_krylov_iters=0, ctr=(0, 0, 0, 0), key=(0, 0), qr_exp=-1, timing=False):
    """ABRIK::call on a DenseOperator / CsrOperator.  Same outputs as drv_abrik; timing=True arms ABRIK's subroutine timers and adds
    times_us (the 13 entries of ABRIK::times, rl_abrik.hh:733-734, names in ABRIK_TIMES)."""
    ld, rd, m, n, _ = _op_descs(op)
    Up, Sp, Vp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    trip, iters = C.c_int64(0), C.c_int64(0)
    nre = C.c_double(0)
    st = _state_arr(ctr, key)
    times = (C.c_long * 13)() if timing else None
    if timing:
        if rd is not None:
            raise ValueError("ABRIK runs on single operators only")
        rc = ctx.lib.rlhip_drv_abrik_linop_timed_f64(ctx.h, C.byref(ld), k, tol, max_krylov_iters, C.byref(Up), C.byref(Sp), C.byref(Vp), st,
                                                     C.byref(trip), C.byref(iters), C.byref(nre), qr_exp, times)
    else:
        rc = ctx.lib.rlhip_drv_abrik_linop_f64(ctx.h, C.byref(ld), C.byref(rd) if rd is not None else None, k, tol, max_krylov_iters,
                                               C.byref(Up), C.byref(Sp), C.byref(Vp), st, C.byref(trip), C.byref(iters), C.byref(nre), qr_exp)
    _drv_check(ctx, rc, "abrik_linop")
    t = int(trip.value)
    out = dict(rc=rc, U=_adopt(ctx, Up, m, t), S=_adopt(ctx, Sp, t, 1).reshape(-1), V=_adopt(ctx, Vp, n, t), triplets=t,
               iters=int(iters.value), norm_R_end=float(nre.value), next_ctr=tuple(int(x) for x in st[:4]))
    if timing:
        out["times_us"] = [int(x) for x in times]
    return out


def linop_apply(ctx: Context, op, side, trans, B, m, n, k, alpha=1.0, beta=0.0, C_in=None):
    """C (m x n) = alpha * op(A) * B + beta * C (side 'L') or alpha * B * op(A) + beta * C (side 'R'); column-major tensors."""
    dev = f"cuda:{ctx.device}"
    ld, rd, _, _, _ = _op_descs(op)
    Cout = C_in if C_in is not None else cm_zeros(m, n, device=dev)
    ldb = B.shape[1]
    rc = ctx.lib.rlhip_linop_apply_f64(ctx.h, C.byref(ld), C.byref(rd) if rd is not None else None, side.encode(), trans.encode(), m, n, k,
                                       alpha, B.data_ptr(), ldb, beta, Cout.data_ptr(), m)
    _drv_check(ctx, rc, "linop_apply")
    return Cout


VIEW_HOW = {"row_block": 0, "col_block": 1, "submatrix": 2}


def linop_apply_view(ctx: Context, op, how, view, side, trans, B, m, n, k, alpha=1.0, beta=0.0, C_in=None):
    """the same product with a block view of the operator: how in VIEW_HOW, view = (row_start, col_start, row_count, col_count)"""
    dev = f"cuda:{ctx.device}"
    ld, rd, _, _, _ = _op_descs(op)
    Cout = C_in if C_in is not None else cm_zeros(m, n, device=dev)
    v = (C.c_int64 * 4)(*[int(x) for x in view])
    rc = ctx.lib.rlhip_linop_apply_view_f64(ctx.h, C.byref(ld), C.byref(rd) if rd is not None else None, VIEW_HOW[how], v, side.encode(), trans.encode(),
                                            m, n, k, alpha, B.data_ptr(), B.shape[1], beta, Cout.data_ptr(), m)
    _drv_check(ctx, rc, "linop_apply_view")
    return Cout


def regsym_apply(ctx: Context, A, dim, regs, eval_includes_reg, B, n, alpha=1.0, beta=0.0, C_in=None, lda=None):
    """linops::RegExplicitSymLinOp: C = alpha (A + mu_i I) B + beta C, A by its upper triangle (column-major tensor (dim, lda))"""
    dev = f"cuda:{ctx.device}"
    Cout = C_in if C_in is not None else cm_zeros(dim, n, device=dev)
    rg = (C.c_double * max(len(regs), 1))(*[float(x) for x in regs])
    rc = ctx.lib.rlhip_regsym_apply_f64(ctx.h, dim, A.data_ptr(), lda or dim, rg, len(regs), int(bool(eval_includes_reg)), n, alpha, B.data_ptr(),
                                        B.shape[1], beta, Cout.data_ptr(), dim)
    _drv_check(ctx, rc, "regsym_apply")
    return Cout


def drv_hqrrp(ctx: Context, A, m, n, nb_alg=64, pp=10, panel_pivoting=1, qr_type=0, ctr=(0, 0, 0, 0), key=(0, 0), want_G=False, m_global=None):
    """hqrrp: A (column-major tensor (n, m)) is overwritten in GEQP3 format.  Returns dict(rc, tau, J, next_ctr[, G]).
    Row-sharded context: m = this rank's rows, m_global = the matrix's (tau has min(m_global, n) entries)."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    tau = torch.zeros(min(m_global or m, n), dtype=A.dtype, device=dev)
    J = torch.zeros(n, dtype=torch.int64, device=dev)
    G = cm_empty(nb_alg + pp, m, dtype=A.dtype, device=dev) if want_G else None
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_hqrrp_{_suffix(A)[0]}")(ctx.h, m, n, A.data_ptr(), m, J.data_ptr(), tau.data_ptr(), nb_alg, pp, panel_pivoting, qr_type,
                                     st, G.data_ptr() if G is not None else None)
    _drv_check(ctx, rc, "hqrrp")
    out = dict(rc=rc, tau=tau, J=J, next_ctr=tuple(int(x) for x in st[:4]))
    if want_G:
        out["G"] = G
    return out


def drv_hqrrp_timed(ctx: Context, A, m, n, nb_alg=64, pp=10, panel_pivoting=0, qr_type=0, ctr=(0, 0, 0, 0), key=(0, 0)):
    """hqrrp with the reference's timing argument armed: dict(rc, tau, J, times_us (27 entries, rl_hqrrp.hh:1144-1164))"""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    tau = torch.zeros(min(m, n), dtype=A.dtype, device=dev)
    J = torch.zeros(n, dtype=torch.int64, device=dev)
    st = _state_arr(ctr, key)
    times = (C.c_double * 27)()
    rc = ctx.lib.rlhip_drv_hqrrp_timed_f64(ctx.h, m, n, A.data_ptr(), m, J.data_ptr(), tau.data_ptr(), nb_alg, pp, panel_pivoting, qr_type, st, times)
    _drv_check(ctx, rc, "hqrrp_timed")
    return dict(rc=rc, tau=tau, J=J, times_us=[float(x) for x in times])


def drv_cqrrpt(ctx: Context, A, m, n, d_factor=1.25, nnz=4, eps=None, ctr=(0, 0, 0, 0), key=(0, 0), sketch_in=None,
               want_sketch=False, timing=False, qrcp=-1):
    """CQRRPT::call (qrcp = geqp3).  A (column-major tensor (n, m)) is overwritten by Q.  Returns dict(rc, rank, R, J,
    next_ctr[, sketch][, times_us])."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    npdt = np.float64 if A.dtype == torch.float64 else np.float32
    if eps is None:
        eps = float(np.finfo(npdt).eps ** 0.85)
    d = int(d_factor * n)
    R = cm_zeros(n, n, dtype=A.dtype, device=dev)
    J = torch.zeros(n, dtype=torch.int64, device=dev)
    sk_out = cm_empty(d, n, dtype=A.dtype, device=dev) if want_sketch else None
    rank = C.c_int64(0)
    st = _state_arr(ctr, key)
    times = (C.c_long * 8)() if timing else None
    rc = getattr(ctx.lib, f"rlhip_drv_cqrrpt_{_suffix(A)[0]}")(ctx.h, m, n, A.data_ptr(), m, R.data_ptr(), n, J.data_ptr(), d_factor, nnz, eps, st,
                                      sketch_in.data_ptr() if sketch_in is not None else None,
                                      sk_out.data_ptr() if sk_out is not None else None, C.byref(rank), times, qrcp)
    _drv_check(ctx, rc, "cqrrpt")
    out = dict(rc=rc, rank=int(rank.value), R=R, J=J, next_ctr=tuple(int(x) for x in st[:4]))
    if want_sketch:
        out["sketch"] = sk_out
    if timing:
        out["times_us"] = [int(t) for t in times]
    return out


def drv_bqrrp(ctx: Context, A, m, n, b_sz, d_factor=1.0, internal_nb=0, tol=0.0, ctr=(0, 0, 0, 0), key=(0, 0), sketch_in=None,
              want_sketch=False, timing=False, qrcp_wide=-1, qr_tall=-1, apply_trans_q=-1, m_global=None, block_cyclic=False):
    """BQRRP::call; options as in the reference's enums (qrcp_wide 0 luqr | 1 geqp3; qr_tall 0 geqrt | 1 cholqr | 2 geqrf;
    apply_trans_q 0 ormqr | 1 gemqrt; -1 = object default).  A (column-major tensor (n, m)) is overwritten in GEQP3 format.
    Returns dict(rc, rank, tau, J, next_ctr[, sketch][, times_us])."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    d = int(d_factor * b_sz)
    # row-sharded call (context joined to a communicator): m is the LOCAL row count, tau has min(global rows, n) entries
    tau = torch.zeros(min(m_global or m, n), dtype=A.dtype, device=dev)
    J = torch.zeros(n, dtype=torch.int64, device=dev)
    sk_out = cm_empty(d, n, dtype=A.dtype, device=dev) if want_sketch else None
    rank = C.c_int64(0)
    st = _state_arr(ctr, key)
    times = (C.c_long * 9)() if timing else None
    rc = getattr(ctx.lib, f"rlhip_drv_bqrrp_{_suffix(A)[0]}")(ctx.h, m, n, A.data_ptr(), m, d_factor, b_sz, internal_nb, tol, tau.data_ptr(), J.data_ptr(),
                                     st, sketch_in.data_ptr() if sketch_in is not None else None,
                                     sk_out.data_ptr() if sk_out is not None else None, C.byref(rank), times,
                                     qrcp_wide, (16 + (qr_tall if qr_tall >= 0 else 3)) if block_cyclic else qr_tall, apply_trans_q)
    _drv_check(ctx, rc, "bqrrp")
    out = dict(rc=rc, rank=int(rank.value), tau=tau, J=J, next_ctr=tuple(int(x) for x in st[:4]))
    if want_sketch:
        out["sketch"] = sk_out
    if timing:
        out["times_us"] = [int(t) for t in times]
    return out


def drv_bqrrp_gpu(ctx: Context, A, m, n, A_sk, d, b_sz, qr_tall=-1, tol=0.0, timing=False, lda=None):
    """BQRRP_GPU::call (the reference's device class, drivers/rl_bqrrp_gpu.hh:120-129): the d x n sketch A_sk (column-major tensor
    (n, d), OVERWRITTEN) is an input.  qr_tall 0 cholqr | 1 geqrf | -1 object default (geqrf).  A is overwritten in GEQP3 format.
    Returns dict(rc, rank, tau, J[, times_us (15 entries)])."""
    torch = _torch()
    dev = f"cuda:{ctx.device}"
    tau = torch.zeros(n, dtype=A.dtype, device=dev)
    J = torch.zeros(n, dtype=torch.int64, device=dev)
    rank = C.c_int64(0)
    times = (C.c_long * 15)() if timing else None
    rc = getattr(ctx.lib, f"rlhip_drv_bqrrp_gpu_{_suffix(A)[0]}")(ctx.h, m, n, A.data_ptr(), lda or m, A_sk.data_ptr(), d, b_sz, qr_tall, tol,
                                                                   tau.data_ptr(), J.data_ptr(), C.byref(rank), times)
    _drv_check(ctx, rc, "bqrrp_gpu")
    out = dict(rc=rc, rank=int(rank.value), tau=tau, J=J)
    if timing:
        out["times_us"] = [int(t) for t in times]
    return out


def drv_cqrrpt_gpu(ctx: Context, A_host, d_factor=1.25, nnz=4, eps=None, ctr=(0, 0, 0, 0), key=(0, 0), no_hqrrp=-1, want_sketch=False,
                   timing=False, lda=None, ldr=None):
    """CQRRPT_GPU::call (drivers/rl_cqrrpt_gpu.hh:117-127): HOST matrices, as in the reference.  A_host: numpy (m, n); it is NOT
    modified -- the call runs on a column-major copy with leading dimension lda (default m).  Returns dict(rc, rank, Q (m x n numpy),
    R (n x n numpy), J, next_ctr[, sketch (d x n numpy)][, times_us], A_buf / R_buf = the raw padded buffers)."""
    m, n = A_host.shape
    npdt = A_host.dtype.type
    lda = lda or m
    ldr = ldr or n
    if eps is None:
        eps = float(np.finfo(npdt).eps ** 0.85)
    d = int(npdt(d_factor) * n)
    A_buf = np.full(lda * n, np.nan, dtype=npdt)
    A_buf.reshape(n, lda)[:, :m] = A_host.T
    R_buf = np.full(ldr * n, 7.0, dtype=npdt)                       # padding rows keep their marker (checked by the tests)
    R_buf.reshape(n, ldr)[:, :n] = 0.0
    J = np.zeros(n, dtype=np.int64)
    sk = np.zeros(d * n, dtype=npdt) if want_sketch else None
    rank = C.c_int64(0)
    st = _state_arr(ctr, key)
    times = (C.c_long * 8)() if timing else None
    suffix = "f64" if npdt is np.float64 else "f32"
    rc = getattr(ctx.lib, f"rlhip_drv_cqrrpt_gpu_{suffix}")(ctx.h, m, n, A_buf.ctypes.data, lda, R_buf.ctypes.data, ldr, J.ctypes.data, d_factor, nnz, eps,
                                                           no_hqrrp, st, sk.ctypes.data if sk is not None else None, C.byref(rank), times)
    _drv_check(ctx, rc, "cqrrpt_gpu")
    out = dict(rc=rc, rank=int(rank.value), Q=A_buf.reshape(n, lda)[:, :m].T.copy(), R=R_buf.reshape(n, ldr)[:, :n].T.copy(), J=J,
               next_ctr=tuple(int(x) for x in st[:4]), A_buf=A_buf, R_buf=R_buf)
    if want_sketch:
        out["sketch"] = sk.reshape(n, d).T.copy()
    if timing:
        out["times_us"] = [int(t) for t in times]
    return out


# ---- squared-exponential kernel matrices and randomly pivoted Cholesky (rpchol.hip; include/RandLAPACK_amd/rl_rpchol.hh, rl_pdkernels.hh).
#      X is a column-major tensor (n, rows_x): column j of the rows_x x n matrix (one data point) is X[j].  fp64 or fp32 by X's dtype.
def _suf(t):
    torch = _torch()
    if t.dtype == torch.float64:
        return "f64", C.c_double
    if t.dtype == torch.float32:
        return "f32", C.c_float
    raise TypeError(f"unsupported dtype {t.dtype}")


def _ld(t):
    """leading dimension of a column-major tensor (cols, ld-strided rows)"""
    return int(t.stride(0)) if t.dim() == 2 else int(t.numel())


def sqexp_columns(ctx: Context, X, rows_x, n, idx, bandwidth, reg=0.0, out=None):
    """out(i, l) = exp(-|x_i - x_idx[l]|^2 / (2 h^2)) (+ reg where i == idx[l]); idx: int64 device tensor.  Returns out (nidx, n) column-major."""
    torch = _torch()
    suf, _ = _suf(X)
    nidx = int(idx.numel())
    if out is None:
        out = torch.empty((nidx, n), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_sqexp_columns_{suf}")(ctx.h, rows_x, n, X.data_ptr(), _ld(X), nidx, idx.data_ptr(), bandwidth, reg,
                                                       out.data_ptr(), _ld(out) if nidx > 1 else max(n, 1))
    _lib.check(rc, "sqexp_columns")
    return out


def sqexp_submatrix(ctx: Context, X, rows_x, cols_x, rows_k, cols_k, ro, co, bandwidth, sq_colnorms=None):
    """squared_exp_kernel_submatrix: Ksub (cols_k, rows_k) column-major"""
    torch = _torch()
    suf, _ = _suf(X)
    K = torch.empty((cols_k, rows_k), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_sqexp_submatrix_{suf}")(ctx.h, rows_x, cols_x, X.data_ptr(), _ld(X),
                                                         None if sq_colnorms is None else sq_colnorms.data_ptr(), rows_k, cols_k, K.data_ptr(),
                                                         max(rows_k, 1), ro, co, bandwidth)
    _lib.check(rc, "sqexp_submatrix")
    return K


def sq_colnorms(ctx: Context, X, rows_x, cols_x):
    torch = _torch()
    suf, _ = _suf(X)
    nr = torch.empty(cols_x, dtype=X.dtype, device=X.device)
    _lib.check(getattr(ctx.lib, f"rlhip_sq_colnorms_{suf}")(ctx.h, rows_x, cols_x, X.data_ptr(), _ld(X), nr.data_ptr()), "sq_colnorms")
    return nr


def rbf_apply(ctx: Context, X, rows_x, dim, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None, regs=(), eval_includes_reg=False):
    """linops::RBFKernelMatrix::operator(): C = alpha (K [+ regs]) B + beta C; B, C column-major (n, dim)"""
    torch = _torch()
    suf, T = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, dim), dtype=X.dtype, device=X.device)
    rg = (T * max(len(regs), 1))(*(list(regs) or [0.0]))
    rc = getattr(ctx.lib, f"rlhip_rbf_apply_{suf}")(ctx.h, rows_x, dim, X.data_ptr(), _ld(X), bandwidth, rg, max(len(regs), 1),
                                                   1 if eval_includes_reg else 0, n, alpha, B.data_ptr(), _ld(B), beta, C_.data_ptr(), _ld(C_))
    _lib.check(rc, "rbf_apply")
    return C_


# ---- the RBF kernel between two point sets and KRR prediction (rbf.hip).  Z (mz, ldz) and X (nx, ldx) are column-major point tensors like X
#      above; B (n, ldb >= nx) and C (n, ldc >= mz) column-major.
def rbf_split_chunks(mz: int, nx: int) -> int:
    """chunks of X that options(rbf_fused=2) cuts a cross apply with mz points of Z and nx points of X into: a function of the shape alone
    (rlhip_rbf_split_chunks); needs no context and no device"""
    return int(_lib.load().rlhip_rbf_split_chunks(mz, nx))


def rbf_cross_apply(ctx: Context, Z, X, rows_x, mz, nx, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None):
    """C (mz x n) = alpha K(Z, X) B + beta C (rlhip_rbf_cross_apply_*); returns C, column-major (n, mz) when allocated here"""
    torch = _torch()
    suf, _ = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, mz), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_rbf_cross_apply_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), nx, X.data_ptr(), _ld(X), bandwidth, n, alpha,
                                                         B.data_ptr(), max(_ld(B), 1), beta, C_.data_ptr(), max(_ld(C_), 1))
    _lib.check(rc, "rbf_cross_apply")
    return C_


def sqexp_cross_submatrix(ctx: Context, Z, X, rows_x, mz, nx, rows_k, cols_k, ro, co, bandwidth, sq_colnorms_z=None, sq_colnorms_x=None):
    """Ksub (cols_k, rows_k) column-major = K(Z(:, ro : ro + rows_k), X(:, co : co + cols_k)) (rlhip_sqexp_cross_submatrix_*)"""
    torch = _torch()
    suf, _ = _suf(X)
    K = torch.empty((cols_k, rows_k), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_sqexp_cross_submatrix_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), _ptr(sq_colnorms_z), nx, X.data_ptr(), _ld(X),
                                                               _ptr(sq_colnorms_x), rows_k, cols_k, K.data_ptr(), max(rows_k, 1), ro, co, bandwidth)
    _lib.check(rc, "sqexp_cross_submatrix")
    return K


def krr_predict(ctx: Context, Z, mz, Xp, rows_x, n, bandwidth, coeffs, s):
    """RandLAPACK::krr_predict over linops::RBFCrossKernel: Y (mz x s) = K(Z, Xp) coeffs for the n training points Xp and the n x s
    coefficient block of krill_full_rpchol.  Returns Y, column-major (s, mz)."""
    torch = _torch()
    suf, _ = _suf(Xp)
    Y = torch.zeros((s, mz), dtype=Xp.dtype, device=Xp.device)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), bandwidth, s,
                                                         coeffs.data_ptr(), max(_ld(coeffs), 1), Y.data_ptr(), max(mz, 1))
    _drv_check(ctx, rc, "krr_predict")
    return Y


def rbf_kernel_apply(ctx: Context, X, rows_x, dim, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None, regs=(), eval_includes_reg=False,
                     matrix_free=False):
    """linops::RBFKernelMatrix::operator() through the C++ object, with set_matrix_free(matrix_free): same arguments as rbf_apply"""
    torch = _torch()
    suf, T = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, dim), dtype=X.dtype, device=X.device)
    rg = (T * max(len(regs), 1))(*(list(regs) or [0.0]))
    rc = getattr(ctx.lib, f"rlhip_drv_rbf_kernel_apply_{suf}")(ctx.h, X.data_ptr(), _ld(X), rows_x, dim, bandwidth, rg, max(len(regs), 1),
                                                              1 if eval_includes_reg else 0, 1 if matrix_free else 0, n, alpha, B.data_ptr(),
                                                              _ld(B), beta, C_.data_ptr(), _ld(C_))
    _drv_check(ctx, rc, "rbf_kernel_apply")
    return C_


# ---- the kernel function as an argument: the wrappers above with `kernel` in front of the bandwidth -- PDK_SQEXP, PDK_MATERN32 or
#      PDK_MATERN52 (RLHIP_PDK_* of include/rlhip.h).  Same tensors, same layouts, same routes and counters.
PDK_SQEXP, PDK_MATERN32, PDK_MATERN52 = 0, 1, 2


def pdk_columns(ctx: Context, X, rows_x, n, idx, kernel, bandwidth, reg=0.0, out=None):
    """sqexp_columns for the kernel function `kernel`: out(i, l) = K(x_i, x_idx[l]) by differences (+ reg where i == idx[l])"""
    torch = _torch()
    suf, _ = _suf(X)
    nidx = int(idx.numel())
    if out is None:
        out = torch.empty((nidx, n), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_columns_{suf}")(ctx.h, rows_x, n, X.data_ptr(), _ld(X), nidx, idx.data_ptr(), kernel, bandwidth, reg,
                                                     out.data_ptr(), _ld(out) if nidx > 1 else max(n, 1))
    _lib.check(rc, "pdk_columns")
    return out


def pdk_submatrix(ctx: Context, X, rows_x, cols_x, rows_k, cols_k, ro, co, kernel, bandwidth, sq_colnorms=None):
    """sqexp_submatrix for the kernel function `kernel`: Ksub (cols_k, rows_k) column-major"""
    torch = _torch()
    suf, _ = _suf(X)
    K = torch.empty((cols_k, rows_k), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_submatrix_{suf}")(ctx.h, rows_x, cols_x, X.data_ptr(), _ld(X), _ptr(sq_colnorms), rows_k, cols_k, K.data_ptr(),
                                                       max(rows_k, 1), ro, co, kernel, bandwidth)
    _lib.check(rc, "pdk_submatrix")
    return K


def pdk_apply(ctx: Context, X, rows_x, dim, kernel, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None, regs=(), eval_includes_reg=False):
    """rbf_apply for the kernel function `kernel`: C = alpha (K [+ regs]) B + beta C by row blocks of K; B, C column-major (n, dim)"""
    torch = _torch()
    suf, T = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, dim), dtype=X.dtype, device=X.device)
    rg = (T * max(len(regs), 1))(*(list(regs) or [0.0]))
    rc = getattr(ctx.lib, f"rlhip_pdk_apply_{suf}")(ctx.h, rows_x, dim, X.data_ptr(), _ld(X), kernel, bandwidth, rg, max(len(regs), 1),
                                                   1 if eval_includes_reg else 0, n, alpha, B.data_ptr(), _ld(B), beta, C_.data_ptr(), _ld(C_))
    _lib.check(rc, "pdk_apply")
    return C_


def pdk_cross_apply(ctx: Context, Z, X, rows_x, mz, nx, kernel, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None):
    """rbf_cross_apply for the kernel function `kernel`: C (mz x n) = alpha K(Z, X) B + beta C, fused or composed"""
    torch = _torch()
    suf, _ = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, mz), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_cross_apply_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), nx, X.data_ptr(), _ld(X), kernel, bandwidth, n, alpha,
                                                         B.data_ptr(), max(_ld(B), 1), beta, C_.data_ptr(), max(_ld(C_), 1))
    _lib.check(rc, "pdk_cross_apply")
    return C_


def pdk_cross_submatrix(ctx: Context, Z, X, rows_x, mz, nx, rows_k, cols_k, ro, co, kernel, bandwidth, sq_colnorms_z=None, sq_colnorms_x=None):
    """sqexp_cross_submatrix for the kernel function `kernel`: Ksub (cols_k, rows_k) column-major"""
    torch = _torch()
    suf, _ = _suf(X)
    K = torch.empty((cols_k, rows_k), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_cross_submatrix_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), _ptr(sq_colnorms_z), nx, X.data_ptr(), _ld(X),
                                                             _ptr(sq_colnorms_x), rows_k, cols_k, K.data_ptr(), max(rows_k, 1), ro, co, kernel,
                                                             bandwidth)
    _lib.check(rc, "pdk_cross_submatrix")
    return K


def krr_predict_pdk(ctx: Context, Z, mz, Xp, rows_x, n, kernel, bandwidth, coeffs, s):
    """krr_predict over an RBFCrossKernel with set_kernel(kernel): Y (mz x s) = K(Z, Xp) coeffs, column-major (s, mz)"""
    torch = _torch()
    suf, _ = _suf(Xp)
    Y = torch.zeros((s, mz), dtype=Xp.dtype, device=Xp.device)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_pdk_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), kernel, bandwidth, s,
                                                             coeffs.data_ptr(), max(_ld(coeffs), 1), Y.data_ptr(), max(mz, 1))
    _drv_check(ctx, rc, "krr_predict_pdk")
    return Y


def pdk_cross_grad(ctx: Context, Z, X, rows_x, mz, nx, kernel, bandwidth, B, n, alpha=1.0, G=None):
    """rlhip_pdk_cross_grad_*: G (rows_x x (mz n)), column r mz + i = the gradient at Z(:, i) of alpha K(Z, X) B(:, r); a tensor (n mz, ldg)
    column-major, laid out like Z per right-hand side.  G given: written in place with its own leading dimension."""
    torch = _torch()
    suf, _ = _suf(X)
    if G is None:
        G = torch.zeros((n * mz, rows_x), dtype=X.dtype, device=X.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_cross_grad_{suf}")(ctx.h, rows_x, mz, _ptr(Z), _ld(Z), nx, _ptr(X), _ld(X), kernel, bandwidth, n, alpha, _ptr(B),
                                                        max(_ldc(B), 1), G.data_ptr(), max(_ldc(G), 1))
    _lib.check(rc, "pdk_cross_grad")
    return G


def krr_predict_grad_pdk(ctx: Context, Z, mz, Xp, rows_x, n, kernel, bandwidth, coeffs, s):
    """krr_predict_grad: the gradients of krr_predict_pdk's functions at the points of Z; (s mz, rows_x) column-major, row c mz + i of the
    tensor = the gradient at Z(:, i) of the function of the c-th regularization"""
    torch = _torch()
    suf, _ = _suf(Xp)
    G = torch.zeros((s * mz, rows_x), dtype=Xp.dtype, device=Xp.device)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_grad_pdk_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), kernel, bandwidth,
                                                                  s, coeffs.data_ptr(), max(_ldc(coeffs), 1), G.data_ptr(), rows_x)
    _drv_check(ctx, rc, "krr_predict_grad_pdk")
    return G


def krr_predict_restricted_grad_pdk(ctx: Context, Z, mz, Xp, rows_x, n, kernel, bandwidth, S, alpha, s):
    """krr_predict_restricted_grad: the gradients of krr_predict_restricted_pdk's functions at the points of Z, laid out as
    krr_predict_grad_pdk lays them out"""
    torch = _torch()
    suf, _ = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    G = torch.zeros((s * mz, rows_x), dtype=Xp.dtype, device=Xp.device)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_restricted_grad_pdk_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), kernel,
                                                                             bandwidth, int(S.size), S.ctypes.data_as(C.POINTER(C.c_int64)), s,
                                                                             alpha.data_ptr(), max(_ldc(alpha), 1), G.data_ptr(), rows_x)
    _drv_check(ctx, rc, "krr_predict_restricted_grad_pdk")
    return G


def pdk_kernel_apply(ctx: Context, X, rows_x, dim, kernel, bandwidth, B, n, alpha=1.0, beta=0.0, C_=None, regs=(), eval_includes_reg=False,
                     matrix_free=False):
    """linops::RBFKernelMatrix::operator() through the C++ object with set_kernel(kernel) and set_matrix_free(matrix_free)"""
    torch = _torch()
    suf, T = _suf(X)
    if C_ is None:
        C_ = torch.zeros((n, dim), dtype=X.dtype, device=X.device)
    rg = (T * max(len(regs), 1))(*(list(regs) or [0.0]))
    rc = getattr(ctx.lib, f"rlhip_drv_pdk_kernel_apply_{suf}")(ctx.h, X.data_ptr(), _ld(X), rows_x, dim, kernel, bandwidth, rg, max(len(regs), 1),
                                                              1 if eval_includes_reg else 0, 1 if matrix_free else 0, n, alpha, B.data_ptr(),
                                                              _ld(B), beta, C_.data_ptr(), _ld(C_))
    _drv_check(ctx, rc, "pdk_kernel_apply")
    return C_


def sample_indices_iid(ctx: Context, d, k, unique=False, ctr=(0, 0, 0, 0), key=(0, 0)):
    """the library's weighted iid sampler (include/rlhip.h rlhip_sample_indices_iid_*) on the device weights d.
    Returns dict(S (numpy int64: k draws, or the sorted distinct ones), count, status, next_ctr, S_dev)."""
    torch = _torch()
    suf, _ = _suf(d)
    out_dev = torch.empty(max(k, 1), dtype=torch.int64, device=d.device)
    out_host = np.zeros(max(k, 1), dtype=np.int64)
    c4 = (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in ctr])
    k2 = (C.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in key])
    nxt = (C.c_uint32 * 4)()
    cnt, status = C.c_int64(0), C.c_int(0)
    rc = getattr(ctx.lib, f"rlhip_sample_indices_iid_{suf}")(ctx.h, int(d.numel()), d.data_ptr(), k, 1 if unique else 0, c4, k2, nxt,
                                                            out_dev.data_ptr(), out_host.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cnt),
                                                            C.byref(status))
    _lib.check(rc, "sample_indices_iid")
    m = int(cnt.value)
    return dict(S=out_host[:m].copy(), count=m, status=int(status.value), next_ctr=tuple(int(x) for x in nxt), S_dev=out_dev[:m])


def _rpchol_out(ctx, st, kk, S, F, status):
    kf = int(kk.value)
    return dict(F=F, S=S[:kf].copy(), k=kf, status=int(status[0]), c_status=int(status[1]), next_ctr=tuple(int(x) for x in st[:4]))


def drv_rpchol_rbf(ctx: Context, X, rows_x, n, bandwidth, k, b, reg=0.0, ctr=(0, 0, 0, 0), key=(0, 0)):
    """rp_cholesky on the RBF kernel matrix of the points X (column-major (n, rows_x)).  Returns dict(F (k_target, n) column-major -- only the
    first k columns are the factor --, S, k, status (w_status), c_status, next_ctr)."""
    torch = _torch()
    suf, _ = _suf(X)
    F = torch.zeros((k, n), dtype=X.dtype, device=X.device)
    S = np.full(max(k, 1), -1, dtype=np.int64)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    rc = getattr(ctx.lib, f"rlhip_drv_rpchol_rbf_{suf}")(ctx.h, X.data_ptr(), _ld(X), rows_x, n, bandwidth, reg, C.byref(kk), b,
                                                        S.ctypes.data_as(C.POINTER(C.c_int64)), F.data_ptr(), n, st, status)
    _drv_check(ctx, rc, "rpchol_rbf")
    return _rpchol_out(ctx, st, kk, S, F, status)


def drv_rpchol_pdk(ctx: Context, X, rows_x, n, kernel, bandwidth, k, b, reg=0.0, ctr=(0, 0, 0, 0), key=(0, 0)):
    """drv_rpchol_rbf for the kernel function `kernel` (PDK_*): the same dict"""
    torch = _torch()
    suf, _ = _suf(X)
    F = torch.zeros((k, n), dtype=X.dtype, device=X.device)
    S = np.full(max(k, 1), -1, dtype=np.int64)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    rc = getattr(ctx.lib, f"rlhip_drv_rpchol_pdk_{suf}")(ctx.h, X.data_ptr(), _ld(X), rows_x, n, kernel, bandwidth, reg, C.byref(kk), b,
                                                        S.ctypes.data_as(C.POINTER(C.c_int64)), F.data_ptr(), n, st, status)
    _drv_check(ctx, rc, "rpchol_pdk")
    return _rpchol_out(ctx, st, kk, S, F, status)


def drv_rpchol_dense(ctx: Context, A, n, k, b, ctr=(0, 0, 0, 0), key=(0, 0)):
    """rp_cholesky on the symmetric PSD matrix A (column-major (n, n) tensor).  Same dict as drv_rpchol_rbf."""
    torch = _torch()
    suf, _ = _suf(A)
    F = torch.zeros((k, n), dtype=A.dtype, device=A.device)
    S = np.full(max(k, 1), -1, dtype=np.int64)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    rc = getattr(ctx.lib, f"rlhip_drv_rpchol_dense_{suf}")(ctx.h, n, A.data_ptr(), _ld(A), C.byref(kk), b, S.ctypes.data_as(C.POINTER(C.c_int64)),
                                                          F.data_ptr(), n, st, status)
    _drv_check(ctx, rc, "rpchol_dense")
    return _rpchol_out(ctx, st, kk, S, F, status)


def rpchol_pc_data(ctx: Context, X, rows_x, n, bandwidth, k, b, reg=0.0, ctr=(0, 0, 0, 0), key=(0, 0)):
    """rpchol_pc_data on the RBF kernel matrix: dict(V (k, n) column-major, eigvals (k), k, next_ctr) with K ~ V diag(eigvals) V^T"""
    torch = _torch()
    suf, _ = _suf(X)
    V = torch.zeros((k, n), dtype=X.dtype, device=X.device)
    ev = torch.zeros(k, dtype=X.dtype, device=X.device)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_rpchol_pc_data_rbf_{suf}")(ctx.h, X.data_ptr(), _ld(X), rows_x, n, bandwidth, reg, C.byref(kk), b,
                                                                V.data_ptr(), ev.data_ptr(), st)
    _drv_check(ctx, rc, "rpchol_pc_data")
    kf = int(kk.value)
    return dict(V=V[:kf], eigvals=ev[:kf], k=kf, next_ctr=tuple(int(x) for x in st[:4]))


# ---- block / lockstep PCG, the spectral preconditioner and KRILL (pcg.hip; include/RandLAPACK_amd/rl_determiter.hh, rl_krill.hh).
#      Blocks are column-major tensors (s, ld) as everywhere in this module; s x s matrices are (s, s) tensors with ld s.
def _ldc(t):
    """leading dimension of a column-major block (cols, ld): a one-column block says nothing through its strides, its row length does"""
    return int(t.shape[1]) if t.dim() == 2 and t.shape[0] == 1 else _ld(t)


def posm_square(ctx: Context, LHS, RHS, diag_only=False, host_fallback=False):
    """RHS <- LHS^-1 RHS in place for the s x s pair.  host_fallback False: the device attempt alone, returns its status (s, or -1 with both
    matrices untouched).  True: the C++ posm_square (eigenvalue fallback on the host after a failed pivot), returns the rank or -(s+1) / -(s+2)."""
    torch = _torch()
    suf, _ = _suf(LHS)
    s = int(LHS.shape[0])
    if host_fallback:
        code = C.c_int64(0)
        rc = getattr(ctx.lib, f"rlhip_drv_posm_square_{suf}")(ctx.h, s, LHS.data_ptr(), RHS.data_ptr(), 1 if diag_only else 0, C.byref(code))
        _drv_check(ctx, rc, "posm_square")
        return int(code.value)
    st = torch.zeros(1, dtype=torch.int64, device=LHS.device)
    _lib.check(getattr(ctx.lib, f"rlhip_posm_square_{suf}")(ctx.h, s, LHS.data_ptr(), RHS.data_ptr(), 1 if diag_only else 0, st.data_ptr()),
               "posm_square")
    return int(st.item())


def pcg_update_xr(ctx: Context, n, s, alpha, P, GP, X, R, want_norms=True):
    """X += P alpha, R -= GP alpha in place; returns the squared column norms of the new R (float64 tensor, s) or None"""
    torch = _torch()
    suf, _ = _suf(P)
    cn = torch.zeros(s, dtype=torch.float64, device=P.device) if want_norms else None
    rc = getattr(ctx.lib, f"rlhip_pcg_update_xr_{suf}")(ctx.h, n, s, alpha.data_ptr(), P.data_ptr(), _ldc(P), GP.data_ptr(), _ldc(GP), X.data_ptr(), _ldc(X),
                                                       R.data_ptr(), _ldc(R), None if cn is None else cn.data_ptr())
    _lib.check(rc, "pcg_update_xr")
    return cn


def pcg_update_p(ctx: Context, n, s, beta, NR, P):
    """P <- NR + P beta in place"""
    suf, _ = _suf(P)
    _lib.check(getattr(ctx.lib, f"rlhip_pcg_update_p_{suf}")(ctx.h, n, s, beta.data_ptr(), NR.data_ptr(), _ldc(NR), P.data_ptr(), _ldc(P)), "pcg_update_p")
    return P


def spectral_precond_apply(ctx: Context, V, D, B, dim, n, alpha=1.0, beta=0.0, C_=None, want_norms=True):
    """C = alpha (V diag(D_j) V^T + I) B + beta C.  V (dim_pre, ldv), D (num_ops, dim_pre), B (n, ldb), C_ (n, ldc) column-major.
    Returns (C, squared column norms of C as a float64 tensor or None)."""
    torch = _torch()
    suf, _ = _suf(V)
    dim_pre, num_ops = int(V.shape[0]), int(D.shape[0])
    if C_ is None:
        C_ = torch.zeros((n, dim), dtype=V.dtype, device=V.device)
    W = torch.empty((n, max(dim_pre, 1)), dtype=V.dtype, device=V.device)
    cn = torch.zeros(n, dtype=torch.float64, device=V.device) if want_norms else None
    rc = getattr(ctx.lib, f"rlhip_spectral_precond_apply_{suf}")(ctx.h, dim, dim_pre, V.data_ptr(), _ldc(V), D.data_ptr(), num_ops, n, alpha, B.data_ptr(),
                                                                _ldc(B), beta, C_.data_ptr(), _ldc(C_), W.data_ptr(), None if cn is None else cn.data_ptr())
    _lib.check(rc, "spectral_precond_apply")
    return C_, cn


def _pcg_out(X, iters, hist):
    it = int(iters.value)
    h = np.array(hist[: 2 * (it + 1)], dtype=np.float64).reshape(-1, 2)
    h = h[~np.isnan(h[:, 0])]              # (an iteration that ended at its alpha solve recorded no norms)
    return dict(X=X, iters=it, normR=h[:, 0].copy(), normNR=h[:, 1].copy())


def _pcg_args(T, regs, max_iters):
    rg = (T * len(regs))(*regs)
    hist = (T * (2 * (max_iters + 1)))(*([float("nan")] * (2 * (max_iters + 1))))
    return rg, hist, C.c_int64(0)


def pcg_dense(ctx: Context, A, n, regs, V, eigvals, H, X, s, tol, max_iters):
    """pcg on (A + mu_i I) X = H with the spectral preconditioner from (V, eigvals); A (n, lda) column-major, its upper triangle is read.  X is the
    starting point and is overwritten.  Returns dict(X, iters, normR, normNR): the norms of iterations 0 .. iters that were recorded."""
    suf, T = _suf(A)
    rg, hist, iters = _pcg_args(T, regs, max_iters)
    rc = getattr(ctx.lib, f"rlhip_drv_pcg_dense_{suf}")(ctx.h, n, A.data_ptr(), _ldc(A), rg, len(regs), V.data_ptr(), _ldc(V), eigvals.data_ptr(),
                                                       int(eigvals.numel()), H.data_ptr(), X.data_ptr(), s, tol, max_iters, C.byref(iters), hist)
    _drv_check(ctx, rc, "pcg_dense")
    return _pcg_out(X, iters, hist)


def pcg_rbf(ctx: Context, Xp, rows_x, n, bandwidth, regs, V, eigvals, H, X, s, tol, max_iters):
    """pcg_dense over the RBF kernel matrix of the points Xp (column-major (n, rows_x))"""
    suf, T = _suf(Xp)
    rg, hist, iters = _pcg_args(T, regs, max_iters)
    rc = getattr(ctx.lib, f"rlhip_drv_pcg_rbf_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, bandwidth, rg, len(regs), V.data_ptr(), _ldc(V),
                                                     eigvals.data_ptr(), int(eigvals.numel()), H.data_ptr(), X.data_ptr(), s, tol, max_iters,
                                                     C.byref(iters), hist)
    _drv_check(ctx, rc, "pcg_rbf")
    return _pcg_out(X, iters, hist)


def krill_full_rpchol_rbf(ctx: Context, Xp, rows_x, n, bandwidth, regs, H, X, s, tol, max_iters, k=-1, b=-1, ctr=(0, 0, 0, 0), key=(0, 0)):
    """krill_full_rpchol on the RBF kernel matrix: dict(X, iters, normR, normNR, k, next_ctr)"""
    suf, T = _suf(Xp)
    rg, hist, iters = _pcg_args(T, regs, max_iters)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_full_rpchol_rbf_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, bandwidth, rg, len(regs), H.data_ptr(),
                                                                   X.data_ptr(), s, tol, max_iters, C.byref(kk), b, st, C.byref(iters), hist)
    _drv_check(ctx, rc, "krill_full_rpchol_rbf")
    out = _pcg_out(X, iters, hist)
    out.update(k=int(kk.value), next_ctr=tuple(int(x) for x in st[:4]))
    return out


def krill_full_rpchol_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, regs, H, X, s, tol, max_iters, k=-1, b=-1, ctr=(0, 0, 0, 0), key=(0, 0)):
    """krill_full_rpchol_rbf for the kernel function `kernel` (PDK_*): the same dict"""
    suf, T = _suf(Xp)
    rg, hist, iters = _pcg_args(T, regs, max_iters)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_full_rpchol_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, rg, len(regs),
                                                                   H.data_ptr(), X.data_ptr(), s, tol, max_iters, C.byref(kk), b, st, C.byref(iters),
                                                                   hist)
    _drv_check(ctx, rc, "krill_full_rpchol_pdk")
    out = _pcg_out(X, iters, hist)
    out.update(k=int(kk.value), next_ctr=tuple(int(x) for x in st[:4]))
    return out


# ---- restricted kernel ridge regression (include/RandLAPACK_amd/rl_krill.hh): k centres among the n training points, k
#      coefficients per right-hand side.  H (s, ldh >= n) and alpha (s, ldalpha >= k) are column-major blocks as everywhere in this module.
def ridge_filter(ctx: Context, sigma, mus, C_, k, s, rcond=0.0, ldc=None):
    """C(j, i) *= sigma[j] / (sigma[j]^2 + mus[len(mus) == 1 ? 0 : i]) in place on the k x s block C_ (rlhip_ridge_filter_*); mu == 0 cuts
    sigma[j] <= rcond sigma[0] to an exact 0.  Returns C_."""
    suf, _ = _suf(C_)
    rc = getattr(ctx.lib, f"rlhip_ridge_filter_{suf}")(ctx.h, k, s, _ptr(sigma), _ptr(mus), int(mus.numel()), rcond, C_.data_ptr(),
                                                      _ldc(C_) if ldc is None else ldc)
    _lib.check(rc, "ridge_filter")
    return C_


def krill_restricted_rpchol_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, regs, H, s, k=-1, b=-1, ctr=(0, 0, 0, 0), key=(0, 0), ldalpha=None):
    """krill_restricted_rpchol over the kernel matrix of the points Xp with the kernel function `kernel` (PDK_*): dict(alpha (s, ldalpha)
    column-major with zero rows behind the achieved rank, S (numpy, the centres in selection order), k, status, c_status, next_ctr)"""
    torch = _torch()
    suf, T = _suf(Xp)
    k_in = int(np.sqrt(n)) if k < 0 else k
    lda = max(k_in, 1) if ldalpha is None else ldalpha
    alpha = torch.full((s, lda), float("nan"), dtype=Xp.dtype, device=Xp.device)
    S = np.full(max(k_in, 1), -1, dtype=np.int64)
    rg = (T * len(regs))(*regs)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_rpchol_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, rg, len(regs),
                                                                         H.data_ptr(), _ldc(H), s, C.byref(kk), b,
                                                                         S.ctypes.data_as(C.POINTER(C.c_int64)), alpha.data_ptr(), lda, st, status)
    _drv_check(ctx, rc, "krill_restricted_rpchol_pdk")
    kf = int(kk.value)
    return dict(alpha=alpha, S=S[:kf].copy(), S_all=S, k=kf, status=int(status[0]), c_status=int(status[1]), next_ctr=tuple(int(x) for x in st[:4]))


def krill_restricted_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, regs, H, s, S, alpha=None):
    """krill_restricted with the centres S (a sequence of distinct point indices): (info, alpha).  info = 0, or the 1-based position of the
    first centre that depends on the ones before it -- then alpha is as it was handed in."""
    torch = _torch()
    suf, T = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    k = int(S.size)
    if alpha is None:
        alpha = torch.full((s, max(k, 1)), float("nan"), dtype=Xp.dtype, device=Xp.device)
    rg = (T * len(regs))(*regs)
    info = C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, rg, len(regs),
                                                                  H.data_ptr(), _ldc(H), s, k, S.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                  alpha.data_ptr(), _ldc(alpha), C.byref(info))
    _drv_check(ctx, rc, "krill_restricted_pdk")
    return int(info.value), alpha


def krr_predict_restricted_pdk(ctx: Context, Z, mz, Xp, rows_x, n, kernel, bandwidth, S, alpha, s):
    """krr_predict_restricted: Y (mz x s) = K(Z, Xp(:, S)) alpha for the k = len(S) centres and the k x s block alpha; column-major (s, mz)"""
    torch = _torch()
    suf, _ = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    Y = torch.zeros((s, mz), dtype=Xp.dtype, device=Xp.device)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_restricted_pdk_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), kernel,
                                                                        bandwidth, int(S.size), S.ctypes.data_as(C.POINTER(C.c_int64)), s,
                                                                        alpha.data_ptr(), max(_ldc(alpha), 1), Y.data_ptr(), max(mz, 1))
    _drv_check(ctx, rc, "krr_predict_restricted_pdk")
    return Y


# ---- the regularization path of the restricted fits: leave-one-out and residual sums for a grid of regularizations after one
#      factorization and one SVD, and the fits that choose from the grid
CV_LOO, CV_GCV = 0, 1


def ridge_loo(ctx: Context, U, sigma, C_, H, mus, n, k, ell, rcond=0.0, ldu=None, ldc=None, ldh=None):
    """(loo, rss) of rlhip_ridge_loo_*: float64 device tensors (ell, g), column-major g x ell.  U (k, ldu >= n), C_ (ell, ldc >= k) and
    H (ell, ldh >= n) are column-major blocks, sigma (k) and mus (g) vectors, all of one dtype."""
    torch = _torch()
    suf, _ = _suf(U)
    g = int(mus.numel())
    loo = torch.full((ell, g), float("nan"), dtype=torch.float64, device=U.device)
    rss = torch.full((ell, g), float("nan"), dtype=torch.float64, device=U.device)
    rc = getattr(ctx.lib, f"rlhip_ridge_loo_{suf}")(ctx.h, n, k, ell, g, U.data_ptr(), _ldc(U) if ldu is None else ldu, _ptr(sigma), C_.data_ptr(),
                                                   _ldc(C_) if ldc is None else ldc, H.data_ptr(), _ldc(H) if ldh is None else ldh, _ptr(mus), rcond,
                                                   loo.data_ptr(), rss.data_ptr())
    _lib.check(rc, "ridge_loo")
    return loo, rss


def _path_buffers(g, s):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    bufs = dict(loo=np.full((s, g), np.nan), rss=np.full((s, g), np.nan), dof=np.full(g, np.nan), best=np.full(s, -1, dtype=np.int64),
                best_mu=np.full(s, np.nan))
    ptrs = [bufs[name].ctypes.data_as(ip if name == "best" else dp) for name in ("loo", "rss", "dof", "best", "best_mu")]
    return bufs, ptrs


def krill_restricted_rpchol_cv_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, mu_grid, criterion, H, s, k=-1, b=-1, ctr=(0, 0, 0, 0), key=(0, 0),
                                   ldalpha=None):
    """krill_restricted_rpchol_cv: the dict of krill_restricted_rpchol_pdk and the path on the host -- loo, rss (numpy (s, g): row c is
    column c of the g x s table), dof (g), best (s indices into mu_grid), best_mu (s).  criterion: CV_LOO or CV_GCV."""
    torch = _torch()
    suf, T = _suf(Xp)
    k_in = int(np.sqrt(n)) if k < 0 else k
    lda = max(k_in, 1) if ldalpha is None else ldalpha
    alpha = torch.full((s, lda), float("nan"), dtype=Xp.dtype, device=Xp.device)
    S = np.full(max(k_in, 1), -1, dtype=np.int64)
    g = len(mu_grid)
    mg = (T * max(g, 1))(*mu_grid)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    bufs, ptrs = _path_buffers(max(g, 1), s)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_rpchol_cv_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, mg, g, criterion,
                                                                            H.data_ptr(), _ldc(H), s, C.byref(kk), b,
                                                                            S.ctypes.data_as(C.POINTER(C.c_int64)), alpha.data_ptr(), lda, st, status, *ptrs)
    _drv_check(ctx, rc, "krill_restricted_rpchol_cv_pdk")
    kf = int(kk.value)
    return dict(bufs, alpha=alpha, S=S[:kf].copy(), S_all=S, k=kf, status=int(status[0]), c_status=int(status[1]),
                next_ctr=tuple(int(x) for x in st[:4]))


def krill_restricted_cv_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, mu_grid, criterion, H, s, S, alpha=None):
    """krill_restricted_cv with the centres S: (info, alpha, path) with path = dict(loo, rss, dof, best, best_mu) as above; with info != 0
    alpha and the path are as they were handed in (the path: NaN and -1)."""
    torch = _torch()
    suf, T = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    k = int(S.size)
    if alpha is None:
        alpha = torch.full((s, max(k, 1)), float("nan"), dtype=Xp.dtype, device=Xp.device)
    g = len(mu_grid)
    mg = (T * max(g, 1))(*mu_grid)
    info = C.c_int64(0)
    bufs, ptrs = _path_buffers(max(g, 1), s)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_cv_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, mg, g, criterion,
                                                                     H.data_ptr(), _ldc(H), s, k, S.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                     alpha.data_ptr(), _ldc(alpha), C.byref(info), *ptrs)
    _drv_check(ctx, rc, "krill_restricted_cv_pdk")
    return int(info.value), alpha, bufs


# ---- the predictive variance of the restricted fits (rbf_var.hip, rl_krill.hh): the fits that keep their basis, and the
#      variance at new points from it.  G (k, ldg) is a column-major k x k block, V (s, ldv) a column-major mz x s block.
def pdk_cross_var(ctx: Context, Z, mz, Xs, rows_x, k, kernel, bandwidth, G, sigma, mus, s, rcond=0.0, V=None, ldz=None, ldx=None, ldg=None, ldv=None):
    """V(i, c) = max(0, 1 - sum_j t_ij^2) + sum_j mus_c / (sigma_j^2 + mus_c) t_ij^2 with t = K(Z, Xs) G (rlhip_pdk_cross_var_*).  Z (mz, ldz)
    and Xs (k, ldx) are point sets, sigma (k) and mus (1 or s) device vectors.  Returns V (s, ldv)."""
    torch = _torch()
    suf, _ = _suf(Z)
    if V is None:
        V = torch.full((max(s, 1), max(mz, 1) if ldv is None else ldv), float("nan"), dtype=Z.dtype, device=Z.device)
    rc = getattr(ctx.lib, f"rlhip_pdk_cross_var_{suf}")(ctx.h, rows_x, mz, _ptr(Z), (_ldc(Z) if Z is not None else rows_x) if ldz is None else ldz, k, _ptr(Xs),
                                                       (_ldc(Xs) if Xs is not None else rows_x) if ldx is None else ldx, kernel, bandwidth, _ptr(G),
                                                       (max(_ldc(G), 1) if G is not None else max(k, 1)) if ldg is None else ldg, _ptr(sigma), s,
                                                       _ptr(mus), int(mus.numel()) if mus is not None else 1, rcond, V.data_ptr(),
                                                       _ldc(V) if ldv is None else ldv)
    _lib.check(rc, "pdk_cross_var")
    return V


def _basis_buffers(torch, k_in, like, ldg):
    ldg = max(k_in, 1) if ldg is None else ldg
    G = torch.full((max(k_in, 1), ldg), float("nan"), dtype=like.dtype, device=like.device)
    sigma = torch.full((max(k_in, 1),), float("nan"), dtype=like.dtype, device=like.device)
    return G, sigma, ldg


def krill_restricted_rpchol_gp_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, regs, H, s, k=-1, b=-1, ctr=(0, 0, 0, 0), key=(0, 0), ldalpha=None,
                                   ldg=None):
    """krill_restricted_rpchol_pdk that keeps the fit's basis: the same dict and G (k_in, ldg), sigma (k_in) on the device, zero behind the
    achieved rank"""
    torch = _torch()
    suf, T = _suf(Xp)
    k_in = int(np.sqrt(n)) if k < 0 else k
    lda = max(k_in, 1) if ldalpha is None else ldalpha
    alpha = torch.full((s, lda), float("nan"), dtype=Xp.dtype, device=Xp.device)
    G, sigma, ldg = _basis_buffers(torch, k_in, Xp, ldg)
    S = np.full(max(k_in, 1), -1, dtype=np.int64)
    rg = (T * len(regs))(*regs)
    kk = C.c_int64(k)
    st = _state_arr(ctr, key)
    status = (C.c_int * 2)()
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_rpchol_gp_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, rg, len(regs),
                                                                            H.data_ptr(), _ldc(H), s, C.byref(kk), b,
                                                                            S.ctypes.data_as(C.POINTER(C.c_int64)), alpha.data_ptr(), lda, st, status,
                                                                            G.data_ptr(), ldg, sigma.data_ptr())
    _drv_check(ctx, rc, "krill_restricted_rpchol_gp_pdk")
    kf = int(kk.value)
    return dict(alpha=alpha, S=S[:kf].copy(), S_all=S, k=kf, status=int(status[0]), c_status=int(status[1]), next_ctr=tuple(int(x) for x in st[:4]),
                G=G, sigma=sigma)


def krill_restricted_gp_pdk(ctx: Context, Xp, rows_x, n, kernel, bandwidth, regs, H, s, S, alpha=None):
    """krill_restricted_pdk that keeps the fit's basis: (info, alpha, G (k, k), sigma (k)); with info != 0 all three are as handed in (NaN)"""
    torch = _torch()
    suf, T = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    k = int(S.size)
    if alpha is None:
        alpha = torch.full((s, max(k, 1)), float("nan"), dtype=Xp.dtype, device=Xp.device)
    G, sigma, ldg = _basis_buffers(torch, k, Xp, None)
    rg = (T * len(regs))(*regs)
    info = C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_krill_restricted_gp_pdk_{suf}")(ctx.h, Xp.data_ptr(), _ldc(Xp), rows_x, n, kernel, bandwidth, rg, len(regs),
                                                                     H.data_ptr(), _ldc(H), s, k, S.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                     alpha.data_ptr(), _ldc(alpha), C.byref(info), G.data_ptr(), ldg, sigma.data_ptr())
    _drv_check(ctx, rc, "krill_restricted_gp_pdk")
    return int(info.value), alpha, G, sigma


def krr_predict_restricted_var_pdk(ctx: Context, Z, mz, Xp, rows_x, n, kernel, bandwidth, S, G, sigma, mus, s, fused_kernel=False):
    """krr_predict_restricted_var: V (mz x s), column-major (s, mz), for the k = len(S) centres, their fit's basis (G, sigma) and the
    regularizations mus (a host sequence of 1 or s values); fused_kernel: ask for the fused kernel of rlhip_pdk_cross_var_*"""
    torch = _torch()
    suf, T = _suf(Xp)
    S = np.ascontiguousarray(S, dtype=np.int64)
    V = torch.full((max(s, 1), max(mz, 1)), float("nan"), dtype=Xp.dtype, device=Xp.device)
    mh = (T * max(len(mus), 1))(*mus)
    rc = getattr(ctx.lib, f"rlhip_drv_krr_predict_restricted_var_pdk_{suf}")(ctx.h, rows_x, mz, Z.data_ptr(), _ld(Z), n, Xp.data_ptr(), _ld(Xp), kernel,
                                                                            bandwidth, int(S.size), S.ctypes.data_as(C.POINTER(C.c_int64)), G.data_ptr(),
                                                                            max(_ldc(G), 1), sigma.data_ptr(), s, mh, len(mus), V.data_ptr(), max(mz, 1),
                                                                            int(bool(fused_kernel)))
    _drv_check(ctx, rc, "krr_predict_restricted_var_pdk")
    return V


# ---- matrix-vector layer, pcg_saddle and the sketched least-squares preconditioners (lsq.hip; include/RandLAPACK_amd/rl_determiter.hh,
#      rl_preconditioners.hh, rl_lstsq.hh).  A matrix is a column-major tensor (cols, ld) as everywhere in this module, a vector a 1-D tensor
#      that may be longer than the length in use.
def _ptr(t):
    return None if t is None else t.data_ptr()


def gemv(ctx: Context, trans, m, n, alpha, A, x, beta, y, lda=None):
    """y = alpha op(A) x + beta y in place (rlhip_gemv_*); A (n, lda) column-major"""
    suf, _ = _suf(y)
    rc = getattr(ctx.lib, f"rlhip_gemv_{suf}")(ctx.h, trans.encode(), m, n, alpha, _ptr(A), _ldc(A) if lda is None else lda, _ptr(x), beta, _ptr(y))
    _lib.check(rc, "gemv")
    return y


def normal_matvec(ctx: Context, m, n, A, d, delta, q, t=None, want_dq=False, max_wg=0, lda=None):
    """q = A^T (A d) + delta d (rlhip_normal_matvec_*); t (optional, m values) receives A d.  Returns d^T q as a one-element device tensor when
    want_dq, else None."""
    torch = _torch()
    suf, _ = _suf(q)
    dq = torch.zeros(1, dtype=q.dtype, device=q.device) if want_dq else None
    rc = getattr(ctx.lib, f"rlhip_normal_matvec_{suf}")(ctx.h, m, n, _ptr(A), _ldc(A) if lda is None else lda, _ptr(d), delta, _ptr(q), _ptr(t), _ptr(dq),
                                                       max_wg)
    _lib.check(rc, "normal_matvec")
    return dq


def pcg_saddle(ctx: Context, A, m, n, b, c, delta, iter_lim, tol, M, k, x0, lda=None, ldm=None):
    """pcg_saddle on DEVICE operands: (A'A + delta I) x = A'b - c preconditioned with M M' (M (k, ldm) column-major).
    Returns dict(x, y, iters, resid (numpy, iters + 1 entries))."""
    torch = _torch()
    suf, _ = _suf(A)
    x = torch.zeros(n, dtype=A.dtype, device=A.device)
    y = torch.zeros(m, dtype=A.dtype, device=A.device)
    resid = torch.full((iter_lim + 1,), float("nan"), dtype=A.dtype, device=A.device)
    iters = C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_pcg_saddle_{suf}")(ctx.h, m, n, A.data_ptr(), _ldc(A) if lda is None else lda, b.data_ptr(), c.data_ptr(), delta,
                                                        iter_lim, resid.data_ptr(), tol, k, M.data_ptr(), _ldc(M) if ldm is None else ldm,
                                                        x0.data_ptr(), x.data_ptr(), y.data_ptr(), C.byref(iters))
    _drv_check(ctx, rc, "pcg_saddle")
    it = int(iters.value)
    return dict(x=x, y=y, iters=it, resid=resid[: it + 1].cpu().numpy())


def rpc_data_svd_saso(ctx: Context, A, m, n, d, nnz, ctr=(0, 0, 0, 0), key=(0, 0), lda=None):
    """rpc_data_svd_saso: dict(V (n, n) column-major right singular vectors of the sketch, sigma (n), next_ctr)"""
    torch = _torch()
    suf, _ = _suf(A)
    V_sk = torch.zeros(max(d * n, 1), dtype=A.dtype, device=A.device)
    sigma = torch.zeros(n, dtype=A.dtype, device=A.device)
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_rpc_data_svd_saso_{suf}")(ctx.h, m, n, d, nnz, A.data_ptr(), _ldc(A) if lda is None else lda, V_sk.data_ptr(),
                                                               sigma.data_ptr(), st)
    _drv_check(ctx, rc, "rpc_data_svd_saso")
    return dict(V=V_sk[: n * n].view(n, n), sigma=sigma, next_ctr=tuple(int(v) for v in st[:4]))


def make_right_orthogonalizer(ctx: Context, V, sigma, mu, cols_V=-1):
    """scales the leading columns of V (n, n) in place; returns the rank"""
    suf, _ = _suf(V)
    rank = C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_make_right_orthogonalizer_{suf}")(ctx.h, int(V.shape[1]), V.data_ptr(), sigma.data_ptr(), mu, cols_V, C.byref(rank))
    _drv_check(ctx, rc, "make_right_orthogonalizer")
    return int(rank.value)


def sap_lstsq(ctx: Context, A, m, n, b, c, delta, d_factor, nnz, tol, iter_lim, ctr=(0, 0, 0, 0), key=(0, 0), lda=None):
    """sap_lstsq: dict(x, y, rank, iters, resid (numpy), next_ctr)"""
    torch = _torch()
    suf, _ = _suf(A)
    x = torch.zeros(n, dtype=A.dtype, device=A.device)
    y = torch.zeros(m, dtype=A.dtype, device=A.device)
    resid = torch.full((iter_lim + 1,), float("nan"), dtype=A.dtype, device=A.device)
    st = _state_arr(ctr, key)
    rank, iters = C.c_int64(0), C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_sap_lstsq_{suf}")(ctx.h, m, n, A.data_ptr(), _ldc(A) if lda is None else lda, b.data_ptr(), c.data_ptr(), delta,
                                                       d_factor, nnz, tol, iter_lim, x.data_ptr(), y.data_ptr(), resid.data_ptr(), st,
                                                       C.byref(rank), C.byref(iters))
    _drv_check(ctx, rc, "sap_lstsq")
    it = int(iters.value)
    return dict(x=x, y=y, rank=int(rank.value), iters=it, resid=resid[: it + 1].cpu().numpy(), next_ctr=tuple(int(v) for v in st[:4]))


# ---- several right-hand sides (lsq.hip, rl_determiter.hh pcg_saddle_block, rl_lstsq.hh).  A block of s vectors is a
#      column-major tensor (s, ld) like a matrix.
def normal_matmat_fused(n, s, elem_bytes):
    """the chunk width rlhip_normal_matmat_*'s one-pass route uses for this shape, 0 outside its limits (no device needed)"""
    return int(_lib.load().rlhip_normal_matmat_fused(n, s, elem_bytes))


def normal_matmat_default(n, s, elem_bytes):
    """1 where rlhip_normal_matmat_* takes its one-pass route unasked (the ranges in which it measured faster), else 0 (no device needed)"""
    return int(_lib.load().rlhip_normal_matmat_default(n, s, elem_bytes))


def normal_matmat(ctx: Context, m, n, s, A, D, delta, Q, T=None, want_dq=False, max_wg=0, lda=None, ldd=None, ldq=None, ldt=None):
    """Q = A^T (A D) + delta D on s columns (rlhip_normal_matmat_*); T (optional, m x s) receives A D.  Returns the s values d_j^T q_j as a
    device tensor when want_dq, else None."""
    torch = _torch()
    suf, _ = _suf(Q)
    dq = torch.zeros(max(s, 1), dtype=Q.dtype, device=Q.device) if want_dq else None
    rc = getattr(ctx.lib, f"rlhip_normal_matmat_{suf}")(ctx.h, m, n, s, _ptr(A), _ldc(A) if lda is None else lda, _ptr(D), _ldc(D) if ldd is None else ldd,
                                                       delta, _ptr(Q), _ldc(Q) if ldq is None else ldq, _ptr(T),
                                                       (_ldc(T) if T is not None else max(m, 1)) if ldt is None else ldt, _ptr(dq), max_wg)
    _lib.check(rc, "normal_matmat")
    return None if dq is None else dq[:s]


def pcg_saddle_block(ctx: Context, A, m, n, s, B, Cm, delta, iter_lim, tol, M, k, X0=None, lda=None, ldm=None, resid=None):
    """pcg_saddle_block on DEVICE operands: B (s, ldb), Cm (s, ldc) or None, X0 (s, ldx0) or None.  resid (optional): a device tensor
    (s, iter_lim + 1) that receives the residual histories (entries a column does not reach are left as they are).
    Returns dict(x (s, n), y (s, m), iters (list), resid (numpy (s, iter_lim + 1)))."""
    torch = _torch()
    suf, _ = _suf(A)
    X = torch.zeros((max(s, 1), n), dtype=A.dtype, device=A.device)
    Y = torch.zeros((max(s, 1), m), dtype=A.dtype, device=A.device)
    if resid is None:
        resid = torch.full((max(s, 1), iter_lim + 1), float("nan"), dtype=A.dtype, device=A.device)
    iters = (C.c_int64 * max(s, 1))()
    rc = getattr(ctx.lib, f"rlhip_drv_pcg_saddle_block_{suf}")(ctx.h, m, n, A.data_ptr(), _ldc(A) if lda is None else lda, s, _ptr(B),
                                                              _ldc(B) if B is not None else m, _ptr(Cm), _ldc(Cm) if Cm is not None else n, delta, iter_lim, resid.data_ptr(), _ldc(resid), tol, k,
                                                              M.data_ptr(), _ldc(M) if ldm is None else ldm, _ptr(X0), _ldc(X0) if X0 is not None else n,
                                                              X.data_ptr(), n, Y.data_ptr(), m, iters)
    _drv_check(ctx, rc, "pcg_saddle_block")
    return dict(x=X[:s], y=Y[:s], iters=[int(v) for v in iters[:s]], resid=resid[:s].cpu().numpy())


def sap_lstsq_block(ctx: Context, A, m, n, s, B, Cm, delta, d_factor, nnz, tol, iter_lim, ctr=(0, 0, 0, 0), key=(0, 0), lda=None):
    """sap_lstsq with s right-hand sides: one preconditioner, pcg_saddle_block from X0 = 0.  B (s, ldb), Cm (s, ldc) or None.
    Returns dict(x (s, n), y (s, m), rank, iters (list), resid (numpy (s, iter_lim + 1), NaN where a column did not reach), next_ctr)."""
    torch = _torch()
    suf, _ = _suf(A)
    X = torch.zeros((max(s, 1), n), dtype=A.dtype, device=A.device)
    Y = torch.zeros((max(s, 1), m), dtype=A.dtype, device=A.device)
    resid = torch.full((max(s, 1), iter_lim + 1), float("nan"), dtype=A.dtype, device=A.device)
    st = _state_arr(ctr, key)
    rank = C.c_int64(0)
    iters = (C.c_int64 * max(s, 1))()
    rc = getattr(ctx.lib, f"rlhip_drv_sap_lstsq_block_{suf}")(ctx.h, m, n, A.data_ptr(), _ldc(A) if lda is None else lda, s, _ptr(B),
                                                             _ldc(B) if B is not None else m, _ptr(Cm), _ldc(Cm) if Cm is not None else n, delta, d_factor,
                                                             nnz, tol, iter_lim, X.data_ptr(), n, Y.data_ptr(), m, resid.data_ptr(), st, C.byref(rank), iters)
    _drv_check(ctx, rc, "sap_lstsq_block")
    return dict(x=X[:s], y=Y[:s], rank=int(rank.value), iters=[int(v) for v in iters[:s]], resid=resid[:s].cpu().numpy(),
                next_ctr=tuple(int(v) for v in st[:4]))


# ---- the sparse matrix-vector layer (spmv.hip) and least squares over an operator (DenseOperator, CsrOperator, CscOperator, CooOperator)
def csr_spmv(ctx: Context, nrows, ncols, rowptr, colidx, vals, alpha, x, beta, y):
    """y = alpha A x + beta y in place for the nrows x ncols CSR (rowptr, colidx, vals) (rlhip_csr_spmv_*); the transposed product is the
    same call on the transpose's CSR"""
    suf, _ = _suf(y)
    rc = getattr(ctx.lib, f"rlhip_csr_spmv_{suf}")(ctx.h, nrows, ncols, int(vals.numel()), _ptr(rowptr), _ptr(colidx), _ptr(vals), alpha, _ptr(x), beta,
                                                  _ptr(y))
    _lib.check(rc, "csr_spmv")
    return y


def csr_normal_matvec(ctx: Context, m, n, csr, csr_t, d, delta, q, t=None, want_dq=False, max_wg=0):
    """q = A^T (A d) + delta d (rlhip_csr_normal_matvec_*) for A given as csr = (rowptr, colidx, vals) and csr_t, the same of its
    transpose; t (optional, m values) receives A d.  Returns d^T q as a one-element device tensor when want_dq, else None."""
    torch = _torch()
    suf, _ = _suf(q)
    dq = torch.zeros(1, dtype=q.dtype, device=q.device) if want_dq else None
    rc = getattr(ctx.lib, f"rlhip_csr_normal_matvec_{suf}")(ctx.h, m, n, int(csr[2].numel()), _ptr(csr[0]), _ptr(csr[1]), _ptr(csr[2]), _ptr(csr_t[0]),
                                                           _ptr(csr_t[1]), _ptr(csr_t[2]), _ptr(d), delta, _ptr(q), _ptr(t), _ptr(dq), max_wg)
    _lib.check(rc, "csr_normal_matvec")
    return dq


def _single_op_descs(op):
    ld, rd, m, n, dtype = _op_descs(op)
    return C.byref(ld), (C.byref(rd) if rd is not None else None), m, n, dtype, (ld, rd)


def pcg_saddle_op(ctx: Context, op, b, c, delta, iter_lim, tol, M, k, x0, ldm=None):
    """pcg_saddle on an operator: same outputs as pcg_saddle"""
    torch = _torch()
    lp, rp, m, n, dtype, _keep = _single_op_descs(op)
    suf = "f64" if dtype == torch.float64 else "f32"
    dev = f"cuda:{ctx.device}"
    x = torch.zeros(n, dtype=dtype, device=dev)
    y = torch.zeros(m, dtype=dtype, device=dev)
    resid = torch.full((iter_lim + 1,), float("nan"), dtype=dtype, device=dev)
    iters = C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_pcg_saddle_linop_{suf}")(ctx.h, lp, rp, b.data_ptr(), c.data_ptr(), delta, iter_lim, resid.data_ptr(), tol, k,
                                                              M.data_ptr(), _ldc(M) if ldm is None else ldm, x0.data_ptr(), x.data_ptr(), y.data_ptr(),
                                                              C.byref(iters))
    _drv_check(ctx, rc, "pcg_saddle_op")
    it = int(iters.value)
    return dict(x=x, y=y, iters=it, resid=resid[: it + 1].cpu().numpy())


def rpc_data_svd_saso_op(ctx: Context, op, d, nnz, ctr=(0, 0, 0, 0), key=(0, 0)):
    """rpc_data_svd_saso on an operator: same outputs as rpc_data_svd_saso"""
    torch = _torch()
    lp, rp, m, n, dtype, _keep = _single_op_descs(op)
    suf = "f64" if dtype == torch.float64 else "f32"
    dev = f"cuda:{ctx.device}"
    V_sk = torch.zeros(max(d * n, 1), dtype=dtype, device=dev)
    sigma = torch.zeros(n, dtype=dtype, device=dev)
    st = _state_arr(ctr, key)
    rc = getattr(ctx.lib, f"rlhip_drv_rpc_data_svd_saso_linop_{suf}")(ctx.h, lp, rp, d, nnz, V_sk.data_ptr(), sigma.data_ptr(), st)
    _drv_check(ctx, rc, "rpc_data_svd_saso_op")
    return dict(V=V_sk[: n * n].view(n, n), sigma=sigma, next_ctr=tuple(int(v) for v in st[:4]))


def sap_lstsq_op(ctx: Context, op, b, c, delta, d_factor, nnz, tol, iter_lim, ctr=(0, 0, 0, 0), key=(0, 0)):
    """sap_lstsq on an operator: same outputs as sap_lstsq"""
    torch = _torch()
    lp, rp, m, n, dtype, _keep = _single_op_descs(op)
    suf = "f64" if dtype == torch.float64 else "f32"
    dev = f"cuda:{ctx.device}"
    x = torch.zeros(n, dtype=dtype, device=dev)
    y = torch.zeros(m, dtype=dtype, device=dev)
    resid = torch.full((iter_lim + 1,), float("nan"), dtype=dtype, device=dev)
    st = _state_arr(ctr, key)
    rank, iters = C.c_int64(0), C.c_int64(0)
    rc = getattr(ctx.lib, f"rlhip_drv_sap_lstsq_linop_{suf}")(ctx.h, lp, rp, b.data_ptr(), c.data_ptr(), delta, d_factor, nnz, tol, iter_lim,
                                                             x.data_ptr(), y.data_ptr(), resid.data_ptr(), st, C.byref(rank), C.byref(iters))
    _drv_check(ctx, rc, "sap_lstsq_op")
    it = int(iters.value)
    return dict(x=x, y=y, rank=int(rank.value), iters=it, resid=resid[: it + 1].cpu().numpy(), next_ctr=tuple(int(v) for v in st[:4]))
