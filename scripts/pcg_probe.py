"""Times the three fused PCG device steps against the same steps composed from the entry points the library had before them.

    python scripts/pcg_probe.py [--n 200000] [--s 8] [--dim-pre 512] [--reps 30] [--out profiles/pcg_probe.json]

fp64.  fused: rlhip_pcg_update_xr (with the column norms), rlhip_pcg_update_p, rlhip_spectral_precond_apply (with the column norms).
composed: the same updates from rlhip_gemm, rlhip_axpby, rlhip_lacpy and rlhip_lange_fro only (the norm is then one Frobenius norm, read back).
Each figure is the median of `reps` repetitions after 5 warm-up runs, timed by device events on the context's stream; the JSON also holds the
bytes each fused step has to move at the least and the bandwidth that time amounts to."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--dim-pre", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "pcg_probe.json"))
    a = ap.parse_args()
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    ctx = dev.Context(0)
    lib, h = ctx.lib, ctx.h
    n, s, k = a.n, a.s, a.dim_pre
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(cols, rows):
        return torch.randn((cols, rows), dtype=torch.float64, device="cuda", generator=g)

    P, GP, X, R, NR, B, Cm, tmp = (rnd(s, n) for _ in range(8))
    alpha, beta = rnd(s, s) * 0.1, rnd(s, s) * 0.1
    V = rnd(k, n) / n ** 0.5
    D = -torch.rand((1, k), dtype=torch.float64, device="cuda", generator=g)
    Dm = torch.diag(D[0]).contiguous()
    W, W2 = rnd(s, k), rnd(s, k)
    res = C.c_double(0)

    def chk(rc):
        _lib.check(rc, "pcg_probe")

    def fused_xr():
        dev.pcg_update_xr(ctx, n, s, alpha, P, GP, X, R)

    def fused_p():
        dev.pcg_update_p(ctx, n, s, beta, NR, P)

    cn = torch.zeros(s, dtype=torch.float64, device="cuda")

    def fused_precond():
        chk(lib.rlhip_spectral_precond_apply_f64(h, n, k, V.data_ptr(), n, D.data_ptr(), 1, s, 1.0, B.data_ptr(), n, 0.0, Cm.data_ptr(), n, W.data_ptr(),
                                                 cn.data_ptr()))

    def gemm(ta, tb, m, nn, kk, al, A_, lda, B_, ldb, be, C_, ldc):
        chk(lib.rlhip_gemm_f64(h, ta, tb, m, nn, kk, al, A_.data_ptr(), lda, B_.data_ptr(), ldb, be, C_.data_ptr(), ldc))

    def composed_xr():
        gemm(b"N", b"N", n, s, s, 1.0, P, n, alpha, s, 1.0, X, n)
        gemm(b"N", b"N", n, s, s, -1.0, GP, n, alpha, s, 1.0, R, n)
        chk(lib.rlhip_lange_fro_f64(h, n, s, R.data_ptr(), n, C.byref(res)))

    def composed_p():
        chk(lib.rlhip_lacpy_f64(h, b"G", n, s, NR.data_ptr(), n, tmp.data_ptr(), n))
        gemm(b"N", b"N", n, s, s, 1.0, P, n, beta, s, 1.0, tmp, n)
        chk(lib.rlhip_lacpy_f64(h, b"G", n, s, tmp.data_ptr(), n, P.data_ptr(), n))

    def composed_precond():
        gemm(b"T", b"N", k, s, n, 1.0, V, n, B, n, 0.0, W, k)
        gemm(b"N", b"N", k, s, k, 1.0, Dm, k, W, k, 0.0, W2, k)
        chk(lib.rlhip_axpby_f64(h, n * s, 1.0, B.data_ptr(), 0.0, Cm.data_ptr()))
        gemm(b"N", b"N", n, s, k, 1.0, V, n, W2, k, 1.0, Cm, n)
        chk(lib.rlhip_lange_fro_f64(h, n, s, Cm.data_ptr(), n, C.byref(res)))

    def median_ms(f):
        for _ in range(5):
            f()
        ctx.sync()
        t = []
        for _ in range(max(a.reps, 20)):
            ctx.timer_start()
            f()
            t.append(ctx.timer_stop_ms())
        return statistics.median(t)

    e = 8
    must = {"update_xr": 6 * n * s * e, "update_p": 3 * n * s * e, "spectral_precond_apply": (2 * n * k + 6 * n * s) * e}
    out = {"n": n, "s": s, "dim_pre": k, "dtype": "f64", "reps": max(a.reps, 20), "device": torch.cuda.get_device_name(0), "lib_sha256": _lib.lib_sha256(),
           "fused_ms": {}, "composed_ms": {}, "fused_min_bytes": must, "fused_gb_per_s": {}}
    for name, ff, cf in (("update_xr", fused_xr, composed_xr), ("update_p", fused_p, composed_p),
                         ("spectral_precond_apply", fused_precond, composed_precond)):
        out["fused_ms"][name] = median_ms(ff)
        out["composed_ms"][name] = median_ms(cf)
        out["fused_gb_per_s"][name] = must[name] / out["fused_ms"][name] / 1e6
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
