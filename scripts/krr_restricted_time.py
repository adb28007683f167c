"""Times of restricted kernel ridge regression next to the full one, from device events:
  fit      krill_restricted_rpchol (rp_cholesky + the SVD / filter tail) next to krill_full_rpchol (rpchol_pc_data + PCG) on the same
           points, right-hand sides and regularizations, and rp_cholesky alone;
  tail     the steps of the restricted tail on the factor of that rp_cholesky, one by one: the thin SVD, the two products (U^T H and W C),
           the filter, the triangular step (R^-1 = I R^-1, alpha = R^-1 Y);
  predict  krr_predict_restricted on the k centres next to krr_predict on the n x s coefficient block, at mz new points.

    python scripts/krr_restricted_time.py [--n 131072] [--rows-x 16] [--k 362,1024] [--s 8] [--mz 16384] [--prec f64,f32] [--reps 3]
                                          [--kernel sqexp|matern32|matern52] [--step-timeout 420] [--out profiles/krr_restricted_time.jsonl]

One warm-up, then the best of --reps.  One JSON line per (precision, k, what).  The device work of one precision is one child process under
its own time limit (--step-timeout seconds); the first child that does not exit with 0 ends the run with its code.  Reads nothing outside
the tree."""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, fn, reps, before=None):
    if before:
        before()
    fn()                                   # warm-up: kernels loaded, scratch arena grown
    times = []
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def worker(a, prec):
    import numpy as np
    import torch
    from randlapack_amd import device as dev

    kind = {"sqexp": dev.PDK_SQEXP, "matern32": dev.PDK_MATERN32, "matern52": dev.PDK_MATERN52}[a.kernel]
    dt = torch.float64 if prec == "f64" else torch.float32
    ct = C.c_double if prec == "f64" else C.c_float
    n, rows_x, s, mz = a.n, a.rows_x, a.s, a.mz
    h = 0.7 * rows_x ** 0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((n, rows_x), dtype=dt, device="cuda", generator=g)
    Z = torch.randn((mz, rows_x), dtype=dt, device="cuda", generator=g)
    H = torch.randn((s, n), dtype=dt, device="cuda", generator=g)
    mus = [float(m) for m in np.logspace(-3, 0, s)]
    tol = 1e-6 if prec == "f64" else 1e-4
    ctx = dev.Context(0)
    lines = []

    def emit(k, what, times, **extra):
        line = dict(kernel=a.kernel, prec=prec, n=n, rows_x=rows_x, k=k, s=s, what=what, ms=[round(t, 3) for t in times], ms_min=round(min(times), 3))
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for k in [int(v) for v in a.k.split(",")]:
        b = 64
        # ---- the fits
        out = {}
        emit(k, "rp_cholesky", timed(torch, lambda: out.update(rp=dev.drv_rpchol_pdk(ctx, X, rows_x, n, kind, h, k, b, key=(1, 0))), a.reps))
        emit(k, "fit_restricted", timed(torch, lambda: out.update(r=dev.krill_restricted_rpchol_pdk(ctx, X, rows_x, n, kind, h, mus, H, s, k=k, b=b, key=(1, 0))),
                                       a.reps), achieved_k=out["r"]["k"])
        X0 = torch.zeros((s, n), dtype=dt, device="cuda")
        emit(k, "fit_full", timed(torch, lambda: out.update(f=dev.krill_full_rpchol_pdk(ctx, X, rows_x, n, kind, h, mus, H, X0, s, tol, a.max_iters, k=k, b=b,
                                                                                       key=(1, 0))), a.reps, before=lambda: X0.zero_()),
             iters=out["f"]["iters"], max_iters=a.max_iters, tol=tol, normNR_last=float(out["f"]["normNR"][-1]) if len(out["f"]["normNR"]) else None)
        # ---- the tail, step by step, on the factor F (n x k, ld n) of rp_cholesky
        kk = out["rp"]["k"]
        F0 = out["rp"]["F"][:kk]
        F = torch.empty_like(F0)
        U = torch.empty((kk, n), dtype=dt, device="cuda")
        VT = torch.empty((kk, kk), dtype=dt, device="cuda")
        sg = torch.empty(kk, dtype=dt, device="cuda")
        gesdd = getattr(ctx.lib, f"rlhip_gesdd_{prec}")
        emit(kk, "tail_svd", timed(torch, lambda: gesdd(ctx.h, n, kk, F.data_ptr(), n, sg.data_ptr(), U.data_ptr(), n, VT.data_ptr(), kk, None), a.reps,
                                   before=lambda: F.copy_(F0)))
        Cm = torch.empty((s, kk), dtype=dt, device="cuda")
        Y = torch.empty((s, kk), dtype=dt, device="cuda")

        def products():
            ctx.gemm("T", "N", kk, s, n, 1.0, U, n, H, n, 0.0, Cm, kk)
            ctx.gemm("T", "N", kk, s, kk, 1.0, VT, kk, Cm, kk, 0.0, Y, kk)

        emit(kk, "tail_gemm", timed(torch, products, a.reps))
        mus_d = torch.tensor(mus, dtype=dt, device="cuda")
        emit(kk, "tail_filter", timed(torch, lambda: dev.ridge_filter(ctx, sg, mus_d, Cm, kk, s, rcond=0.0, ldc=kk), a.reps))
        S_dev = torch.from_numpy(out["rp"]["S"]).cuda()
        R = F0[:, S_dev].T.contiguous()                   # F0[:, S] is M = F(S, :) as a column-major tensor; its transpose is upper triangular
        Rinv = torch.empty_like(R)
        al = torch.empty((s, kk), dtype=dt, device="cuda")

        def triangular():
            ctx.laset("G", kk, kk, 0.0, 1.0, Rinv, kk)
            ctx.trsm(kk, kk, 1.0, R, kk, Rinv, kk)
            ctx.gemm("N", "N", kk, s, kk, 1.0, Rinv, kk, Y, kk, 0.0, al, kk)

        emit(kk, "tail_trsm", timed(torch, triangular, a.reps))
        # ---- prediction at mz points: k centres against all n coefficients
        r = out["r"]
        emit(k, "predict_restricted", timed(torch, lambda: dev.krr_predict_restricted_pdk(ctx, Z, mz, X, rows_x, n, kind, h, r["S"], r["alpha"], s), a.reps),
             mz=mz, kernel_evals=mz * r["k"])
        emit(k, "predict_full", timed(torch, lambda: dev.krr_predict_pdk(ctx, Z, mz, X, rows_x, n, kind, h, out["f"]["X"], s), a.reps), mz=mz, kernel_evals=mz * n)
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--rows-x", type=int, default=16)
    ap.add_argument("--k", default="362,1024")
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--mz", type=int, default=1 << 14)
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--kernel", choices=["sqexp", "matern32", "matern52"], default="sqexp")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a, a.worker)
        return 0
    if a.out:
        open(a.out, "w").close()
    for prec in a.prec.split(","):         # one child per precision, each under its own time limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, str(Path(__file__).resolve())] + sys.argv[1:] + ["--worker", prec], timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"# the {prec} step did not finish within {a.step_timeout} s", flush=True)
            return 124
        if rc != 0:
            print(f"# the {prec} step exited with {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
