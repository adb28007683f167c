"""Times of choosing the regularization of restricted kernel ridge regression, from device events:
  loo_kernel     rlhip_ridge_loo_* alone, on the U, sigma and C = U^T H of the factor of rp_cholesky on the same points;
  tail_svd       the thin SVD in front of it, for comparison;
  fit_cv         krill_restricted_rpchol_cv: factor, SVD, C, the kernel, the selection on the host, the filter and the rest of the tail;
  fit_single     one krill_restricted_rpchol with given regularizations: the same operations as before the path was added;
  fit_by_hand    g such fits one after the other, which is what choosing from a grid of g values costs without the path.

    python scripts/krr_loo_time.py [--n 131072] [--rows-x 16] [--k 362,1024] [--s 1,8] [--g 8,32] [--prec f64,f32] [--reps 3]
                                   [--kernel sqexp|matern32|matern52] [--step-timeout 420] [--out profiles/krr_loo_time.jsonl]

One warm-up, then the best of --reps (fit_by_hand: one run after the warm-up of fit_single).  One JSON line per (precision, k, s, g, what).
The device work of one precision is one child process under its own time limit (--step-timeout seconds); the first child that does not exit
with 0 ends the run with its code.  Reads nothing outside the tree."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, fn, reps):
    fn()                                   # warm-up: kernels loaded, scratch arena grown
    times = []
    for _ in range(reps):
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
    n, rows_x = a.n, a.rows_x
    h = 0.7 * rows_x ** 0.5
    gen = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((n, rows_x), dtype=dt, device="cuda", generator=gen)
    smax = max(int(v) for v in a.s.split(","))
    Hall = torch.randn((smax, n), dtype=dt, device="cuda", generator=gen)
    ctx = dev.Context(0)
    lines = []

    def emit(k, s, g, what, times, **extra):
        line = dict(kernel=a.kernel, prec=prec, n=n, rows_x=rows_x, k=k, s=s, g=g, what=what, ms=[round(t, 3) for t in times], ms_min=round(min(times), 3))
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for k in [int(v) for v in a.k.split(",")]:
        b = 64
        rp = dev.drv_rpchol_pdk(ctx, X, rows_x, n, kind, h, k, b, key=(1, 0))
        kk = rp["k"]
        F0 = rp["F"][:kk]
        F = torch.empty_like(F0)
        U = torch.empty((kk, n), dtype=dt, device="cuda")
        VT = torch.empty((kk, kk), dtype=dt, device="cuda")
        sg = torch.empty(kk, dtype=dt, device="cuda")
        gesdd = getattr(ctx.lib, f"rlhip_gesdd_{prec}")

        def svd():
            F.copy_(F0)
            gesdd(ctx.h, n, kk, F.data_ptr(), n, sg.data_ptr(), U.data_ptr(), n, VT.data_ptr(), kk, None)

        emit(kk, 0, 0, "tail_svd", timed(torch, svd, a.reps), note="includes the copy of the factor")
        for s in [int(v) for v in a.s.split(",")]:
            H = Hall[:s]
            Cm = torch.empty((s, kk), dtype=dt, device="cuda")
            ctx.gemm("T", "N", kk, s, n, 1.0, U, n, H, n, 0.0, Cm, kk)
            single = dict(ms=None)
            for g in [int(v) for v in a.g.split(",")]:
                grid = [float(m) for m in np.logspace(-6, 1, g)]
                mus_d = torch.tensor(grid, dtype=dt, device="cuda")
                emit(kk, s, g, "loo_kernel", timed(torch, lambda: dev.ridge_loo(ctx, U, sg, Cm, H, mus_d, n, kk, s, rcond=0.0, ldu=n, ldc=kk, ldh=n), a.reps),
                     flop=2 * n * kk * g * (1 + s), bytes_u=n * kk * U.element_size())
                out = {}
                emit(k, s, g, "fit_cv", timed(torch, lambda: out.update(r=dev.krill_restricted_rpchol_cv_pdk(ctx, X, rows_x, n, kind, h, grid, dev.CV_LOO, H, s, k=k,
                                                                                                            b=b, key=(1, 0))), a.reps),
                     achieved_k=out["r"]["k"], best=[int(v) for v in out["r"]["best"]])
                mus = [float(m) for m in out["r"]["best_mu"]]
                fit = lambda: dev.krill_restricted_rpchol_pdk(ctx, X, rows_x, n, kind, h, mus, H, s, k=k, b=b, key=(1, 0))
                if single["ms"] is None:
                    single["ms"] = timed(torch, fit, a.reps)
                emit(k, s, g, "fit_single", single["ms"])

                def by_hand():
                    for mu in grid:
                        dev.krill_restricted_rpchol_pdk(ctx, X, rows_x, n, kind, h, [mu], H, s, k=k, b=b, key=(1, 0))

                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                by_hand()
                e1.record()
                torch.cuda.synchronize()
                emit(k, s, g, "fit_by_hand", [e0.elapsed_time(e1)], fits=g)
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
    ap.add_argument("--s", default="1,8")
    ap.add_argument("--g", default="8,32")
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--reps", type=int, default=3)
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
