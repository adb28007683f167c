"""Times of the predictive variance of restricted kernel ridge regression, rlhip_pdk_cross_var_*, from device events:
  fused      the one-launch kernel (on request: rlhip_pdk_var_set_fused, where rlhip_pdk_var_fused(rows_x, k, s) says so);
  composed   the same call with the default options: row blocks of t by the cross apply, one thread per row;
  baseline   what the library offered before this entry for the same result: rlhip_pdk_cross_apply_* with B = G into an mz x k buffer,
             then the squares and the weighted row sums in torch (in double, as the kernel takes them).

    python scripts/krr_var_time.py [--n 131072] [--rows-x 16] [--k 362,1024] [--mz 64,16384,131072] [--s 8] [--prec f64,f32] [--reps 3]
                                   [--kernel sqexp|matern32|matern52] [--step-timeout 420] [--out profiles/krr_var_time.jsonl]

The centres are the first k of n standard normal points, the basis is synthetic (G with entries N(0, 1) / sqrt(k), sigma descending): the
time does not depend on the values.  One warm-up of each of the three, then --reps rounds that time them in turn, so that drift hits all
three alike; ms_min is the best round.  The timed window holds the library call alone (the baseline's: the call and the torch
reductions); the switch between the routes is thrown outside it.  Every line also carries the largest difference of the route's result from the fused one.  One JSON
line per (precision, k, mz, what).  The device work of one precision is one child process under its own time limit (--step-timeout
seconds); the first child that does not exit with 0 ends the run with its code.  Reads nothing outside the tree."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def one(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def worker(a, prec):
    import torch
    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    kind = {"sqexp": dev.PDK_SQEXP, "matern32": dev.PDK_MATERN32, "matern52": dev.PDK_MATERN52}[a.kernel]
    dt = torch.float64 if prec == "f64" else torch.float32
    n, rows_x, s = a.n, a.rows_x, a.s
    h = 0.7 * rows_x ** 0.5
    gen = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((n, rows_x), dtype=dt, device="cuda", generator=gen)
    mzs = [int(v) for v in a.mz.split(",")]
    Zall = torch.randn((max(mzs), rows_x), dtype=dt, device="cuda", generator=gen)
    mus = torch.logspace(-6, 1, s, dtype=torch.float64, device="cuda").to(dt)
    ctx = dev.Context(0)
    lines = []
    for k in [int(v) for v in a.k.split(",")]:
        Xs = X[:k]
        G = torch.randn((k, k), dtype=dt, device="cuda", generator=gen) / k ** 0.5
        sigma = torch.sort(torch.rand(k, dtype=dt, device="cuda", generator=gen) * 3 + 1e-3, descending=True).values
        E = (mus.double()[:, None] / (sigma.double()[None, :] ** 2 + mus.double()[:, None])).contiguous()      # s x k
        for mz in mzs:
            Z = Zall[:mz]
            V = torch.empty((s, mz), dtype=dt, device="cuda")
            t = torch.empty((k, mz), dtype=dt, device="cuda")

            def var():
                return dev.pdk_cross_var(ctx, Z, mz, Xs, rows_x, k, kind, h, G, sigma, mus, s, V=V)

            def baseline():
                dev.pdk_cross_apply(ctx, Z, Xs, rows_x, mz, k, kind, h, G, k, C_=t)
                q = t.double() ** 2
                return (torch.clamp(1.0 - q.sum(dim=0), min=0.0)[None, :] + E @ q).to(dt)

            routes = [("fused", var, True), ("composed", var, False), ("baseline", baseline, False)]      # (name, call, the fused kernel asked for)
            on_fused_route = bool(_lib.load().rlhip_pdk_var_fused(rows_x, k, s))
            before = [ctx.var_path_count(w) for w in (58, 59)]
            results = {}
            for name, fn, want_fused in routes:                              # warm-up: kernels loaded, scratch arena grown
                with ctx.var_fused(want_fused):
                    results[name] = fn().clone()
            torch.cuda.synchronize()
            took = [ctx.var_path_count(w) - c for w, c in zip((58, 59), before)]
            assert took == ([1, 1] if on_fused_route else [0, 2]), took
            times = {name: [] for name, _, _ in routes}
            for _ in range(a.reps):
                for name, fn, want_fused in routes:
                    with ctx.var_fused(want_fused):
                        times[name].append(one(torch, fn))
            for name, _, _ in routes:
                diff = float((results[name].double() - results["fused"].double()).abs().max())
                line = dict(kernel=a.kernel, prec=prec, n=n, rows_x=rows_x, k=k, mz=mz, s=s, what=name, ms=[round(x, 3) for x in times[name]],
                            ms_min=round(min(times[name]), 3), max_diff_from_fused=diff, fused_route_serves_shape=on_fused_route,
                            flop_second_product=2 * mz * k * k, kernel_evaluations_fused=mz * k * ((k + 63) // 64))
                lines.append(line)
                print(json.dumps(line), flush=True)
            del V, t, results
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
    ap.add_argument("--mz", default="64,16384,131072")
    ap.add_argument("--s", type=int, default=8)
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
