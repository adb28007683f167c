"""Times of the kernel-gradient apply rlhip_pdk_cross_grad_* from device events, beside the value it is the gradient of:
  fused      the one-launch kernel (on request: rlhip_pdk_grad_set_fused, where rlhip_pdk_grad_fused(rows_x, n) says so);
  composed   the same call with the default options: B' in scratch, the cross apply with the weight function, one thread per entry;
  value      rlhip_pdk_cross_apply_* on the same points and right-hand sides: the prediction alone.

    python scripts/pdk_grad_time.py [--n 131072] [--shapes 16:64,16:4096,16:16384,3:4096] [--rhs 1] [--prec f64,f32]
                                    [--kernel sqexp,matern32,matern52] [--reps 5] [--window-ms 250] [--step-timeout 420]
                                    [--out profiles/pdk_grad_time.jsonl]

--shapes lists rows_x:mz.  X is n standard normal points, Z the first mz of another such set, B standard normal: the time does not depend
on the values.  One warm-up of each of the three, which also sizes the timed window: a window is as many back-to-back calls as fill
--window-ms (at least 1, at most 200), between two device events; ms is the window over the calls.  --reps rounds time the three in turn, so
that drift hits all alike; ms_min is the best round, ms_spread the worst over the best.  The switch between the routes is thrown outside the
window.  Every line carries the largest difference of the route's gradient from the fused one, relative to the largest entry.  One JSON line
per (kernel, precision, shape, what).  The device work of one precision is one child process under its own time limit (--step-timeout
seconds); the first child that does not exit with 0 ends the run with its code.  Reads nothing outside the tree."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def window(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def worker(a, prec):
    import torch
    from randlapack_amd import device as dev

    kinds = {"sqexp": dev.PDK_SQEXP, "matern32": dev.PDK_MATERN32, "matern52": dev.PDK_MATERN52}
    dt = torch.float64 if prec == "f64" else torch.float32
    n, rhs = a.n, a.rhs
    ctx = dev.Context(0)
    lines = []
    for shape in a.shapes.split(","):
        rows_x, mz = (int(v) for v in shape.split(":"))
        h = 0.7 * rows_x ** 0.5
        gen = torch.Generator(device="cuda").manual_seed(rows_x)
        X = torch.randn((n, rows_x), dtype=dt, device="cuda", generator=gen)
        Z = torch.randn((mz, rows_x), dtype=dt, device="cuda", generator=gen)
        B = torch.randn((rhs, n), dtype=dt, device="cuda", generator=gen)
        G = torch.empty((rhs * mz, rows_x), dtype=dt, device="cuda")
        Y = torch.empty((rhs, mz), dtype=dt, device="cuda")
        on_fused_route = bool(ctx.lib.rlhip_pdk_grad_fused(rows_x, rhs))
        for kname in a.kernel.split(","):
            kind = kinds[kname]

            def grad():
                return dev.pdk_cross_grad(ctx, Z, X, rows_x, mz, n, kind, h, B, rhs, G=G)

            def value():
                return dev.pdk_cross_apply(ctx, Z, X, rows_x, mz, n, kind, h, B, rhs, C_=Y)

            routes = [("fused", grad, True), ("composed", grad, False), ("value", value, False)]      # (name, call, the fused kernel asked for)
            before = [ctx.grad_path_count(w) for w in (74, 75)]
            results, calls = {}, {}
            for name, fn, want_fused in routes:                              # warm-up: kernels loaded, scratch arena grown; sizes the window
                with ctx.grad_fused(want_fused):
                    results[name] = fn().clone()
                    calls[name] = max(1, min(200, int(a.window_ms / max(window(torch, fn, 1), 1e-3))))
            took = [ctx.grad_path_count(w) - c for w, c in zip((74, 75), before)]
            assert took == ([2, 2] if on_fused_route else [0, 4]), took
            times = {name: [] for name, _, _ in routes}
            for _ in range(a.reps):
                for name, fn, want_fused in routes:
                    with ctx.grad_fused(want_fused):
                        times[name].append(window(torch, fn, calls[name]))
            top = float(results["fused"].double().abs().max())
            for name, _, _ in routes:
                line = dict(kernel=kname, prec=prec, n=n, rows_x=rows_x, mz=mz, rhs=rhs, what=name, calls_per_window=calls[name],
                            ms=[round(x, 4) for x in times[name]], ms_min=round(min(times[name]), 4),
                            ms_spread=round(max(times[name]) / min(times[name]), 3), fused_route_serves_shape=on_fused_route,
                            kernel_evaluations=mz * n)
                if name != "value":
                    line["rel_diff_from_fused"] = float((results[name].double() - results["fused"].double()).abs().max()) / top
                    line["ms_over_value"] = round(min(times[name]) / min(times["value"]), 3)
                lines.append(line)
                print(json.dumps(line), flush=True)
            del results
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--shapes", default="16:64,16:4096,16:16384,3:4096")
    ap.add_argument("--rhs", type=int, default=1)
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--kernel", default="sqexp,matern32,matern52")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
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
