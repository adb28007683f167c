"""Times of K * B for the squared-exponential kernel (or, with --kernel, a Matern kernel: DESIGN 4.23) on three routes, from device events
(DESIGN 4.22):
  (a) rlhip_rbf_apply_*            row blocks of K in scratch, three passes per block (the square operator's route)
  (b) rlhip_rbf_cross_apply_*      composed: the same scheme for two point sets (RLHIP_OPT_RBF_FUSED = 0)
  (c) rlhip_rbf_cross_apply_*      fused: one launch, K never in memory (RLHIP_OPT_RBF_FUSED = 1)
for the square shape dim x dim (Z = X) and one prediction shape mz x nx, in fp64 and fp32.

    python scripts/rbf_cross_time.py [--kernel sqexp|matern32|matern52] [--dim 131072] [--rows-x 16] [--n 1,8,64] [--mz 16384] [--reps 3]
                                     [--out profiles/rbf_cross_time.jsonl]

--kernel sqexp calls the rlhip_rbf_* entries named above, the Matern kinds their rlhip_pdk_* generalisations (the same routes).
One JSON line per (shape, precision, n, route): milliseconds, kernel evaluations per second (exp_per_s), and the scratch arena's high-water mark of a fresh
context that ran this route only.  Reads nothing outside the tree."""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1 << 17)
    ap.add_argument("--rows-x", type=int, default=16)
    ap.add_argument("--n", default="1,8,64")
    ap.add_argument("--mz", type=int, default=1 << 14, help="points of Z of the prediction shape (its X has --dim points)")
    ap.add_argument("--n-predict", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel", choices=["sqexp", "matern32", "matern52"], default="sqexp")
    a = ap.parse_args()
    import torch
    from randlapack_amd import device as dev

    h = 0.7 * a.rows_x ** 0.5
    kind = {"sqexp": dev.PDK_SQEXP, "matern32": dev.PDK_MATERN32, "matern52": dev.PDK_MATERN52}[a.kernel]
    lines = []
    for prec in a.prec.split(","):
        dt = torch.float64 if prec == "f64" else torch.float32
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((a.dim, a.rows_x), dtype=dt, device="cuda", generator=g)
        Z = torch.randn((a.mz, a.rows_x), dtype=dt, device="cuda", generator=g)
        shapes = [("square", X, a.dim, int(n)) for n in a.n.split(",")] + [("predict", Z, a.mz, a.n_predict)]
        for shape, Zp, mz, n in shapes:
            B = torch.randn((n, a.dim), dtype=dt, device="cuda", generator=g)
            Cm = torch.empty((n, mz), dtype=dt, device="cuda")
            routes = [("composed", 0), ("fused", 1)]
            if shape == "square":
                routes.insert(0, ("rbf_apply", None))
            results = {}
            for route, opt in routes:
                ctx = dev.Context(0)       # a fresh scratch arena: its high-water mark is this route's
                if opt is not None:
                    ctx.set_option("rbf_fused", opt)
                if a.kernel == "sqexp":
                    fn = ((lambda: dev.rbf_apply(ctx, X, a.rows_x, a.dim, h, B, n, C_=Cm)) if opt is None else
                          (lambda: dev.rbf_cross_apply(ctx, Zp, X, a.rows_x, mz, a.dim, h, B, n, C_=Cm)))
                else:
                    fn = ((lambda: dev.pdk_apply(ctx, X, a.rows_x, a.dim, kind, h, B, n, C_=Cm)) if opt is None else
                          (lambda: dev.pdk_cross_apply(ctx, Zp, X, a.rows_x, mz, a.dim, kind, h, B, n, C_=Cm)))
                before = [ctx.rbf_path_count(w) for w in (55, 56)]
                times = timed(torch, fn, a.reps)
                took = [ctx.rbf_path_count(w) - b for w, b in zip((55, 56), before)]
                results[route] = Cm.clone()
                ms = min(times)
                line = dict(kernel=a.kernel, shape=shape, prec=prec, rows_x=a.rows_x, mz=mz, nx=a.dim, n=n, route=route, ms=[round(t, 3) for t in times],
                            ms_min=round(ms, 3), exp_per_s=round(mz * a.dim / (ms * 1e-3), 0), fused_calls=took[0], composed_calls=took[1],
                            arena_highwater_bytes=int(ctx.lib.rlhip_workspace_highwater(ctx.h)))
                ctx.close()
                lines.append(line)
                print(json.dumps(line), flush=True)
            ref = results["composed"]
            scale = float(ref.abs().max())
            for route, out in results.items():
                print(f"# {shape} {prec} n={n}: max |{route} - composed| / max |composed| = {float((out - ref).abs().max()) / scale:.3g}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
