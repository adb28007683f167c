"""Times the normal product of least squares with s right-hand sides, Q = A^T (A D) + delta D, three ways, and one whole solve.

    python scripts/lsq_block_probe.py [--m 1048576] [--reps 30] [--out profiles/lsq_block_probe.json]

Shapes: fp64 at n = 64, 256, 1024 and fp32 at n = 256, 1024, each with s = 1, 2, 4, 8, 16, 32.  At each shape:
single    s calls of rlhip_normal_matvec on its default route: what the library could do before it had a block form;
composed  rlhip_normal_matmat on its composed route (two GEMMs: A read twice, whatever s);
one_pass  rlhip_normal_matmat on its one-pass route (A read once per chunk of columns); absent where n is beyond the kernel's limit.
The protocol is that of scripts/lsq_probe.py: 5 warm-up runs of every contender, then `reps` rounds in which the contenders ALTERNATE, each run
timed by device events on the context's stream; the figure is the median.  The JSON also holds the least bytes each form has to move (m n
values per chunk pass for one_pass, 2 m n + 2 m s for composed, s times the single call's for single) and the bandwidth that time amounts to.
The whole solve: sap_lstsq_block against s = 8 calls of sap_lstsq at m x 256 in fp64 on a Gaussian A (host clock around calls that end in a
synchronise; median of 5 after one warm-up).  Run the command twice to see the spread between runs."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "lsq_block_probe.json"))
    a = ap.parse_args()
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    ctx = dev.Context(0)
    m, reps = a.m, a.reps

    def alternate_ms(fs):
        """fs: dict name -> callable.  Medians of `reps` alternating rounds after 5 warm-up runs of each."""
        for f in fs.values():
            for _ in range(5):
                f()
        ctx.sync()
        t = {k: [] for k in fs}
        for _ in range(reps):
            for k, f in fs.items():
                ctx.timer_start()
                f()
                t[k].append(ctx.timer_stop_ms())
        return {k: statistics.median(v) for k, v in t.items()}

    out = {"m": m, "reps": reps, "device": torch.cuda.get_device_name(0), "lib_sha256": _lib.lib_sha256(), "shapes": []}
    for prec, n in (("f64", 64), ("f64", 256), ("f64", 1024), ("f32", 256), ("f32", 1024)):
        dt = torch.float64 if prec == "f64" else torch.float32
        e = 8 if prec == "f64" else 4
        g = torch.Generator(device="cuda").manual_seed(n)
        A = torch.randn((n, m), dtype=dt, device="cuda", generator=g)
        for s in (1, 2, 4, 8, 16, 32):
            D = torch.randn((s, n), dtype=dt, device="cuda", generator=g)
            Q = torch.zeros((s, n), dtype=dt, device="cuda")
            sc = dev.normal_matmat_fused(n, s, e)

            def single():
                for j in range(s):
                    dev.normal_matvec(ctx, m, n, A, D[j], 0.5, Q[j])

            def composed():
                with ctx.normal_matmat_route(0):
                    dev.normal_matmat(ctx, m, n, s, A, D, 0.5, Q)

            def one_pass():
                with ctx.normal_matmat_route(1):
                    dev.normal_matmat(ctx, m, n, s, A, D, 0.5, Q)

            fs = {"single": single, "composed": composed}
            if sc:
                fs["one_pass"] = one_pass
            c46 = ctx.lsq_path_count(46)
            single()
            single_fused = ctx.lsq_path_count(46) > c46
            single_bytes = (m * n + 2 * n) * e if single_fused else (2 * m * n + 2 * m + 2 * n) * e
            row = {"dtype": prec, "n": n, "s": s, "chunk": sc, "A_bytes": m * n * e, "single_route": "one pass" if single_fused else "two gemv",
                   "min_bytes": {"single": s * single_bytes, "composed": (2 * m * n + 2 * m * s) * e}}
            if sc:
                row["min_bytes"]["one_pass"] = -(-s // sc) * m * n * e
            row["ms"] = alternate_ms(fs)
            row["gb_per_s"] = {k: row["min_bytes"][k] / v / 1e6 for k, v in row["ms"].items()}
            out["shapes"].append(row)
            print(json.dumps(row), flush=True)
        del A
        torch.cuda.empty_cache()

    # the whole solve
    n, s, dt = 256, 8, torch.float64
    g = torch.Generator(device="cuda").manual_seed(7)
    A = torch.randn((n, m), dtype=dt, device="cuda", generator=g)
    B = torch.randn((s, m), dtype=dt, device="cuda", generator=g)
    z = torch.zeros(n, dtype=dt, device="cuda")
    tol, lim = 1e-10, 60

    def host_ms(f):
        f()
        t = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            r = f()
            ctx.sync()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t), r

    def singles():
        return [dev.sap_lstsq(ctx, A, m, n, B[j], z, 0.0, 4.0, 8, tol, lim, key=(7, 0))["iters"] for j in range(s)]

    def block(route):
        def f():
            with ctx.normal_matmat_route(route):
                return dev.sap_lstsq_block(ctx, A, m, n, s, B, None, 0.0, 4.0, 8, tol, lim, key=(7, 0))["iters"]
        return f

    solve = {"dtype": "f64", "m": m, "n": n, "s": s, "tol": tol, "ms": {}, "iters": {}}
    for name, f in (("eight_sap_lstsq", singles), ("sap_lstsq_block_composed", block(0)), ("sap_lstsq_block_one_pass", block(1)), ("sap_lstsq_block_default", block(-1))):
        solve["ms"][name], solve["iters"][name] = host_ms(f)
    out["solve"] = solve
    print(json.dumps(solve), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
