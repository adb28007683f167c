"""Times the normal matvec q = A^T (A d) + delta d of pcg_saddle three ways, and one full pcg_saddle iteration.

    python scripts/lsq_probe.py [--m 1048576] [--reps 30] [--more] [--out profiles/lsq_probe.json]

Shapes: fp64 at n = 256 and n = 1024, fp32 at n = 1024 (A is 2.1, 8.6 and 4.3 GB: past the 256 MiB last-level cache).  At each shape:
fused     rlhip_normal_matvec on its one-pass route (A read once: m n values at the least);
composed  rlhip_gemv 'N' then rlhip_gemv 'T' (A read twice);
gemm      rlhip_gemm twice with a one-column right-hand side: what the library could do before it had a gemv (A read twice).
Each figure is the median of `reps` repetitions after 5 warm-up runs, timed by device events on the context's stream; the JSON also holds
the least bytes each form has to move and the bandwidth that time amounts to.  The pcg_saddle figure is the difference between a run of 12
and a run of 2 iterations (M = I / ||A||_F, tol too small to stop), divided by 10, host reads included."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--more", action="store_true", help="also n = 64 and 512 in fp64, 256 and 2048 in fp32 (where the default route changes)")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "lsq_probe.json"))
    a = ap.parse_args()
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    ctx = dev.Context(0)
    lib, h = ctx.lib, ctx.h
    m, reps = a.m, max(a.reps, 20)

    def median_ms(f):
        for _ in range(5):
            f()
        ctx.sync()
        t = []
        for _ in range(reps):
            ctx.timer_start()
            f()
            t.append(ctx.timer_stop_ms())
        return statistics.median(t)

    out = {"m": m, "reps": reps, "device": torch.cuda.get_device_name(0), "lib_sha256": _lib.lib_sha256(), "shapes": []}
    shapes = [("f64", 256), ("f64", 1024), ("f32", 1024)] + ([("f64", 64), ("f64", 512), ("f32", 256), ("f32", 2048)] if a.more else [])
    for prec, n in shapes:
        dt = torch.float64 if prec == "f64" else torch.float32
        e = 8 if prec == "f64" else 4
        g = torch.Generator(device="cuda").manual_seed(n)
        A = torch.randn((n, m), dtype=dt, device="cuda", generator=g)
        d = torch.randn(n, dtype=dt, device="cuda", generator=g)
        q, t = torch.zeros(n, dtype=dt, device="cuda"), torch.zeros(m, dtype=dt, device="cuda")
        gemm = getattr(lib, f"rlhip_gemm_{prec}")

        def fused():
            ctx.set_option("lsq_normal_fused", 1)
            dev.normal_matvec(ctx, m, n, A, d, 0.5, q)

        def composed():
            dev.gemv(ctx, "N", m, n, 1.0, A, d, 0.0, t)
            dev.gemv(ctx, "T", m, n, 1.0, A, t, 0.0, q)

        def by_gemm():
            _lib.check(gemm(h, b"N", b"N", m, 1, n, 1.0, A.data_ptr(), m, d.data_ptr(), n, 0.0, t.data_ptr(), m), "gemm")
            _lib.check(gemm(h, b"T", b"N", n, 1, m, 1.0, A.data_ptr(), m, t.data_ptr(), m, 0.0, q.data_ptr(), n), "gemm")

        row = {"dtype": prec, "n": n, "A_bytes": m * n * e, "ms": {}, "min_bytes": {"fused": (m * n + 2 * n) * e, "composed": (2 * m * n + 2 * m + 2 * n) * e,
                                                                                 "gemm": (2 * m * n + 2 * m + 2 * n) * e}, "gb_per_s": {}}
        for name, f in (("fused", fused), ("composed", composed), ("gemm", by_gemm)):
            row["ms"][name] = median_ms(f)
            row["gb_per_s"][name] = row["min_bytes"][name] / row["ms"][name] / 1e6
        ctx.set_option("lsq_normal_fused", -1)
        nrm = float(torch.linalg.norm(A))
        M = torch.eye(n, dtype=dt, device="cuda") / nrm
        b, c, x0 = torch.randn(m, dtype=dt, device="cuda", generator=g), torch.zeros(n, dtype=dt, device="cuda"), torch.zeros(n, dtype=dt, device="cuda")

        def run(iters):
            return lambda: dev.pcg_saddle(ctx, A, m, n, b, c, 0.5, iters, 1e-30, M, n, x0)

        t12, t2 = median_ms(run(12)), median_ms(run(2))
        row["ms"]["pcg_saddle_iteration"] = (t12 - t2) / 10.0
        row["route_counts_46_49"] = [ctx.lsq_path_count(i) for i in (46, 47, 48, 49)]
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del A, t, b
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
