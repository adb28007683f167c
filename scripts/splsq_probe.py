"""Times the sparse normal matvec q = A^T (A d) + delta d of pcg_saddle on a SparseLinOp, its two halves on every route, the only way the
library had before (two SpMM calls with a one-column operand) and one full sparse pcg_saddle iteration.

    python scripts/splsq_probe.py [--m 1048576] [--reps 30] [--out profiles/splsq_probe.json]

Shapes: m = 2^20 rows, n = 256 and 1024 columns, 4, 16 and 64 nonzeros per row at uniformly random columns, fp64 and fp32.  At each:
normal        rlhip_csr_normal_matvec on its default routes;
forward_W     rlhip_csr_spmv on the CSR of A with 4, 16, 64 lanes per row forced (RLHIP_OPT_SPMV_LANES);
transposed_*  rlhip_csr_spmv on the CSR of A^T on the split route (0) and with 64 lanes per row;
spmm          rlhip_csr_spmm twice with one column-major column: what linops::SparseLinOp ran for a product with a vector before.
Each figure is the median of `reps` repetitions after 5 warm-up runs, timed by device events on the context's stream; the JSON also holds
the least bytes the normal matvec has to move, 2 nnz (8 + sizeof(T)) plus the vectors, and the bandwidth each time amounts to.  The
pcg_saddle figure is the difference between a run of 12 and a run of 2 iterations (M = I / ||A||_F, tol too small to stop), divided by 10,
host reads included."""
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
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "splsq_probe.json"))
    a = ap.parse_args()
    import torch

    from randlapack_amd import _lib
    from randlapack_amd import device as dev

    ctx = dev.Context(0)
    lib, h = ctx.lib, ctx.h
    m, reps = a.m, a.reps

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
    for prec in ("f64", "f32"):
        dt = torch.float64 if prec == "f64" else torch.float32
        e = 8 if prec == "f64" else 4
        for n in (256, 1024):
            for k in (4, 16, 64):
                g = torch.Generator(device="cuda").manual_seed(1000 * n + k)
                nnz = m * k
                rowptr = torch.arange(m + 1, dtype=torch.int64, device="cuda") * k
                colidx = torch.randint(0, n, (nnz,), dtype=torch.int64, device="cuda", generator=g)
                vals = torch.randn(nnz, dtype=dt, device="cuda", generator=g)
                # the CSR of the transpose: a stable sort of the entries by column (set-up, not timed)
                _, order = torch.sort(colidx, stable=True)
                rowptr_t = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                rowptr_t[1:] = torch.cumsum(torch.bincount(colidx, minlength=n), 0)
                colidx_t = torch.div(order, k, rounding_mode="floor")
                vals_t = vals[order]
                del order
                fwd, bwd = (rowptr, colidx, vals), (rowptr_t, colidx_t, vals_t)
                d = torch.randn(n, dtype=dt, device="cuda", generator=g)
                q, t = torch.zeros(n, dtype=dt, device="cuda"), torch.zeros(m, dtype=dt, device="cuda")
                spmm = getattr(lib, f"rlhip_csr_spmm_{prec}")

                def normal():
                    dev.csr_normal_matvec(ctx, m, n, fwd, bwd, d, 0.5, q)

                def forward():
                    dev.csr_spmv(ctx, m, n, rowptr, colidx, vals, 1.0, d, 0.0, t)

                def transposed():
                    dev.csr_spmv(ctx, n, m, rowptr_t, colidx_t, vals_t, 1.0, t, 0.0, q)

                def by_spmm():
                    _lib.check(spmm(h, b"C", m, 1, n, 1.0, rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr(), d.data_ptr(), n, 0.0, t.data_ptr(), m), "spmm")
                    _lib.check(spmm(h, b"C", n, 1, m, 1.0, rowptr_t.data_ptr(), colidx_t.data_ptr(), vals_t.data_ptr(), t.data_ptr(), m, 0.0, q.data_ptr(), n),
                               "spmm")

                row = {"dtype": prec, "n": n, "nnz_per_row": k, "nnz": nnz, "min_bytes": 2 * nnz * (8 + e) + (2 * m + 2 * n) * e, "ms": {}, "gb_per_s": {}}
                before = [ctx.spmv_path_count(i) for i in range(50, 55)]
                row["ms"]["normal"] = median_ms(normal)
                row["default_routes_50_54"] = [ctx.spmv_path_count(i) - b for i, b in zip(range(50, 55), before)]
                for w in (4, 16, 64):
                    ctx.set_option("spmv_lanes", w)
                    row["ms"][f"forward_{w}"] = median_ms(forward)
                for w, name in ((0, "transposed_split"), (64, "transposed_64")):
                    ctx.set_option("spmv_lanes", w)
                    row["ms"][name] = median_ms(transposed)
                ctx.set_option("spmv_lanes", -1)
                row["ms"]["spmm"] = median_ms(by_spmm)
                row["gb_per_s"] = {name: row["min_bytes"] * (1.0 if name in ("normal", "spmm") else 0.5) / ms / 1e6 for name, ms in row["ms"].items()}
                nrm = float(torch.linalg.norm(vals))
                M = torch.eye(n, dtype=dt, device="cuda") / nrm
                b, c, x0 = torch.randn(m, dtype=dt, device="cuda", generator=g), torch.zeros(n, dtype=dt, device="cuda"), torch.zeros(n, dtype=dt, device="cuda")
                op = dev.CsrOperator(m, n, rowptr, colidx, vals)

                def run(iters):
                    return lambda: dev.pcg_saddle_op(ctx, op, b, c, 0.5, iters, 1e-30, M, n, x0)

                # (every call builds the operator's transpose anew: the difference of the two runs cancels it)
                t12, t2 = median_ms(run(12)), median_ms(run(2))
                row["ms"]["pcg_saddle_iteration"] = (t12 - t2) / 10.0
                out["shapes"].append(row)
                print(json.dumps(row), flush=True)
                del rowptr, colidx, vals, rowptr_t, colidx_t, vals_t, fwd, bwd, op, t, b
                torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
