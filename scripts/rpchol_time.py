"""Per-call times of randomly pivoted Cholesky on an RBF kernel matrix (rlhip_drv_rpchol_rbf_*), from device events.

    python scripts/rpchol_time.py [--n 1048576] [--rows-x 16] [--k 1024] [--b 64] [--reps 3]

Prints one JSON line per precision.  The per-kernel split comes from a separate run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rows-x", type=int, default=16)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--bandwidth", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prec", default="f64,f32")
    a = ap.parse_args()
    import torch
    from randlapack_amd import device as dev

    ctx = dev.Context(0)
    for prec in a.prec.split(","):
        dt = torch.float64 if prec == "f64" else torch.float32
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((a.n, a.rows_x), dtype=dt, device="cuda", generator=g)
        dev.drv_rpchol_rbf(ctx, X, a.rows_x, a.n, a.bandwidth, a.k, a.b, key=(1, 0))      # warm-up: kernels loaded, scratch arena grown
        times = []
        for r in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = dev.drv_rpchol_rbf(ctx, X, a.rows_x, a.n, a.bandwidth, a.k, a.b, key=(1, r))
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        gemm_flop = a.n * a.k * a.k          # sum over blocks of 2 n b ell ~ n k^2
        print(json.dumps(dict(prec=prec, n=a.n, rows_x=a.rows_x, k=a.k, b=a.b, k_achieved=out["k"], status=out["status"],
                              c_status=out["c_status"], ms=[round(t, 3) for t in times], ms_min=round(min(times), 3),
                              downdate_gemm_tflops_if_all_time=round(gemm_flop / (min(times) * 1e-3) / 1e12, 2))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
