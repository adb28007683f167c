"""Times of the cross apply C = K(Z, X) B for few to many points of Z against 2^17 points of X, on the three values of RLHIP_OPT_RBF_FUSED
(DESIGN 4.25):
  0  composed: row blocks of K in scratch
  1  fused, one launch: ceil(mz / 64) workgroups that each walk all of X
  2  fused, split over X into rlhip_rbf_split_chunks(mz, nx) chunks where that is > 1: two launches, partial sums in scratch
from device events, the method of scripts/rbf_cross_time.py: one warm-up, then the best of --reps.

    python scripts/rbf_split_time.py [--nx 131072] [--rows-x 16] [--n 1,8,64] [--mz 1,64,1000,4096,16384,131072] [--prec f64,f32]
                                     [--wide-rows-x 128] [--wide-mz 1000] [--reps 3] [--out profiles/rbf_split_time.jsonl]

--wide-rows-x adds one line per precision and n at the other end of the fused limits (mz = --wide-mz); 0 leaves it out.
One JSON line per (rows_x, precision, n, mz, value): the times, the chunks, the routes that ran, and the scratch arena's high-water mark of a
fresh context that ran this value only.  Reads nothing outside the tree."""
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
    ap.add_argument("--nx", type=int, default=1 << 17)
    ap.add_argument("--rows-x", type=int, default=16)
    ap.add_argument("--n", default="1,8,64")
    ap.add_argument("--mz", default="1,64,1000,4096,16384,131072")
    ap.add_argument("--wide-rows-x", type=int, default=128)
    ap.add_argument("--wide-mz", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prec", default="f64,f32")
    ap.add_argument("--values", default="0,1,2")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from randlapack_amd import device as dev

    ns = [int(v) for v in a.n.split(",")]
    mzs = [int(v) for v in a.mz.split(",")]
    sets = [(a.rows_x, mzs)] + ([(a.wide_rows_x, [a.wide_mz])] if a.wide_rows_x > 0 else [])
    lines = []
    for prec in a.prec.split(","):
        dt = torch.float64 if prec == "f64" else torch.float32
        for rows_x, mz_list in sets:
            h = 0.7 * rows_x ** 0.5
            g = torch.Generator(device="cuda").manual_seed(0)
            X = torch.randn((a.nx, rows_x), dtype=dt, device="cuda", generator=g)
            Zall = torch.randn((max(mz_list), rows_x), dtype=dt, device="cuda", generator=g)
            for n in ns:
                B = torch.randn((n, a.nx), dtype=dt, device="cuda", generator=g)
                for mz in mz_list:
                    Z = Zall[:mz]
                    Cm = torch.empty((n, mz), dtype=dt, device="cuda")
                    results = {}
                    for value in [int(v) for v in a.values.split(",")]:
                        ctx = dev.Context(0)       # a fresh scratch arena: its high-water mark is this value's
                        ctx.set_option("rbf_fused", value)
                        before = [ctx.rbf_path_count(w) for w in (55, 56)] + [ctx.rbf_split_count()]
                        times = timed(torch, lambda: dev.rbf_cross_apply(ctx, Z, X, rows_x, mz, a.nx, h, B, n, C_=Cm), a.reps)
                        took = [x - b for x, b in zip([ctx.rbf_path_count(w) for w in (55, 56)] + [ctx.rbf_split_count()], before)]
                        results[value] = Cm.clone()
                        ms = min(times)
                        line = dict(prec=prec, rows_x=rows_x, mz=mz, nx=a.nx, n=n, value=value, chunks=dev.rbf_split_chunks(mz, a.nx) if value == 2 else 1,
                                    ms=[round(t, 4) for t in times], ms_min=round(ms, 4), exp_per_s=round(mz * a.nx / (ms * 1e-3), 0),
                                    fused_calls=took[0], composed_calls=took[1], split_calls=took[2],
                                    arena_highwater_bytes=int(ctx.lib.rlhip_workspace_highwater(ctx.h)))
                        ctx.close()
                        lines.append(line)
                        print(json.dumps(line), flush=True)
                    ref = results[min(results)]
                    scale = float(ref.abs().max())
                    for value, out in results.items():
                        print(f"# {prec} rows_x={rows_x} n={n} mz={mz}: max |value {value} - value {min(results)}| / max = "
                              f"{float((out - ref).abs().max()) / scale:.3g}", flush=True)
                    if a.out:                      # rewritten as the run goes: what was measured survives an interrupted run
                        with open(a.out, "w") as f:
                            for ln in lines:
                                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
