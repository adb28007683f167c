#!/usr/bin/env python3
"""bench.py -- headline benchmark: RSVD rank-256 of a 200000 x 20000 fp64 dense matrix (BASELINE.json configs[1]).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one full RandLAPACK::RSVD::call (sketch GEMM -> CholQR -> B = Q^T A -> SVD of B^T -> U) on the
synthetic matrix, which is generated ON the GPU before the timed region (inputs resident in HBM).  Rank 0
prints ONE JSON line; ms_per_step is the wall time of one timed step.  A plain run sets up, warms up, times
the steps and prints the line.
  --dump-outputs DIR -- after the timed steps, rank 0 writes what the last step returned as float64 .npy files:
                  S.npy (all k values), V.npy (n x k) and U_rows.npy (rows of U, m x k; a fixed sample of rows drawn by
                  numpy default_rng(0), sorted, once U is over 16 MB; on N ranks: rank 0's block), 64 MB at most.
                  Inputs are seeded, so two builds run with the same arguments can be compared file by file.
  --full       -- also measures the extras below (runs of their own, after the timed steps):
  roofline     -- the dominant kernel (fused-sketch MFMA GEMM  Y = A * Omega): algorithmic 2*m*n*k flops per
                  launch / average launch duration measured live with HIP events on the kernel's stream,
                  against the 78.6 TFLOP/s dense fp64 MFMA peak of MI355X.
  cpu_baseline -- the CPU oracle (restatement of the reference path over host LAPACK) timed on the host cores
                  on a bounded row-sample of the same workload (N=1, rank 0 only; --no-cpu-baseline drops it).

Multi-GPU: tall matrices shard by row blocks: every rank owns m/N rows, regenerates the same
Omega from the counter-based RNG, and the only exchanges are all-reduces of the k x k Gram matrix and the
n x k factor B^T over RCCL.  Total work is fixed as N grows -> "scaling": "strong".
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

M, N, K = 200_000, 20_000, 256
PEAK_F64_MFMA_TFLOPS = 78.6   # MI355X dense fp64 matrix peak (measured 77.7 by rlhip_mfma_peak)


def rsvd_flops(m, n, k, p=0):
    # 2mnk(2+p) + 2mk^2 (CholQR syrk+trsm) + 2mk^2 (U = Q*Uhat) + gesdd(n,k) ~ 6nk^2 + 8k^3
    return 2.0 * m * n * k * (2 + p) + 2.0 * m * k * k + 2.0 * m * k * k + 6.0 * n * k * k + 8.0 * k**3


def cpu_baseline(n, k, budget_rows=49152):
    """Oracle RSVD on a bounded sample (same n and k, fewer rows) on the host cores."""
    import numpy as np
    import oracle

    # as many threads as the host BLAS started with (OPENBLAS_NUM_THREADS / OMP_NUM_THREADS, else this process's CPUs): raising
    # OpenBLAS above the count it sized its buffers for crashes inside the library
    oracle.load()
    rng = np.random.default_rng(0)
    A = np.asfortranarray(rng.standard_normal((budget_rows, n)))
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        r = oracle.rsvd(A, k, k, 1e-12, 0, 1)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert r["k"] == k
    # the reference also pays the m x n copy and the wasted final update (rl_qb.hh:171,260): count useful flops only
    gf = rsvd_flops(budget_rows, n, k) / best / 1e9
    return dict(value=round(gf, 2), unit="GFLOP/s", cores=oracle.get_threads(), kind="port",
                sample=f"oracle RSVD (CholQRQ, p=0, one block) on {budget_rows}x{n} fp64 Gaussian, rank {k}, "
                       f"best of 2, {best:.2f} s")


DUMP_BYTES = dict(V=44_000_000, U_rows=16_000_000)   # with S (k values) under 64 MB in all


def _rows_sample(t, rows, cap_bytes):
    """Column-major device tensor t (k, rows) -> float64 numpy (r, k): every row while it fits in cap_bytes, else a fixed
    seeded sample of rows (sorted), taken on the device."""
    import numpy as np
    import torch

    k = t.shape[0]
    keep = max(1, cap_bytes // (8 * max(k, 1)))
    if rows > keep:
        idx = np.sort(np.random.default_rng(0).choice(rows, size=keep, replace=False))
        t = t.index_select(1, torch.from_numpy(idx).to(t.device))
    return t.detach().to(torch.float64).cpu().numpy().T.copy()


def dump_outputs(out_dir, r, mloc, n):
    """What a caller of the timed path receives from the last step (U, S, V of RSVD::call) as DIR/<name>.npy, float64."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    arrays = dict(S=r["S"].detach().double().cpu().numpy().copy(),
                  V=_rows_sample(r["V"], n, DUMP_BYTES["V"]),
                  U_rows=_rows_sample(r["U"], mloc, DUMP_BYTES["U_rows"]))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float64))


def roofline_leg(ctx, A, mloc, m, n, k, world, local_rank):
    """--full: the dominant kernel, timed live with HIP events on the kernel's own stream (its own launches, after the steps)."""
    from randlapack_amd import device as dev

    Om = dev.cm_empty(n, k, device=f"cuda:{local_rank}")
    ctx.fill_dense(Om, n, k, key=(0, 0))
    Y = dev.cm_empty(mloc, k, device=f"cuda:{local_rank}")
    reps = 5
    import ctypes as C

    nrm, fused = C.c_double(0), C.c_int(0)

    def sketch_gemm():   # exactly what RF/QB launch inside a step: Y = A * Omega with ||A||_F fused into the same pass
        rc = ctx.lib.rlhip_gemm_norma_f64(ctx.h, b"N", b"N", mloc, k, n, 1.0, A.data_ptr(), mloc, Om.data_ptr(), n, 0.0, Y.data_ptr(), mloc,
                                          C.byref(nrm), C.byref(fused))
        if rc != 0:
            raise RuntimeError(f"rlhip_gemm_norma_f64 failed: {rc}")

    sketch_gemm()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        sketch_gemm()
    kernel_ms = ctx.timer_stop_ms() / reps
    achieved = 2.0 * mloc * n * k / (kernel_ms * 1e-3) / 1e12
    # L2<->fabric bytes of this kernel from the PMC passes committed under profiles/ (collected at exactly this shape on one
    # GPU; separate --pmc passes, gfx950 x2 correction on FETCH_SIZE); other shapes / rank counts: not measured -> null
    # (a process cannot read its own PMC counters: the number is the committed measurement, and the line says which file and when)
    traffic, traffic_source = None, None
    try:
        if world == 1 and (m, n, k) == (M, N, K):
            import glob
            from randlapack_amd import _lib as _rl_lib
            here = os.path.dirname(os.path.abspath(__file__))
            # the latest committed pass (round 3 on: scripts/pmc_all.py writes one file per kernel; earlier rounds: pmc_traffic.sh)
            cands = glob.glob(os.path.join(here, "profiles", "round*_pmc_traffic.json")) + glob.glob(os.path.join(here, "profiles", "round*_pmc_gemm_sk_nn.json"))
            tfile = sorted(cands, key=lambda f: os.path.basename(f).split("_")[0])[-1]
            with open(tfile) as fh:
                tj = json.load(fh)
            tfile = os.path.relpath(tfile, here)
            # a counter file is only quoted when it describes THIS kernel: its own launch time (taken under the counters, which costs a
            # few per cent) must be within 5 % of the live one -- a stale file from another build reports null instead of a wrong number
            pmc_ms = float(tj.get("launch_ms_fetch_pass", tj.get("launch_ms", 0.0)) or 0.0)
            if pmc_ms > 0 and abs(pmc_ms - kernel_ms) <= 0.05 * kernel_ms:
                traffic = float(tj["traffic_bytes"])
                traffic_source = (f"{tfile} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel at this shape, scripts/pmc_all.py; launch {pmc_ms:.2f} ms "
                                  f"under counters vs {kernel_ms:.2f} ms live: within 5 %; not re-measured by this run)")
            elif pmc_ms > 0 and tj.get("librlhip_sha256") == _rl_lib.lib_sha256() and abs(pmc_ms - kernel_ms) <= 0.15 * kernel_ms:
                traffic = float(tj["traffic_bytes"])
                traffic_source = (f"{tfile} (counters taken on THIS build of librlhip.so (sha256 match); launch {pmc_ms:.2f} ms under counters vs "
                                  f"{kernel_ms:.2f} ms live -- the profiler's overhead, bytes are unaffected; not re-measured by this run)")
            else:
                traffic_source = f"{tfile} NOT quoted: its launch time {pmc_ms:.2f} ms is not within 5 % of the live {kernel_ms:.2f} ms"
    except Exception:
        traffic, traffic_source = None, None
    return dict(bound="mfma", achieved=round(achieved, 2), peak=PEAK_F64_MFMA_TFLOPS, unit="TFLOP/s",
                frac=round(achieved / PEAK_F64_MFMA_TFLOPS, 4), traffic=traffic, traffic_source=traffic_source,
                kernel="gemm_sk_kernel<NN> stream-K 128x256x16 (Y = A*Omega, ||A||_F fused) + fix-up",
                launch_ms=round(kernel_ms, 3), flops_per_launch=2.0 * mloc * n * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--m", type=int, default=M)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--k", type=int, default=K)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU oracle baseline")
    ap.add_argument("--full", action="store_true",
                    help="also measure the extras (roofline leg of the dominant kernel, CPU oracle baseline); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's U (row sample), S, V as DIR/<name>.npy (float64)")
    ap.add_argument("--opt", action="append", default=[], help="context option name=value (include/rlhip.h, enum rlhip_option), e.g. jacobi_clock_holders=0; A/B runs only")
    ap.add_argument("--busy-side", type=int, default=0, help="A/B runs only: keep this many workgroups of a SECOND stream busy with fp64 FMAs during every step (a device that is not ours alone)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if os.environ.get("RLHIP_BENCH_SHAPE"):      # tests: torch.distributed.run's own parser chokes on unknown short-looking options
        args.m, args.n, args.k = (int(x) for x in os.environ["RLHIP_BENCH_SHAPE"].split(","))

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N > 1")
    # RLHIP_BENCH_BACKEND=gloo lets the N > 1 code path be exercised on a box with fewer GPUs than ranks (tests): the ranks then share
    # the visible devices and the library's all-reduce hook exchanges through the host.  The driver's runs use nccl (= RCCL).
    backend = os.environ.get("RLHIP_BENCH_BACKEND", "nccl")
    ndev = max(torch.cuda.device_count(), 1)
    local_rank = local_rank % ndev
    torch.cuda.set_device(local_rank)
    pg_dev = "cpu" if backend == "gloo" else f"cuda:{local_rank}"
    dist = None
    if world > 1:
        import torch.distributed as dist

        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(backend)

    from randlapack_amd import device as dev
    from randlapack_amd import sharded

    ctx = dev.Context(local_rank)
    for kv in args.opt:
        ctx.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    m, n, k = args.m, args.n, args.k
    # row-block sharding: rank r owns rows [r*mloc, (r+1)*mloc) (last rank takes the remainder)
    mloc = m // world + (m % world if rank == world - 1 else 0)
    row0 = rank * (m // world)
    A = dev.cm_empty(mloc, n, device=f"cuda:{local_rank}")
    # synthetic iid N(0,1) data, generated in HBM; each rank uses its own key so the global matrix is iid
    ctx.fill_dense(A, mloc, n, key=(7 + rank, 0))
    ctx.sync()

    def step():
        if args.busy_side:                       # (A/B only) a second stream of this device is busy while the step runs
            ctx.lib.rlhip_dvfs_burn(ctx.h, args.busy_side, 1, int(1.3e3 * max(1.0, 62.0 * m / 200000.0)), 1)
        if world == 1:
            return dev.drv_rsvd(ctx, A, mloc, n, k, k, 1e-12, 0, 1, key=(0, 0))
        return sharded.rsvd_rowsharded(ctx, dist, A, mloc, n, k, key=(0, 0))

    transport = "none" if world == 1 else "rccl"
    if world > 1:
        # first sharded call (joins the RCCL communicator).  If the direct binding misbehaves on this machine, every rank falls
        # back to the library's all-reduce hook over torch.distributed's RCCL communicator -- still device-side over xGMI.
        ok = 1
        try:
            step()
        except Exception as e:  # noqa: BLE001
            ok = 0
            print(f"[bench rank {rank}] direct RCCL path failed ({e}); retrying through torch.distributed", file=sys.stderr, flush=True)
        flag = torch.tensor([ok], dtype=torch.int32, device=pg_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            ctx.lib.rlhip_comm_destroy(ctx.h)
            ctx.comm_transport = sharded.init_comm(ctx, dist, force_hook=True)
            step()
        transport = getattr(ctx, "comm_transport", "rccl")
    for _ in range(args.warmup):
        r = step()       # (held like the timed steps' results: the output pool then owns both alternating sets of U, S, V before the clock starts)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        r = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=pg_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / args.steps * 1e3
    flops = rsvd_flops(m, n, k)
    value = flops / (dt / args.steps) / 1e9
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, r, mloc, n)
    roofline = roofline_leg(ctx, A, mloc, m, n, k, world, local_rank) if args.full else None

    if rank == 0:
        out = {
            "metric": "GFLOP/s (sketch+factor) for RSVD rank-256 on m x n dense fp64",
            "value": round(value, 1),
            "unit": "GFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic iid N(0,1), generated on-device from Philox4x32-10",
            "config": {"workload": f"RSVD {m}x{n} fp64 rank {k}, one QB block, p=0, CholQRQ (BASELINE configs[1])",
                       "m": m, "n": n, "k": k, "parallelism": f"row-block x{world}", "collectives": transport,
                       # what the library's communicator actually saw (a scaling line must prove it ran on N ranks over RCCL)
                       "ranks_seen": int(ctx.lib.rlhip_comm_size(ctx.h)),
                       "comm_kind": {0: "none", 1: "rccl communicator of librlhip (ncclAllReduce on the context's stream)", 2: "hook"}[int(ctx.lib.rlhip_comm_kind(ctx.h))],
                       "rccl_version": int(ctx.lib.rlhip_comm_rccl_version()) if world > 1 else None,
                       "collectives_per_step": 0 if world == 1 else 2,   # Gram matrix of Y (+ ||A||_F^2 riding on it), B^T
                       "algorithmic_flops": flops, "qb_return": r["qb_rc"], "k_out": r["k"],
                       **({"ab_options": args.opt, "ab_busy_side_workgroups": args.busy_side} if (args.opt or args.busy_side) else {})},
            **({"roofline": roofline} if roofline is not None else {}),
            "frac_of_peak_whole_job": round(value / 1e3 / (PEAK_F64_MFMA_TFLOPS * world), 4),
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(n, k)
            except Exception as e:  # the baseline is a reported extra, never a reason to lose the bench line
                out["cpu_baseline"] = {"value": None, "unit": "GFLOP/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": f"failed: {e}"}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
