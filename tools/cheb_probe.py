#!/usr/bin/env python3
"""tools/cheb_probe.py [--shapes banded,laplacian] [--banded-n 1000000] [--grid 1000] [--reps 3] [--out profiles/cheb_probe.log] -- what the Chebyshev
polynomial preconditioner buys and costs on the device (needs a GPU).

For each shape in fp64 -- the banded SPD matrix (synth.banded_sym made SPD by synth.spd_from_pattern, condition <= 3) and the 5-point Laplacian of a
grid x grid mesh (synth.laplacian_2d, condition ~ 0.4 grid^2) -- solves A x = b to rtol 1e-8 from x = 0 with
  (a) cvr_cg_device, no preconditioner;
  (b) cvr_pcg_device with block-Jacobi, block_size 8;
  (c) cvr_pcg_device with Chebyshev objects of degree 2, 4 and 8, bounds from cvr_chebyshev_bounds (20 power steps, ratio 30);
and reports iterations, the time to the tolerance (cvr_cg_result.seconds, the median of --reps runs after one warm-up run) and microseconds per step,
split into the SpMVs of a step (their number times the SpMV alone on the same handle, cvr_spmv_bench) and the rest: the vector kernels and the
read-backs.  Prints one JSON line per (shape, solver) and a table in Markdown; everything printed also goes to --out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402

RTOL = 1e-8
MAX_ITERS = 20000


def matrix(shape, args):
    if shape == "banded":
        n, _, rp, ci, _ = synth.banded_sym(args.banded_n)
        return synth.spd_from_pattern(n, rp, ci)
    if shape == "laplacian":
        return synth.laplacian_2d(args.grid)
    raise SystemExit(f"unknown shape {shape}")


def timed(solve, xt, reps):
    """(the result of the last run, the median seconds of `reps` runs after a warm-up run)"""
    ts = []
    for rep in range(reps + 1):
        xt.zero_()
        torch.cuda.synchronize()
        res = solve()
        if rep:
            ts.append(res.seconds)
    return res, statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="banded,laplacian")
    ap.add_argument("--banded-n", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cheb_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/cheb_probe.py --shapes {args.shapes} --banded-n {args.banded_n} --grid {args.grid} --reps {args.reps}: {cvr_amd.version()}, "
        f"{torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    rows = []
    for shape in args.shapes.split(","):
        n, _, rp, ci, va = matrix(shape, args)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        bt = torch.from_numpy(synth.x_rand(n)).cuda()
        xt = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.bench(20, 20)
        spmv_us = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
        lmin, lmax = A.chebyshev_bounds()
        base = dict(shape=shape, n=int(n), nnz=int(rp[-1]), spmv_us=spmv_us, lmin=lmin, lmax=lmax)
        solvers = [("cg", 1, None), ("block_jacobi_8", 1, lambda: capi.Precond.block_jacobi(rp, ci, va, 8))]
        solvers += [(f"chebyshev_{d}", d, (lambda d=d: capi.Precond.chebyshev(A, d, lmin, lmax))) for d in (2, 4, 8)]
        for name, per_step, make in solvers:
            P = make() if make else None
            if P is None:
                res, sec = timed(lambda: A.cg(bt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS), xt, args.reps)
            else:
                res, sec = timed(lambda: A.pcg(P, bt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS), xt, args.reps)
                P.close()
            steps = max(res.iterations, 1)
            out = dict(base, solver=name, status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, ms=sec * 1e3, us_per_step=sec * 1e6 / steps,
                       spmvs_per_step=per_step, spmv_us_per_step=per_step * spmv_us, other_us_per_step=sec * 1e6 / steps - per_step * spmv_us,
                       residual=res.residual_norm / res.b_norm)
            say(json.dumps(out))
            rows.append(out)
        A.close()
    say()
    say("| shape | n | solver | status | steps | time to 1e-8 | per step | of it SpMVs (count x SpMV alone) | vector kernels and read-backs |")
    say("|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        say(f"| {o['shape']} | {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us | "
            f"{o['spmv_us_per_step']:.1f} us ({o['spmvs_per_step']} x {o['spmv_us']:.1f}) | {o['other_us_per_step']:.1f} us |")
    log.close()


if __name__ == "__main__":
    main()
