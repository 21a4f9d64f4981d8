#!/usr/bin/env python3
"""tools/fgmres_probe.py [--grid 1000] [--cx -0.5] [--cy -0.25] [--restart 30] [--reps 15] [--iters 60] [--max-iters 3000] [--kinds a,b,..] -- what flexible
GMRES costs per step and what each kind of preconditioner buys on a nonsymmetric system (needs a GPU).

The matrix: synth.upwind_2d(grid, cx, cy), first-order upwind convection-diffusion on a grid x grid mesh (5-point pattern; diffusion 1; convection
(bx, by) h = (cx, cy); every row is weakly diagonally dominant for any of them), fp64, b = synth.x_rand.  For restart = --restart it reports, for
  gmres                     cvr_gmres_device without a preconditioner
  pgmres block-jacobi       cvr_pgmres_device with the block-Jacobi object (block size 4)
  pgmres ilu0-jacobi        cvr_pgmres_device with ILU(0), Jacobi-swept, 2 sweeps
  fgmres none               cvr_fgmres_device with neither an object nor a callback (Z is the basis)
  fgmres <kind>             cvr_fgmres_device with every kind that builds on the matrix: block-jacobi, ilu0, ilu0-jacobi, mcsgs, amg, amg-smoothed,
                            amg-mis2 (a kind whose constructor declines the matrix is listed with its message)
  (a) us / step: rtol = 0 and max_iters = --iters, so every run does the same work; res.seconds / iterations
  (b) steps, status and milliseconds to rtol = 1e-8, max_iters = --max-iters
each the median of --reps runs behind one warm-up run (a variant whose warm-up solve takes more than 2 s gets 3 runs, more than 20 s one: the count
is printed).  The last column is (a) against "pgmres block-jacobi", the same step of the solver that was there before.  Prints one JSON line per
variant and a table in Markdown."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402

KINDS = {
    "block-jacobi": lambda A, rp, ci, va: capi.Precond.block_jacobi(rp, ci, va, 4),
    "ilu0": lambda A, rp, ci, va: capi.Precond.ilu0(rp, ci, va),
    "ilu0-jacobi": lambda A, rp, ci, va: capi.Precond.ilu0_jacobi(rp, ci, va, 2),
    "mcsgs": lambda A, rp, ci, va: capi.Precond.mcsgs(rp, ci, va),
    "amg": lambda A, rp, ci, va: capi.Precond.amg(A, rp, ci, va),
    "amg-smoothed": lambda A, rp, ci, va: capi.Precond.amg_smoothed(A, rp, ci, va),
    "amg-mis2": lambda A, rp, ci, va: capi.Precond.amg_mis2(A, rp, ci, va),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--cx", type=float, default=-0.5)
    ap.add_argument("--cy", type=float, default=-0.25)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--kinds", default=",".join(KINDS))
    args = ap.parse_args()
    rtol = 1e-8
    n, _, rp, ci, va = synth.upwind_2d(args.grid, args.cx, args.cy)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    bt = torch.from_numpy(synth.x_rand(n)).cuda()
    xt = torch.zeros(n, dtype=torch.float64, device="cuda")
    print(f"upwind_2d({args.grid}, {args.cx}, {args.cy}): n = {n}, nnz = {int(rp[-1])}, restart {args.restart}, rtol {rtol}", flush=True)
    objects = {}
    for kind in args.kinds.split(","):
        t0 = time.perf_counter()
        try:
            objects[kind] = KINDS[kind](A, rp, ci, va)
            print(f"built {kind} in {time.perf_counter() - t0:.2f} s", flush=True)
        except capi.CvrError as e:
            print(f"{kind} does not build on this matrix: {e}", flush=True)
    variants = [("gmres", "gmres", None)]
    variants += [(f"pgmres {k}", "pgmres", objects[k]) for k in ("block-jacobi", "ilu0-jacobi") if k in objects]
    variants += [("fgmres none", "fgmres", None)] + [(f"fgmres {k}", "fgmres", P) for k, P in objects.items()]
    rows = []
    for name, solver, P in variants:
        def solve(**kw):
            xt.zero_()
            torch.cuda.synchronize()
            if solver == "gmres":
                return A.gmres(bt, x0=xt, restart=args.restart, **kw)[1]
            if solver == "pgmres":
                return A.pgmres(P, bt, x0=xt, restart=args.restart, **kw)[1]
            return A.fgmres(bt, args.restart, precond=P, x0=xt, **kw)[1]

        t0 = time.perf_counter()
        res = solve(rtol=rtol, max_iters=args.max_iters)          # the warm-up run
        warm = time.perf_counter() - t0
        reps = args.reps if warm <= 2 else 3 if warm <= 20 else 1
        solve_ms = statistics.median(solve(rtol=rtol, max_iters=args.max_iters).seconds for _ in range(reps)) * 1e3
        solve(rtol=0.0, max_iters=args.iters)
        step_us = statistics.median((lambda r: r.seconds / max(r.iterations, 1))(solve(rtol=0.0, max_iters=args.iters)) for _ in range(reps)) * 1e6
        out = dict(variant=name, reps=reps, steps=res.iterations, status=res.status, rel_residual=res.residual_norm / res.b_norm, spmv_count=res.spmv_count,
                   solve_ms=solve_ms, step_us=step_us)
        print(json.dumps(out), flush=True)
        rows.append(out)
    base = next((r["step_us"] for r in rows if r["variant"] == "pgmres block-jacobi"), None)
    plain = rows[0]
    status = {capi.CG_CONVERGED: "converged", capi.CG_MAX_ITERS: "max_iters", capi.CG_BREAKDOWN: "breakdown"}
    print("\n| variant | runs | steps to 1e-8 | status | solve ms | against gmres | us / step | against pgmres block-jacobi |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['variant']} | {r['reps']} | {r['steps']} | {status.get(r['status'], r['status'])} | {r['solve_ms']:.1f} | {r['solve_ms'] / plain['solve_ms']:.3f} | "
              f"{r['step_us']:.1f} | {'' if base is None else format(r['step_us'] / base, '.3f')} |")
    for P in objects.values():
        P.close()
    A.close()


if __name__ == "__main__":
    main()
