#!/usr/bin/env python3
"""tools/lobpcg_probe.py [--k 4] [--reps 3] [--grid 1000] [--band 100000] [--log profiles/lobpcg_probe.log] -- what the block eigensolver
(cvr_lobpcg_device) costs on the device and what a preconditioner buys it (needs a GPU).  Recorded, not gated.

On the five-point Laplacian of a grid x grid mesh and on synth.banded_sym(band, 2) made SPD (synth.spd_from_pattern), fp64, k columns, the lowest end:
  (a) time per iteration: cvr_lobpcg_device at tol = 0 and max_iters = 20 and 40, the difference of res.seconds over 20 -- beside k times the SpMV
      alone (cvr_spmv_bench) and k times the apply alone (events around a row of cvr_precond_apply_device calls); the rest is the vector kernels
      (residual, two Gram-Schmidt passes, Gram, combine), the read-back and the Rayleigh-Ritz step on the host, which this tool does not separate;
  (b) iterations and seconds to tol = 1e-8 (at most --max-iters) with no object, block-Jacobi 8, FSAI and amg_mis2;
  (c) beside them cvr_eigsh (which = SA, the default 20 columns, 100 restarts at most) on the same handle.
Each time is the median of --reps runs after one warm-up run.  Prints one JSON line per row and a table in Markdown; --log writes the same text."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--band", type=int, default=100000)
    ap.add_argument("--max-iters", type=int, default=600)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    k, lines, rows = args.k, [], []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    band = synth.spd_from_pattern(args.band, *synth.banded_sym(args.band, half_band=2)[2:4])
    for name, (n, _, rp, ci, va) in ((f"laplacian {args.grid} x {args.grid}", synth.laplacian_2d(args.grid)), (f"banded_sym({args.band}, 2), SPD", band)):
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        X0 = torch.from_numpy(np.random.default_rng(20261021).standard_normal((k, n))).cuda()
        r, z = torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        A.bench(20, 20)
        spmv_us = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
        objs = {"none": None, "block-Jacobi 8": capi.Precond.block_jacobi(rp, ci, va, 8), "FSAI": capi.Precond.fsai(rp, ci, va),
                "amg_mis2": capi.Precond.amg_mis2(A, rp, ci, va)}

        def run(pc, tol, max_iters):
            out = []
            for rep in range(args.reps + 1):
                X = X0.clone()
                ev, rn, res = A.lobpcg(X, pc, tol=tol, max_iters=max_iters)
                if rep:
                    out.append(res)
            out.sort(key=lambda q: q.seconds)
            return out[len(out) // 2]

        def apply_us(pc):
            ts = []
            for rep in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(20):
                    pc.apply(r.data_ptr(), z.data_ptr())
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ts.append(e0.elapsed_time(e1) * 1e3 / 20)
            return statistics.median(ts)

        for kind, pc in objs.items():
            t20, t40 = run(pc, 0.0, 20), run(pc, 0.0, 40)
            solve = run(pc, 1e-8, args.max_iters)
            o = dict(matrix=name, n=int(n), k=k, kind=kind, spmv_us=spmv_us, apply_us=apply_us(pc) if pc else 0.0,
                     iter_us=(t40.seconds - t20.seconds) / (t40.iterations - t20.iterations) * 1e6, iterations=solve.iterations, status=solve.status,
                     nconv=solve.nconv, solve_ms=solve.seconds * 1e3, without_p=solve.restarts_without_p, max_rel_residual=solve.max_rel_residual)
            say(json.dumps(o))
            rows.append(o)
        ts = []
        for rep in range(args.reps + 1):
            ev, _, res = A.eigsh(k, "SA", tol=1e-8, vectors=True)
            if rep:
                ts.append(res)
        ts.sort(key=lambda q: q.seconds)
        res = ts[len(ts) // 2]
        o = dict(matrix=name, n=int(n), k=k, kind="cvr_eigsh SA", iterations=res.spmv_count, status=res.status, nconv=res.nconv, solve_ms=res.seconds * 1e3,
                 restarts=res.restarts)
        say(json.dumps(o))
        rows.append(o)
        for pc in objs.values():
            if pc:
                pc.close()
        A.close()
    say()
    say("| matrix | k | object | per iteration | k SpMVs alone | k applies alone | the rest | iterations to 1e-8 | status (converged columns) | time |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        if o["kind"] == "cvr_eigsh SA":
            say(f"| {o['matrix']} | {o['k']} | cvr_eigsh SA | - | - | - | - | {o['iterations']} steps, {o['restarts']} restarts | {o['status']} ({o['nconv']}) | {o['solve_ms']:.1f} ms |")
        else:
            rest = o["iter_us"] - o["k"] * (o["spmv_us"] + o["apply_us"])
            say(f"| {o['matrix']} | {o['k']} | {o['kind']} | {o['iter_us']:.1f} us | {o['k'] * o['spmv_us']:.1f} us | {o['k'] * o['apply_us']:.1f} us | {rest:.1f} us | "
                f"{o['iterations']} | {o['status']} ({o['nconv']}) | {o['solve_ms']:.1f} ms |")
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
