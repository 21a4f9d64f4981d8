#!/usr/bin/env python3
"""tools/mcsgs_probe.py [--shapes laplacian,banded] [--grid 1000] [--banded-n 100000] [--block 8] [--reps 3] [--no-solves] [--out profiles/mcsgs_probe.log]
-- what the multicolour symmetric Gauss-Seidel preconditioner (Precond.mcsgs, kind 5) costs and buys beside plain CG, block-Jacobi, FSAI, ILU(0)
and amg_mis2, all in the same process (needs a GPU; fp64), modelled on tools/amg_probe.py.

For each shape -- the 5-point Laplacian of a grid x grid mesh and the banded SPD matrix (synth.banded_sym(n, half_band=2) made SPD) -- it reports
  (a) the colouring alone (capi.color_device from device arrays: the median wall time of --reps calls after a warm-up), its colours and rounds;
  (b) per preconditioner the set-up from host arrays (the median wall time of --reps builds after one warm-up build) and microseconds per apply,
      beside microseconds per SpMV of the same matrix: an apply of the new kind reads A once in each sweep, so two SpMVs are its yardstick;
  (c) PCG steps and time to rtol 1e-8 from x = 0 with every object, and plain CG.
Prints one JSON line per measurement and two tables in Markdown; everything printed also goes to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402
from amg_probe import RTOL, MAX_ITERS, apply_us, build_ms, matrix          # noqa: E402


def spmv_us(A, xt, yt, reps, inner=50):
    A.spmv_device(xt.data_ptr(), yt.data_ptr())
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            A.spmv_device(xt.data_ptr(), yt.data_ptr())
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="laplacian,banded")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--banded-n", type=int, default=100_000)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mcsgs_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/mcsgs_probe.py --shapes {args.shapes} --grid {args.grid} --banded-n {args.banded_n} --block {args.block} --reps {args.reps}: "
        f"{cvr_amd.version()}, {torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    rows = []
    for shape in args.shapes.split(","):
        n, _, rp, ci, va = matrix(shape, args)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        dev = [torch.from_numpy(a).cuda() for a in (rp, ci)]
        rt = torch.from_numpy(synth.x_rand(n)).cuda()
        zt = torch.zeros(n, dtype=torch.float64, device="cuda")
        xbuf = torch.zeros(max(A.info.x_elems, n + 1), dtype=torch.float64, device="cuda")
        ybuf = torch.zeros(max(A.info.yext_elems, n, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        base = dict(shape=shape, n=int(n), nnz=int(rp[-1]))
        ts = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            color, perm, ptr, nc, rounds = capi.color_device(dev[0].data_ptr(), dev[1].data_ptr(), on_device=True, n=n)
            ts.append((time.perf_counter() - t0) * 1e3)
        say(json.dumps(dict(base, what="color_device", ms=statistics.median(ts[1:]), ncolors=nc, rounds=rounds, rows_per_colour=np.diff(ptr).tolist())))
        one_spmv = spmv_us(A, xbuf, ybuf, args.reps)
        say(json.dumps(dict(base, what="spmv", us=one_spmv)))
        kinds = (("block_jacobi", lambda: capi.Precond.block_jacobi(rp, ci, va, args.block)), ("fsai", lambda: capi.Precond.fsai(rp, ci, va)),
                 ("ilu0", lambda: capi.Precond.ilu0(rp, ci, va)), ("amg_mis2", lambda: capi.Precond.amg_mis2(A, rp, ci, va)),
                 ("mcsgs", lambda: capi.Precond.mcsgs(rp, ci, va)))
        xt = torch.zeros(n, dtype=torch.float64, device="cuda")
        if not args.no_solves:
            torch.cuda.synchronize()
            res = A.cg(rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
            out = dict(base, kind="cg", build_ms=0.0, apply_us=0.0, spmv_us=one_spmv, launches=0, status=res.status, iterations=res.iterations, ms=res.seconds * 1e3)
            say(json.dumps(out))
            rows.append(out)
        for kind, make in kinds:
            P, ms = build_ms(make, args.reps)
            out = dict(base, kind=kind, build_ms=ms, apply_us=apply_us(P, rt, zt, args.reps), spmv_us=one_spmv)
            if kind == "mcsgs":
                i = P.mcsgs_info()
                out.update(launches=i.launches_per_apply, ncolors=i.ncolors, rounds=i.rounds, lanes=i.lanes_per_row, max_color_rows=i.max_color_rows, min_color_rows=i.min_color_rows)
            if kind == "ilu0":
                i = P.ilu0_info()
                out.update(launches=i.launches_lower + i.launches_upper, levels=i.levels_lower + i.levels_upper, lanes=i.lanes_per_row)
            if not args.no_solves:
                xt.zero_()
                torch.cuda.synchronize()
                res = A.pcg(P, rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                out.update(status=res.status, iterations=res.iterations, ms=res.seconds * 1e3)
            say(json.dumps(out))
            rows.append(out)
            P.close()
        A.close()
    say()
    say("| shape | n | preconditioner | set-up | per apply | in SpMVs | launches per apply | status | steps | time to 1e-8 | per step |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        solve = f"{o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['ms'] * 1e3 / max(o['iterations'], 1):.1f} us" if "iterations" in o else "- | - | - | -"
        say(f"| {o['shape']} | {o['n']} | {o['kind']} | {o['build_ms']:.1f} ms | {o['apply_us']:.1f} us | {o['apply_us'] / o['spmv_us']:.1f} | {o.get('launches', '-')} | {solve} |")
    log.close()


if __name__ == "__main__":
    main()
