#!/usr/bin/env python3
"""tools/ilu_jacobi_probe.py [--grid 1000] [--sweeps 1,2,3,4,5] [--reps 3] [--no-solves] [--out profiles/ilu_jacobi_probe.log] -- what ILU(0) with
Jacobi-swept triangular solves (cvr_precond_ilu0_jacobi) costs and buys on the device, beside the exact ILU(0) object, FSAI and plain CG measured in
the same run (needs a GPU; fp64, one process).

On the 5-point Laplacian of a grid x grid mesh (synth.laplacian_2d: 2 grid - 1 levels in each exact sweep) it reports
  (a) the set-up: wall time of Precond.ilu0_jacobi (s = 3), Precond.ilu0 and Precond.fsai from host arrays (the median of --reps builds after one
      warm-up build);
  (b) microseconds per apply (cvr_precond_apply_device, the median of --reps timings of a few applies in a row after one warm-up apply) for every s of
      --sweeps, for the exact object and for FSAI, beside two plain SpMVs of A's handle (twice cvr_spmv_bench's mean);
  (c) iterations and time to rtol 1e-8 from x = 0 (cvr_cg_result.seconds: the median of --reps runs, of one run where a run takes more than two
      seconds) of PCG with each of them and of plain CG.
Prints one JSON line per measurement and two tables in Markdown; everything printed also goes to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402

RTOL = 1e-8
MAX_ITERS = 20000


def build_ms(make, reps):
    """(an object, the median wall time of `reps` builds after one warm-up build, in ms)"""
    make().close()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = make()
        ts.append(time.perf_counter() - t0)
        if len(ts) < reps:
            P.close()
    return P, statistics.median(ts) * 1e3


def apply_us(P, rt, zt, reps):
    """microseconds per apply: the median of `reps` timings of `inner` applies in a row"""
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    inner = max(1, min(200, int(0.05 / max(one, 1e-6))))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            P.apply(rt.data_ptr(), zt.data_ptr())
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts) * 1e6


def solve(A, P, rt, xt, reps):
    """the result of the run with the median cvr_cg_result.seconds (one run where a run takes more than two seconds)"""
    runs = []
    for _ in range(reps):
        xt.zero_()
        torch.cuda.synchronize()
        if P is None:
            res = A.cg(rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
        else:
            res = A.pcg(P, rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
        runs.append(res)
        if res.seconds > 2.0:
            break
    runs.sort(key=lambda r: r.seconds)
    return runs[len(runs) // 2], len(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--sweeps", default="1,2,3,4,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ilu_jacobi_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/ilu_jacobi_probe.py --grid {args.grid} --sweeps {args.sweeps} --reps {args.reps}: {cvr_amd.version()}, {torch.cuda.get_device_name(0)}; "
        f"fp64, rtol {RTOL:g}, x0 = 0")
    sweeps = [int(s) for s in args.sweeps.split(",") if s]
    n, _, rp, ci, va = synth.laplacian_2d(args.grid)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    rt = torch.from_numpy(synth.x_rand(n)).cuda()
    zt = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.bench(20, 20)
    spmv_us = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
    base = dict(shape="laplacian", n=int(n), nnz=int(rp[-1]), two_spmv_us=2 * spmv_us)
    objects = []          # (name, object, set-up in ms or None, detail)
    for s in sweeps:
        if s == 3:
            P, ms = build_ms(lambda: capi.Precond.ilu0_jacobi(rp, ci, va, 3), args.reps)
        else:
            P, ms = capi.Precond.ilu0_jacobi(rp, ci, va, s), None
        j = P.ilu0_jacobi_info()
        objects.append((f"ilu0_jacobi_s{s}", P, ms, f"{j.launches_per_apply} launches, {j.lanes_per_row} lanes per row"))
    U, u_ms = build_ms(lambda: capi.Precond.ilu0(rp, ci, va), args.reps)
    ui = U.ilu0_info()
    objects.append(("ilu0_exact", U, u_ms, f"levels {ui.levels_lower}, {ui.levels_upper}; launches {ui.launches_lower}, {ui.launches_upper}"))
    F, f_ms = build_ms(lambda: capi.Precond.fsai(rp, ci, va), args.reps)
    objects.append(("fsai", F, f_ms, f"nnz(W) {F.fsai_info().nnz}"))
    applies, solves = [], []
    for name, P, ms, detail in objects:
        out = dict(base, kind=name, build_ms=ms, apply_us=apply_us(P, rt, zt, args.reps), detail=detail)
        say(json.dumps(out))
        applies.append(out)
    if not args.no_solves:
        xt = torch.zeros(n, dtype=torch.float64, device="cuda")
        for name, P in [(o[0], o[1]) for o in objects] + [("cg", None)]:
            res, runs = solve(A, P, rt, xt, args.reps)
            out = dict(base, solver=name, status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, ms=res.seconds * 1e3,
                       us_per_step=res.seconds * 1e6 / max(res.iterations, 1), residual=res.residual_norm / res.b_norm, runs=runs)
            say(json.dumps(out))
            solves.append(out)
    for _, P, _, _ in objects:
        P.close()
    A.close()
    say()
    say("| n | kind | set-up | per apply | two SpMVs of A | detail |")
    say("|---|---|---|---|---|---|")
    for o in applies:
        setup = "" if o["build_ms"] is None else f"{o['build_ms']:.1f} ms"
        say(f"| {o['n']} | {o['kind']} | {setup} | {o['apply_us']:.1f} us | {o['two_spmv_us']:.1f} us | {o['detail']} |")
    if solves:
        say()
        say("| n | solver | status | steps | time to 1e-8 | per step | runs |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us | {o['runs']} |")
    log.close()


if __name__ == "__main__":
    main()
