#!/usr/bin/env python3
"""tools/ilu_probe.py [--shapes laplacian,banded] [--grid 1000] [--banded-n 100000] [--wides 1,256,1024,4096,1000000] [--lanes 1,2,4] [--reps 3]
[--no-solves] [--out profiles/ilu_probe.log] -- what the ILU(0) preconditioner buys and costs on the device (needs a GPU).

For each shape in fp64 -- the 5-point Laplacian of a grid x grid mesh (synth.laplacian_2d: 2 grid - 1 levels each way, the widest of `grid` rows) and
the banded SPD matrix (synth.banded_sym(n, half_band=2) made SPD by synth.spd_from_pattern) -- it reports
  (a) per setting of the two tunables (CVR_DEBUG=ilu_wide=<w> and ilu_lanes=<g> while the object is built; "default" is the library's own choice):
      levels, launches and microseconds per apply (cvr_precond_apply_device, the median of --reps timings of a few applies in a row after one warm-up
      apply), beside the microseconds of one SpMV of the same handle (cvr_spmv_bench);
  (b) iterations and time to rtol 1e-8 from x = 0 (cvr_cg_result.seconds of one run) for plain CG, Chebyshev-PCG of degree 4 (bounds from
      cvr_chebyshev_bounds) and ILU(0)-PCG with the default settings.
A banded matrix has n levels of ONE row each way: its sweeps are n dependent steps of one workgroup and are slow by construction -- the shape is here
as the worst case of level scheduling, not as a use case (its ILU(0) is exact, so PCG stops after one step all the same).
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


def matrix(shape, args):
    if shape == "banded":
        n, _, rp, ci, _ = synth.banded_sym(args.banded_n, half_band=2)
        return synth.spd_from_pattern(n, rp, ci)
    if shape == "laplacian":
        return synth.laplacian_2d(args.grid)
    raise SystemExit(f"unknown shape {shape}")


def build(rp, ci, va, wide=None, lanes=None):
    knobs = [f"ilu_wide={wide}"] if wide is not None else []
    knobs += [f"ilu_lanes={lanes}"] if lanes is not None else []
    old = os.environ.get("CVR_DEBUG")
    try:
        if knobs:
            os.environ["CVR_DEBUG"] = ",".join(knobs)
        else:
            os.environ.pop("CVR_DEBUG", None)
        t0 = time.perf_counter()
        P = capi.Precond.ilu0(rp, ci, va)
        return P, time.perf_counter() - t0
    finally:
        if old is None:
            os.environ.pop("CVR_DEBUG", None)
        else:
            os.environ["CVR_DEBUG"] = old


def apply_us(P, rt, zt, reps):
    """microseconds per apply: the median of `reps` timings of `inner` applies in a row"""
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    inner = max(1, min(20, int(0.05 / max(one, 1e-6))))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            P.apply(rt.data_ptr(), zt.data_ptr())
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="laplacian,banded")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--banded-n", type=int, default=100_000)
    ap.add_argument("--wides", default="1,256,1024,4096,1000000")
    ap.add_argument("--lanes", default="1,2,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ilu_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/ilu_probe.py --shapes {args.shapes} --grid {args.grid} --banded-n {args.banded_n} --wides {args.wides} --lanes {args.lanes} --reps {args.reps}: "
        f"{cvr_amd.version()}, {torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    say("# (a banded matrix has n levels of one row: its sweeps are n dependent steps of one workgroup, slow by construction)")
    applies, solves = [], []
    for shape in args.shapes.split(","):
        n, _, rp, ci, va = matrix(shape, args)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        rt = torch.from_numpy(synth.x_rand(n)).cuda()
        zt = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.bench(20, 20)
        spmv_us = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
        base = dict(shape=shape, n=int(n), nnz=int(rp[-1]), spmv_us=spmv_us)
        settings = [("default", None, None)] + [(f"wide={w}", int(w), None) for w in args.wides.split(",") if w]
        if shape != "banded":          # (one row per level: every threshold gives the same plan but w = 1, and a row has two entries per triangle)
            settings += [(f"lanes={g}", None, int(g)) for g in args.lanes.split(",") if g]
        else:
            settings = [s for s in settings if s[1] in (None, 1000000)]          # (w = 1 would be 2 n launches per apply)
        for name, wide, lanes in settings:
            P, build_s = build(rp, ci, va, wide, lanes)
            i = P.ilu0_info()
            out = dict(base, setting=name, wide_threshold=i.wide_threshold, lanes_per_row=i.lanes_per_row, levels=[i.levels_lower, i.levels_upper],
                       launches=[i.launches_lower, i.launches_upper], max_level_width=i.max_level_width, build_ms=build_s * 1e3, apply_us=apply_us(P, rt, zt, args.reps))
            P.close()
            say(json.dumps(out))
            applies.append(out)
        if not args.no_solves:
            xt = torch.zeros(n, dtype=torch.float64, device="cuda")
            lmin, lmax = A.chebyshev_bounds()
            for name, make in (("cg", None), ("chebyshev_4", lambda: capi.Precond.chebyshev(A, 4, lmin, lmax)), ("ilu0", lambda: build(rp, ci, va)[0])):
                P = make() if make else None
                xt.zero_()
                torch.cuda.synchronize()
                if P is None:
                    res = A.cg(rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                else:
                    res = A.pcg(P, rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                    P.close()
                out = dict(base, solver=name, status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, ms=res.seconds * 1e3,
                           us_per_step=res.seconds * 1e6 / max(res.iterations, 1), residual=res.residual_norm / res.b_norm)
                say(json.dumps(out))
                solves.append(out)
        A.close()
    say()
    say("| shape | n | setting | wide_threshold | lanes per row | levels (L, U) | launches (L, U) | widest level | build | per apply | one SpMV |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for o in applies:
        say(f"| {o['shape']} | {o['n']} | {o['setting']} | {o['wide_threshold']} | {o['lanes_per_row']} | {o['levels'][0]}, {o['levels'][1]} | "
            f"{o['launches'][0]}, {o['launches'][1]} | {o['max_level_width']} | {o['build_ms']:.1f} ms | {o['apply_us']:.1f} us | {o['spmv_us']:.1f} us |")
    if solves:
        say()
        say("| shape | n | solver | status | steps | time to 1e-8 | per step |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['shape']} | {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us |")
    log.close()


if __name__ == "__main__":
    main()
