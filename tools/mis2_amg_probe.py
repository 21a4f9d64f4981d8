#!/usr/bin/env python3
"""tools/mis2_amg_probe.py [--shapes laplacian,banded] [--grid 1000] [--banded-n 100000] [--reps 3] [--no-solves] [--out profiles/mis2_amg_probe.log]
-- what the device set-up with the MIS(2) aggregation (Precond.amg_mis2) costs and buys beside Precond.amg_smoothed (needs a GPU; fp64, one
process), modelled on tools/sa_amg_probe.py.

For each shape -- the 5-point Laplacian of a grid x grid mesh and the banded SPD matrix (synth.banded_sym(n, half_band=2) made SPD) -- it reports
  (a) the set-up of Precond.amg_smoothed and Precond.amg_mis2, from host arrays and from device arrays each (the median wall time of --reps builds
      after one warm-up build), the levels' rows, the operator complexity, the MIS rounds per level;
  (b) the aggregation's kernels alone per level: cvr_amg_mis2_aggregate_device on the exported level, uploaded again (the median of --reps calls
      after a warm-up; the call includes its checks of the view, the diagonal kernel and three to four scalar read-backs);
  (c) microseconds per apply of both objects;
  (d) PCG steps and time to rtol 1e-8 from x = 0 with both objects.
Prints one JSON line per measurement and three tables in Markdown; everything printed also goes to --out."""
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


def aggregation_ms(P, reps):
    """the aggregation alone on every level of an object that was coarsened: a list of dicts"""
    info, minfo = P.amg_info(), P.amg_mis2_info()
    out = []
    for l in range(info.levels - 1):
        e = P.amg_export_level(l)
        t = [torch.from_numpy(a).cuda() for a in (e.rp, e.ci, e.va)]
        agg = torch.zeros(e.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        times = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            nc, rounds = capi.amg_mis2_aggregate_device(e.n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), agg.data_ptr(), strength=info.strength)
            times.append((time.perf_counter() - t0) * 1e3)
        assert nc == info.n[l + 1] and rounds == minfo.rounds[l] and np.array_equal(agg.cpu().numpy(), e.agg)
        out.append(dict(level=l, rows=int(e.n), nnz=int(info.nnz[l]), aggregates=int(nc), rounds=int(rounds), aggregate_ms=statistics.median(times[1:])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="laplacian,banded")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--banded-n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mis2_amg_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/mis2_amg_probe.py --shapes {args.shapes} --grid {args.grid} --banded-n {args.banded_n} --reps {args.reps}: "
        f"{cvr_amd.version()}, {torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    builds, aggs, solves = [], [], []
    for shape in args.shapes.split(","):
        n, _, rp, ci, va = matrix(shape, args)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        dev = [torch.from_numpy(a).cuda() for a in (rp, ci, va)]
        rt = torch.from_numpy(synth.x_rand(n)).cuda()
        zt = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        base = dict(shape=shape, n=int(n), nnz=int(rp[-1]))
        ptrs = [t.data_ptr() for t in dev]
        keep = {}
        for kind, source, make in (("amg_smoothed", "host", lambda: capi.Precond.amg_smoothed(A, rp, ci, va)),
                                   ("amg_smoothed", "device", lambda: capi.Precond.amg_smoothed_from_device(A, n, *ptrs)),
                                   ("amg_mis2", "host", lambda: capi.Precond.amg_mis2(A, rp, ci, va)),
                                   ("amg_mis2", "device", lambda: capi.Precond.amg_mis2_from_device(A, n, *ptrs))):
            P, ms = build_ms(make, args.reps)
            mi, minfo = P.amg_info(), P.amg_mis2_info()
            out = dict(base, kind=kind, arrays=source, build_ms=ms, levels=[int(mi.n[l]) for l in range(mi.levels)], operator_complexity=mi.operator_complexity,
                       rounds=[int(minfo.rounds[l]) for l in range(mi.levels - 1)] if minfo.mis2 else None, products=P.amg_smoothed_info().products_per_apply)
            if source == "device":
                out["apply_us"] = apply_us(P, rt, zt, args.reps)
                keep[kind] = P
            else:
                P.close()
            say(json.dumps(out))
            builds.append(out)
        for o in aggregation_ms(keep["amg_mis2"], args.reps):
            o = dict(shape=shape, **o)
            say(json.dumps(o))
            aggs.append(o)
        if not args.no_solves:
            xt = torch.zeros(n, dtype=torch.float64, device="cuda")
            for kind, P in keep.items():
                xt.zero_()
                torch.cuda.synchronize()
                res = A.pcg(P, rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                out = dict(base, solver=kind, status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, ms=res.seconds * 1e3,
                           us_per_step=res.seconds * 1e6 / max(res.iterations, 1), residual=res.residual_norm / res.b_norm)
                say(json.dumps(out))
                solves.append(out)
        for P in keep.values():
            P.close()
        A.close()
    say()
    say("| shape | n | kind | arrays | set-up | levels | operator complexity | MIS rounds | per apply |")
    say("|---|---|---|---|---|---|---|---|---|")
    for o in builds:
        rounds = ", ".join(map(str, o["rounds"])) if o["rounds"] is not None else "-"
        apply = f"{o['apply_us']:.1f} us" if "apply_us" in o else "-"
        say(f"| {o['shape']} | {o['n']} | {o['kind']} | {o['arrays']} | {o['build_ms']:.1f} ms | {', '.join(map(str, o['levels']))} | {o['operator_complexity']:.3f} | {rounds} | {apply} |")
    say()
    say("| shape | level | rows | nnz | aggregates | rounds | the aggregation alone |")
    say("|---|---|---|---|---|---|---|")
    for o in aggs:
        say(f"| {o['shape']} | {o['level']} | {o['rows']} | {o['nnz']} | {o['aggregates']} | {o['rounds']} | {o['aggregate_ms']:.2f} ms |")
    if solves:
        say()
        say("| shape | n | preconditioner | status | steps | time to 1e-8 | per step |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['shape']} | {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us |")
    log.close()


if __name__ == "__main__":
    main()
