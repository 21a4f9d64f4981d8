#!/usr/bin/env python3
"""tools/amg_probe.py [--shapes laplacian,banded] [--grid 1000] [--banded-n 100000] [--block 8] [--reps 3] [--no-solves]
[--out profiles/amg_probe.log] -- what the aggregation AMG preconditioner buys and costs on the device (needs a GPU; fp64, one process).

For each shape -- the 5-point Laplacian of a grid x grid mesh (synth.laplacian_2d) and the banded SPD matrix (synth.banded_sym(n, half_band=2) made
SPD by synth.spd_from_pattern) -- it reports
  (a) the set-up: wall time of Precond.amg from host arrays (the median of --reps builds after one warm-up build: the host hierarchy, the uploads and
      the creation of the coarse levels' handles), the levels' rows, the operator complexity, the products of one apply;
  (b) microseconds per apply (cvr_precond_apply_device, the median of --reps timings of a few applies in a row after one warm-up apply) beside the
      same number of plain SpMVs of A's handle (that many times cvr_spmv_bench's mean);
  (c) iterations and time to rtol 1e-8 from x = 0 (cvr_cg_result.seconds of one run) of PCG with AMG (the defaults, and coarse_scale = 1.5), FSAI,
      block-Jacobi (--block) and of plain CG, in the same run.
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
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "amg_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/amg_probe.py --shapes {args.shapes} --grid {args.grid} --banded-n {args.banded_n} --block {args.block} --reps {args.reps}: "
        f"{cvr_amd.version()}, {torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    applies, solves = [], []
    for shape in args.shapes.split(","):
        n, _, rp, ci, va = matrix(shape, args)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        rt = torch.from_numpy(synth.x_rand(n)).cuda()
        zt = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.bench(20, 20)
        spmv_us = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
        base = dict(shape=shape, n=int(n), nnz=int(rp[-1]), spmv_us=spmv_us)
        M, m_ms = build_ms(lambda: capi.Precond.amg(A, rp, ci, va), args.reps)
        M15 = capi.Precond.amg(A, rp, ci, va, coarse_scale=1.5)
        F = capi.Precond.fsai(rp, ci, va)
        J = capi.Precond.block_jacobi(rp, ci, va, args.block)
        mi = M.amg_info()
        s = mi.sweeps
        products = 2 * s * (mi.levels - 1) + (0 if mi.coarse_direct else 2 * s - 1)
        out = dict(base, kind="amg", build_ms=m_ms, apply_us=apply_us(M, rt, zt, args.reps), levels=[int(mi.n[l]) for l in range(mi.levels)],
                   operator_complexity=mi.operator_complexity, coarse_direct=mi.coarse_direct, products=products, same_products_of_a_us=products * spmv_us)
        say(json.dumps(out))
        applies.append(out)
        if not args.no_solves:
            xt = torch.zeros(n, dtype=torch.float64, device="cuda")
            for name, P in (("amg", M), ("amg_coarse_scale_1.5", M15), ("fsai", F), (f"block_jacobi_{args.block}", J), ("cg", None)):
                xt.zero_()
                torch.cuda.synchronize()
                if P is None:
                    res = A.cg(rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                else:
                    res = A.pcg(P, rt.data_ptr(), xt.data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                out = dict(base, solver=name, status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, ms=res.seconds * 1e3,
                           us_per_step=res.seconds * 1e6 / max(res.iterations, 1), residual=res.residual_norm / res.b_norm)
                say(json.dumps(out))
                solves.append(out)
        for P in (M, M15, F, J):
            P.close()
        A.close()
    say()
    say("| shape | n | set-up | levels | operator complexity | products per apply | per apply | as many SpMVs of A |")
    say("|---|---|---|---|---|---|---|---|")
    for o in applies:
        say(f"| {o['shape']} | {o['n']} | {o['build_ms']:.1f} ms | {', '.join(map(str, o['levels']))} | {o['operator_complexity']:.3f} | {o['products']} | "
            f"{o['apply_us']:.1f} us | {o['same_products_of_a_us']:.1f} us |")
    if solves:
        say()
        say("| shape | n | solver | status | steps | time to 1e-8 | per step |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['shape']} | {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us |")
    log.close()


if __name__ == "__main__":
    main()
