#!/usr/bin/env python3
"""tools/sa_amg_probe.py [--shapes laplacian,banded] [--grid 1000] [--banded-n 100000] [--reps 3] [--no-solves] [--no-split]
[--out profiles/sa_amg_probe.log] -- what smoothed-aggregation AMG buys and costs on the device beside plain aggregation (needs a GPU; fp64, one
process), modelled on tools/amg_probe.py.

For each shape -- the 5-point Laplacian of a grid x grid mesh (synth.laplacian_2d) and the banded SPD matrix (synth.banded_sym(n, half_band=2) made
SPD by synth.spd_from_pattern) -- it reports
  (a) the set-up of Precond.amg and Precond.amg_smoothed from host arrays (the median wall time of --reps builds after one warm-up build), the levels'
      rows, the operator complexity, the products of one apply;
  (b) the smoothed set-up's three products per level on their own (A_l T_l, A_l P_l, R_l (A_l P_l)): each recreated by capi.SpGemm from the exported
      arrays, with its products, the rows per class and the seconds cvr_spgemm_get_info reports (the second of two creations);
  (c) microseconds per apply (the median of --reps timings of a few applies in a row after one warm-up apply) beside as many plain SpMVs of A;
  (d) iterations and time to rtol 1e-8 from x = 0 (cvr_cg_result.seconds of one run) of PCG with plain AMG, plain AMG with coarse_scale = 1.5, the
      smoothed kind, and of plain CG, in the same run.
Prints one JSON line per measurement and three tables in Markdown; everything printed also goes to --out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402
from amg_probe import RTOL, MAX_ITERS, apply_us, build_ms, matrix          # noqa: E402


def transpose(p):
    """(nc, n, row_ptr, col_idx, vals) of P^T, stable"""
    rows = np.repeat(np.arange(p.n, dtype=np.int64), np.diff(p.rp))
    order = np.argsort(p.ci, kind="stable")
    rp = np.zeros(p.nc + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(p.ci, minlength=p.nc))
    return p.nc, p.n, rp, rows[order].astype(np.int32), p.va[order]


def product_split(S):
    """the three products of every level of a smoothed object, recreated from its exports: a list of dicts"""
    info = S.amg_info()
    out = []
    for l in range(info.levels - 1):
        e, p = S.amg_export_level(l), S.amg_export_prolongator(l)
        a = (e.n, e.n, e.rp, e.ci, e.va)
        t = (e.n, p.nc, np.arange(e.n + 1, dtype=np.int64), e.agg, np.ones(e.n))
        pc = (p.n, p.nc, p.rp, p.ci, p.va)
        g = capi.SpGemm.create(a, pc)
        ap = (e.n, p.nc) + tuple(g.export())
        g.close()
        for name, left, right in (("A T", a, t), ("A P", a, pc), ("R (A P)", transpose(p), ap)):
            capi.SpGemm.create(left, right).close()          # (warm-up: code objects, allocator)
            g = capi.SpGemm.create(left, right)
            i = g.info()
            g.close()
            out.append(dict(level=l, product=name, rows=int(i.nrows), nnz=int(i.nnz), products=int(i.products), max_row_products=int(i.max_row_products),
                            rows_group=int(i.rows_group), rows_block=int(i.rows_block), rows_spill=int(i.rows_spill), symbolic_ms=i.symbolic_s * 1e3, numeric_ms=i.numeric_s * 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="laplacian,banded")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--banded-n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sa_amg_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/sa_amg_probe.py --shapes {args.shapes} --grid {args.grid} --banded-n {args.banded_n} --reps {args.reps}: "
        f"{cvr_amd.version()}, {torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, x0 = 0")
    applies, solves, splits = [], [], []
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
        S, s_ms = build_ms(lambda: capi.Precond.amg_smoothed(A, rp, ci, va), args.reps)
        for kind, P, ms in (("amg", M, m_ms), ("amg_smoothed", S, s_ms)):
            mi = P.amg_info()
            s = mi.sweeps
            products = P.amg_smoothed_info().products_per_apply or 2 * s * (mi.levels - 1) + (0 if mi.coarse_direct else 2 * s - 1)
            out = dict(base, kind=kind, build_ms=ms, apply_us=apply_us(P, rt, zt, args.reps), levels=[int(mi.n[l]) for l in range(mi.levels)],
                       level_nnz=[int(mi.nnz[l]) for l in range(mi.levels)], operator_complexity=mi.operator_complexity, coarse_direct=mi.coarse_direct, products=products,
                       same_products_of_a_us=products * spmv_us)
            say(json.dumps(out))
            applies.append(out)
        if not args.no_split:
            for o in product_split(S):
                o = dict(shape=shape, **o)
                say(json.dumps(o))
                splits.append(o)
        if not args.no_solves:
            xt = torch.zeros(n, dtype=torch.float64, device="cuda")
            for name, P in (("amg", M), ("amg_coarse_scale_1.5", M15), ("amg_smoothed", S), ("cg", None)):
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
        for P in (M, M15, S):
            P.close()
        A.close()
    say()
    say("| shape | n | kind | set-up | levels | operator complexity | products per apply | per apply | as many SpMVs of A |")
    say("|---|---|---|---|---|---|---|---|---|")
    for o in applies:
        say(f"| {o['shape']} | {o['n']} | {o['kind']} | {o['build_ms']:.1f} ms | {', '.join(map(str, o['levels']))} | {o['operator_complexity']:.3f} | {o['products']} | "
            f"{o['apply_us']:.1f} us | {o['same_products_of_a_us']:.1f} us |")
    if splits:
        say()
        say("| shape | level | product | rows | nnz(C) | products | longest row | group / block / spill rows | symbolic | numeric | ns per product |")
        say("|---|---|---|---|---|---|---|---|---|---|---|")
        for o in splits:
            total = o["symbolic_ms"] + o["numeric_ms"]
            say(f"| {o['shape']} | {o['level']} | {o['product']} | {o['rows']} | {o['nnz']} | {o['products']} | {o['max_row_products']} | {o['rows_group']} / {o['rows_block']} / "
                f"{o['rows_spill']} | {o['symbolic_ms']:.2f} ms | {o['numeric_ms']:.2f} ms | {total * 1e6 / max(o['products'], 1):.1f} |")
    if solves:
        say()
        say("| shape | n | solver | status | steps | time to 1e-8 | per step |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['shape']} | {o['n']} | {o['solver']} | {o['status']} | {o['iterations']} | {o['ms']:.2f} ms | {o['us_per_step']:.1f} us |")
    log.close()


if __name__ == "__main__":
    main()
