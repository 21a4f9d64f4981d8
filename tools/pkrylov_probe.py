#!/usr/bin/env python3
"""tools/pkrylov_probe.py [--shapes banded1000000,blockdiag1000000] [--iters 32] [--reps 3] [--restart 30] [--block-sizes 1,4,8,16,32] [--json FILE] -- what the block-Jacobi object
costs per step in BiCGSTAB and GMRES(m) and what it saves in steps (needs a GPU).

Shapes: banded<rows> (synth.nonsym_from_pattern of synth.banded_sym: spectrum in the disc |z - 1| <= 0.5, nothing for a preconditioner to win) and
blockdiag<rows> (synth.block_diag_nonsym with blocks of 8 and condition 1e3: the case block-Jacobi is for).  For each, in fp64 and fp32, for both
solvers, and for
  plain     cvr_bicgstab_device / cvr_gmres_device without a preconditioner
  diag      the same with minv_dev = the inverse diagonal (the block_size = 1 object's exported W)
  obj bs    cvr_pbicgstab_device / cvr_pgmres_device at block_size = 1, 4, 8, 16, 32
it measures
  (a) seconds per step: rtol = 0 and max_iters = --iters, so every run does the same work; res.seconds / iterations
  (b) iterations, status and seconds to rtol = 1e-8 (fp32: 1e-4), max_iters = 1000
Each figure is the median of --reps runs after one warm-up run.  "obj 1 / diag" is the ratio of (a): the step with the apply launches of its own (two
more in BiCGSTAB, one more in GMRES) against the fused one on the same handle in the same process.  Prints one JSON line per (shape, precision,
solver) and a table in Markdown; the JSON goes to --json (default: profiles/pkrylov_probe.json).  --block-sizes 1 keeps a kernel trace of the
probe to the comparison of "obj 1" with "diag": the apply kernels' times in it are then those of block size 1."""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402

RTOL = {np.float64: 1e-8, np.float32: 1e-4}


def matrix(shape, dtype):
    m = re.fullmatch(r"(banded|blockdiag)(\d+)", shape)
    if not m:
        raise SystemExit(f"unknown shape {shape}: banded<rows> or blockdiag<rows>")
    rows = int(m.group(2))
    if m.group(1) == "banded":
        n, _, rp, ci, _ = synth.banded_sym(rows)
        return synth.nonsym_from_pattern(n, rp, ci, dtype=dtype)
    return synth.block_diag_nonsym(rows, 8, cond=1e3, dtype=dtype)


def median_of(fn, reps):
    fn()
    return statistics.median(fn() for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="banded1000000,blockdiag1000000")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--block-sizes", default="1,4,8,16,32", help="block sizes of the object; 1 is always among them")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pkrylov_probe.json"))
    args = ap.parse_args()
    block_sizes = sorted({1} | {int(v) for v in args.block_sizes.split(",")})
    rows = []
    for shape in args.shapes.split(","):
        for dtype in (np.float64, np.float32):
            n, _, rp, ci, va = matrix(shape, dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
            bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            objects = {bs: capi.Precond.block_jacobi(rp, ci, va, bs) for bs in block_sizes}
            minv = torch.from_numpy(objects[1].export().reshape(-1)).cuda()
            for solver in ("bicgstab", "gmres"):
                out = dict(shape=shape, prec=np.dtype(dtype).name, solver=solver, n=int(n), nnz=int(rp[-1]), iters=args.iters, reps=args.reps,
                           restart=args.restart if solver == "gmres" else None, rtol=RTOL[dtype], variants={})

                def solve(P, mv, **kw):
                    xt.zero_()
                    torch.cuda.synchronize()
                    if solver == "bicgstab":
                        if P is not None:
                            return A.pbicgstab(P, bt.data_ptr(), xt.data_ptr(), **kw)
                        return A.bicgstab(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mv is None else mv.data_ptr(), **kw)
                    if P is not None:
                        return A.pgmres(P, bt, x0=xt, restart=args.restart, **kw)[1]
                    return A.gmres(bt, x0=xt, restart=args.restart, minv=mv, **kw)[1]

                def measure(name, P, mv):
                    def step():
                        res = solve(P, mv, rtol=0.0, max_iters=args.iters)
                        return res.seconds / max(res.iterations, 1)
                    v = dict(step_us=median_of(step, args.reps) * 1e6)
                    res = solve(P, mv, rtol=RTOL[dtype], max_iters=1000)
                    v.update(iterations=res.iterations, status=res.status, rel_residual=res.residual_norm / res.b_norm if res.b_norm else 0.0,
                             solve_ms=median_of(lambda: solve(P, mv, rtol=RTOL[dtype], max_iters=1000).seconds, args.reps) * 1e3)
                    out["variants"][name] = v

                measure("plain", None, None)
                measure("diag", None, minv)
                for bs in block_sizes:
                    measure(f"obj {bs}", objects[bs], None)
                out["obj1_over_diag"] = out["variants"]["obj 1"]["step_us"] / out["variants"]["diag"]["step_us"]
                print(json.dumps(out), flush=True)
                rows.append(out)
            for P in objects.values():
                P.close()
            A.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    status = {capi.CG_CONVERGED: "converged", capi.CG_MAX_ITERS: "max_iters", capi.CG_BREAKDOWN: "breakdown"}
    print("\n| shape | type | solver | variant | us / step | steps to rtol | status | solve ms |")
    print("|---|---|---|---|---|---|---|---|")
    for o in rows:
        for name, v in o["variants"].items():
            print(f"| {o['shape']} | {o['prec']} | {o['solver']} | {name} | {v['step_us']:.1f} | {v['iterations']} | {status.get(v['status'], v['status'])} | {v['solve_ms']:.2f} |")
        print(f"| {o['shape']} | {o['prec']} | {o['solver']} | obj 1 / diag, us / step | {o['obj1_over_diag']:.3f} | | | |")


if __name__ == "__main__":
    main()
