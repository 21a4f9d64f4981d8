#!/usr/bin/env python3
"""tools/lsqr_probe.py [--shapes tall,wide,scattered] [--iters 16] [--reps 5] [--damp 0.0] -- what an LSQR step costs on the device (needs a GPU).

For each shape from synth.rect_banded -- tall banded (2 M x 250 k, five entries per row), its wide counterpart (250 k x 2 M) and a tall one with
scattered columns (1 M x 200 k: the band plus four random columns per row) --, in fp64 and fp32, with A^T's handle made by transpose = 1:
  (a) cvr_lsqr_device with rtol = 0 and max_iters = --iters (every run does the same work): seconds / iterations at check_every = 1, 8, max_iters;
  (b) the two products alone (cvr_spmv_bench on each handle): (a) - (b) is the solver's own cost per step, its share of the step the three
      vector kernels';
  (c) the solve to rtol = 1e-8 from x0 = 0 for an inconsistent b: iterations, the test that stopped it, seconds.
Each figure is the median of --reps runs after one warm-up run.  Prints one JSON line per (shape, precision) and a table in Markdown."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvr_amd                      # noqa: E402
from cvr_amd import synth          # noqa: E402

SHAPES = dict(tall=(2_000_000, 250_000, 2, 0), wide=(250_000, 2_000_000, 2, 0), scattered=(1_000_000, 200_000, 2, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tall,wide,scattered")
    ap.add_argument("--iters", type=int, default=16)          # (these shapes are well conditioned: 32 steps would reach the rounding floor)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--damp", type=float, default=0.0)
    args = ap.parse_args()
    rows = []
    for shape in args.shapes.split(","):
        if shape not in SHAPES:
            raise SystemExit(f"unknown shape {shape}")
        m, n, hb, extra = SHAPES[shape]
        m, n, rp, ci, va64 = synth.rect_banded(m, n, half_band=hb, extra=extra)
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            va = va64.astype(dtype)
            A = cvr_amd.CvrMatrix(m, n, rp, ci, va)
            AT = cvr_amd.CvrMatrix(m, n, rp, ci, va, transpose=1)
            bt = torch.from_numpy(synth.x_rand(m).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(shape=shape, prec=np.dtype(dtype).name, m=int(m), n=int(n), nnz=int(rp[-1]), iters=args.iters, damp=args.damp,
                       vector_mb=(3 * m + 9 * n) * np.dtype(dtype).itemsize / 1e6)
            for H, key in ((A, "spmv_a_us"), (AT, "spmv_at_us")):
                H.bench(20, 20)
                out[key] = statistics.median(H.bench(5, 50) for _ in range(args.reps)) * 1e6
            for every in (1, 8, args.iters):
                ts = []
                for rep in range(args.reps + 1):
                    xt.zero_()
                    torch.cuda.synchronize()
                    res, _ = A.lsqr(AT, bt.data_ptr(), xt.data_ptr(), damp=args.damp, rtol=0.0, max_iters=args.iters, check_every=every)
                    if res.iterations != args.iters:
                        out["stopped"] = dict(iterations=res.iterations, status=res.status)
                        break
                    if rep:
                        ts.append(res.seconds / res.iterations)
                out[f"step_us_every_{every}"] = statistics.median(ts) * 1e6 if ts else float("nan")
            out["own_us_at_8"] = out["step_us_every_8"] - out["spmv_a_us"] - out["spmv_at_us"]
            out["vector_share_at_8"] = out["own_us_at_8"] / out["step_us_every_8"]
            ts = []
            for rep in range(args.reps + 1):
                xt.zero_()
                torch.cuda.synchronize()
                res, info = A.lsqr(AT, bt.data_ptr(), xt.data_ptr(), damp=args.damp, rtol=1e-8, max_iters=2000)
                if rep:
                    ts.append(res.seconds)
            out.update(solve_iterations=res.iterations, solve_status=res.status, solve_stop_test=info.stop_test, solve_ms=statistics.median(ts) * 1e3)
            print(json.dumps(out), flush=True)
            rows.append(out)
            AT.close()
            A.close()
    it = args.iters
    print(f"\n| shape | type | A v alone | A^T u alone | LSQR step, check_every 1 | 8 | {it} | own cost at 8 | its share of the step | (3 m + 9 n) sizeof(T) | to rtol 1e-8 |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        print(f"| {o['shape']} {o['m']} x {o['n']} | {o['prec']} | {o['spmv_a_us']:.1f} us | {o['spmv_at_us']:.1f} us | {o['step_us_every_1']:.1f} | {o['step_us_every_8']:.1f} | "
              f"{o[f'step_us_every_{it}']:.1f} | {o['own_us_at_8']:.1f} us | {100 * o['vector_share_at_8']:.0f} % | {o['vector_mb']:.0f} MB | "
              f"{o['solve_iterations']} steps (test {o['solve_stop_test']}), {o['solve_ms']:.2f} ms |")


if __name__ == "__main__":
    main()
