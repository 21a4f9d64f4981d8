#!/usr/bin/env python3
"""tools/minres_probe.py [--shapes banded,web] [--iters 32] [--reps 5] -- what a MINRES step costs on the device beside a conjugate-gradient step on the
same handle in the same process (needs a GPU).

For each shape (banded 2 M rows, web-Google-like), made SPD by synth.spd_from_pattern so that both solvers run on it, in fp64 and fp32:
  (a) cvr_minres_device with rtol = 0 and max_iters = --iters (every run does the same work): seconds / iterations at check_every = 1, 8, max_iters,
      without a preconditioner, with minv_dev, and with a shift;
  (b) cvr_cg_device the same way at check_every = 8, with and without minv_dev;
  (c) the SpMV alone on the same handle (cvr_spmv_bench): (a) - (c) and (b) - (c) are the solvers' own costs per step, the three vector kernels'.
Each figure is the median of --reps runs after one warm-up run (the first run of a process pays for loading the code objects and for the allocator).
Prints one JSON line per (shape, precision) and a table in Markdown."""
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


def pattern(shape):
    if shape == "web":
        n, _, rp, ci, _ = synth.web_google_like()
    elif shape == "banded":
        n, _, rp, ci, _ = synth.banded_sym(2_000_000)
    else:
        raise SystemExit(f"unknown shape {shape}")
    return n, rp, ci


def per_step(run, xt, iters, reps):
    ts = []
    for rep in range(reps + 1):
        xt.zero_()
        torch.cuda.synchronize()
        res = run()
        assert res.iterations == iters, (res.iterations, res.status)
        if rep:
            ts.append(res.seconds / res.iterations)
    return statistics.median(ts) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="banded,web")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    it = args.iters
    rows = []
    for shape in args.shapes.split(","):
        n, rp, ci = pattern(shape)
        n, _, rp2, ci2, va64 = synth.spd_from_pattern(n, rp, ci)
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            sz = np.dtype(dtype).itemsize
            A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va64.astype(dtype))
            bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            mt = torch.from_numpy((0.5 + 1.5 * np.random.default_rng(1).random(n)).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), iters=it, minres_vector_mb=15 * n * sz / 1e6,
                       minres_minv_vector_mb=17 * n * sz / 1e6, cg_vector_mb=11 * n * sz / 1e6)
            A.bench(20, 20)
            out["spmv_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
            for every in (1, 8, it):
                out[f"minres_us_every_{every}"] = per_step(lambda: A.minres(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=it, check_every=every)[0], xt, it, args.reps)
            out["minres_minv_us"] = per_step(lambda: A.minres(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=it, check_every=8, minv_ptr=mt.data_ptr())[0], xt, it, args.reps)
            out["minres_shift_us"] = per_step(lambda: A.minres(bt.data_ptr(), xt.data_ptr(), shift=2.0, rtol=0.0, max_iters=it, check_every=8)[0], xt, it, args.reps)
            out["cg_us"] = per_step(lambda: A.cg(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=it, check_every=8), xt, it, args.reps)
            out["cg_minv_us"] = per_step(lambda: A.cg(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=it, check_every=8, minv_ptr=mt.data_ptr()), xt, it, args.reps)
            out["minres_own_us"] = out["minres_us_every_8"] - out["spmv_us"]
            out["cg_own_us"] = out["cg_us"] - out["spmv_us"]
            out["ratio_to_cg"] = out["minres_us_every_8"] / out["cg_us"]
            out["ratio_to_cg_minv"] = out["minres_minv_us"] / out["cg_minv_us"]
            print(json.dumps(out), flush=True)
            rows.append(out)
            A.close()
    print(f"\n| shape | type | SpMV alone | MINRES step, check_every 1 | 8 | {it} | with minv | with a shift | CG step at 8 | with minv | MINRES own cost | CG own cost | MINRES / CG | with minv |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        print(f"| {o['shape']} | {o['prec']} | {o['spmv_us']:.1f} us | {o['minres_us_every_1']:.1f} | {o['minres_us_every_8']:.1f} | {o[f'minres_us_every_{it}']:.1f} | "
              f"{o['minres_minv_us']:.1f} | {o['minres_shift_us']:.1f} | {o['cg_us']:.1f} | {o['cg_minv_us']:.1f} | {o['minres_own_us']:.1f} us | {o['cg_own_us']:.1f} us | "
              f"{o['ratio_to_cg']:.2f} | {o['ratio_to_cg_minv']:.2f} |")


if __name__ == "__main__":
    main()
