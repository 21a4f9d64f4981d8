#!/usr/bin/env python3
"""tools/cg_probe.py [--shapes web,banded,lj] [--iters 64] [--reps 5] -- what a conjugate-gradient step costs on the device (needs a GPU).

For each shape (web-Google-like, banded 2 M rows, soc-LiveJournal1-like), made SPD by synth.spd_from_pattern, in fp64 and fp32:
  (a) cvr_cg_device with rtol = 0 and max_iters = --iters (every run does the same work): seconds / iterations at check_every = 1, 4, 8, 16, max_iters;
  (b) the SpMV alone on the same handle (cvr_spmv_bench): (a) - (b) is the solver's own cost per step;
  (c) the loop a user writes without the solver: cvr_spmv_device + torch vector operations + .item() for the two scalars, wall time per step.
Each figure is the median of --reps runs after one warm-up run (the first run of a process pays for loading the code objects and for the allocator).
Prints one JSON line per (shape, precision) and a table in Markdown."""
import argparse
import json
import os
import statistics
import sys
import time

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
    elif shape == "lj":
        n, _, rp, ci, _ = synth.livejournal_like()
    else:
        raise SystemExit(f"unknown shape {shape}")
    return n, rp, ci


def user_loop(A, bt, iters, tdt):
    """plain CG with torch: per step one cvr_spmv_device, five vector operations and two read-backs"""
    n = A.nrows
    x = torch.zeros(n, dtype=tdt, device="cuda")
    r = bt.clone()
    p = torch.zeros(A.info.x_elems, dtype=tdt, device="cuda")
    p[:n] = r
    q = torch.zeros(A.info.yext_elems, dtype=tdt, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rz = torch.dot(r, r).item()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        A.spmv_device(p.data_ptr(), q.data_ptr(), stream=st)
        alpha = rz / torch.dot(p[:n], q[:n]).item()
        x.add_(p[:n], alpha=alpha)
        r.add_(q[:n], alpha=-alpha)
        rz_new = torch.dot(r, r).item()
        p[:n].mul_(rz_new / rz).add_(r)
        rz = rz_new
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="web,banded,lj")
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for shape in args.shapes.split(","):
        n, rp, ci = pattern(shape)
        n, _, rp2, ci2, va64 = synth.spd_from_pattern(n, rp, ci)
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va64.astype(dtype))
            bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), col_panels=A.info.col_panels, col_phases=A.info.col_phases,
                       interleave=A.info.interleave, iters=args.iters, vector_mb=11 * n * np.dtype(dtype).itemsize / 1e6)
            A.bench(20, 20)
            out["spmv_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
            for every in (1, 4, 8, 16, args.iters):
                ts = []
                for rep in range(args.reps + 1):
                    xt.zero_()
                    torch.cuda.synchronize()
                    res = A.cg(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=args.iters, check_every=every)
                    assert res.iterations == args.iters, (res.iterations, res.status)
                    if rep:
                        ts.append(res.seconds / res.iterations)
                out[f"cg_us_every_{every}"] = statistics.median(ts) * 1e6
            user_loop(A, bt, 8, tdt)
            out["user_loop_us"] = statistics.median(user_loop(A, bt, args.iters, tdt) for _ in range(args.reps)) * 1e6
            print(json.dumps(out), flush=True)
            rows.append(out)
            A.close()
    it = args.iters
    print(f"\n| shape | type | SpMV alone | CG step, check_every 1 | 4 | 8 | 16 | {it} | own cost at 8 | torch loop | 11 n sizeof(T) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        print(f"| {o['shape']} | {o['prec']} | {o['spmv_us']:.1f} us | {o['cg_us_every_1']:.1f} | {o['cg_us_every_4']:.1f} | {o['cg_us_every_8']:.1f} | {o['cg_us_every_16']:.1f} | "
              f"{o[f'cg_us_every_{it}']:.1f} | {o['cg_us_every_8'] - o['spmv_us']:.1f} us | {o['user_loop_us']:.1f} us | {o['vector_mb']:.0f} MB |")


if __name__ == "__main__":
    main()
