#!/usr/bin/env python3
"""tools/bicgstab_probe.py [--shapes web,banded,lj] [--iters 32] [--reps 5] [--c 0.95] -- what a BiCGSTAB step costs on the device (needs a GPU).

For each shape (web-Google-like, banded 2 M rows, soc-LiveJournal1-like), made nonsymmetric and diagonally dominant by synth.nonsym_from_pattern
(c close to 1, so that --iters steps do not reach the rounding floor), in fp64 and fp32:
  (a) cvr_bicgstab_device with rtol = 0 and max_iters = --iters (every run does the same work): seconds / iterations at check_every = 1, 4, 8, 16,
      max_iters;
  (b) the SpMV alone on the same handle (cvr_spmv_bench): (a) - 2 (b) is the solver's own cost per step, its share of the step the vector kernels';
  (c) the loop a user writes without the solver: cvr_spmv_device + torch vector operations + .item() for the five scalars, wall time per step.
Each figure is the median of --reps runs after one warm-up run (the first run of a process pays for loading the code objects and for the allocator).
A run that stops before --iters steps (a breakdown) is reported as such and not timed.  Prints one JSON line per (shape, precision) and a table in
Markdown."""
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
    """plain BiCGSTAB with torch: per step two cvr_spmv_device, six vector operations and four read-backs"""
    n = A.nrows
    x = torch.zeros(n, dtype=tdt, device="cuda")
    r = bt.clone()
    rhat = r.clone()
    p = torch.zeros(A.info.x_elems, dtype=tdt, device="cuda")
    s = torch.zeros(A.info.x_elems, dtype=tdt, device="cuda")
    p[:n] = r
    v = torch.zeros(A.info.yext_elems, dtype=tdt, device="cuda")
    t = torch.zeros(A.info.yext_elems, dtype=tdt, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rho = torch.dot(rhat, r).item()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        A.spmv_device(p.data_ptr(), v.data_ptr(), stream=st)
        alpha = rho / torch.dot(rhat, v[:n]).item()
        torch.add(r, v[:n], alpha=-alpha, out=s[:n])
        A.spmv_device(s.data_ptr(), t.data_ptr(), stream=st)
        omega = torch.dot(t[:n], s[:n]).item() / torch.dot(t[:n], t[:n]).item()
        x.add_(p[:n], alpha=alpha).add_(s[:n], alpha=omega)
        torch.add(s[:n], t[:n], alpha=-omega, out=r)
        rho1 = torch.dot(rhat, r).item()
        beta = (rho1 / rho) * (alpha / omega)
        p[:n].add_(v[:n], alpha=-omega).mul_(beta).add_(r)
        rho = rho1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="web,banded,lj")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--c", type=float, default=0.95)
    args = ap.parse_args()
    rows = []
    for shape in args.shapes.split(","):
        n, rp, ci = pattern(shape)
        n, _, rp2, ci2, va64 = synth.nonsym_from_pattern(n, rp, ci, c=args.c)
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va64.astype(dtype))
            bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), col_panels=A.info.col_panels, col_phases=A.info.col_phases,
                       interleave=A.info.interleave, iters=args.iters, vector_mb=18 * n * np.dtype(dtype).itemsize / 1e6)
            A.bench(20, 20)
            out["spmv_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
            for every in (1, 4, 8, 16, args.iters):
                ts = []
                for rep in range(args.reps + 1):
                    xt.zero_()
                    torch.cuda.synchronize()
                    res = A.bicgstab(bt.data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=args.iters, check_every=every)
                    if res.iterations != args.iters:
                        out["stopped"] = dict(iterations=res.iterations, status=res.status)
                        break
                    if rep:
                        ts.append(res.seconds / res.iterations)
                out[f"step_us_every_{every}"] = statistics.median(ts) * 1e6 if ts else float("nan")
            out["own_us_at_8"] = out["step_us_every_8"] - 2 * out["spmv_us"]
            out["vector_share_at_8"] = out["own_us_at_8"] / out["step_us_every_8"]
            user_loop(A, bt, 4, tdt)
            out["user_loop_us"] = statistics.median(user_loop(A, bt, args.iters, tdt) for _ in range(args.reps)) * 1e6
            print(json.dumps(out), flush=True)
            rows.append(out)
            A.close()
    it = args.iters
    print(f"\n| shape | type | SpMV alone | BiCGSTAB step, check_every 1 | 4 | 8 | 16 | {it} | own cost at 8 | its share of the step | torch loop | 18 n sizeof(T) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        print(f"| {o['shape']} | {o['prec']} | {o['spmv_us']:.1f} us | {o['step_us_every_1']:.1f} | {o['step_us_every_4']:.1f} | {o['step_us_every_8']:.1f} | "
              f"{o['step_us_every_16']:.1f} | {o[f'step_us_every_{it}']:.1f} | {o['own_us_at_8']:.1f} us | {100 * o['vector_share_at_8']:.0f} % | "
              f"{o['user_loop_us']:.1f} us | {o['vector_mb']:.0f} MB |")


if __name__ == "__main__":
    main()
