#!/usr/bin/env python3
"""tools/pcg_multi_probe.py [--shapes banded1000000,blockdiag1000000] [--iters 32] [--reps 5] [--json FILE] -- what the block-Jacobi object costs per
step and per column with several right-hand sides, and what the k-wide apply moves (needs a GPU).

Shapes: pcg_probe.py's (banded<rows>, blockdiag<rows>).  For each, in fp64 and fp32, on one handle made with nvec = 8, for block_size = 1, 8, 32 and
nvec = 1, 2, 4, 8 it measures
  (a) cvr_pcg_multi_device: seconds per step (rtol = 0 and max_iters = --iters, so every run does the same work; res.seconds / iterations) and per
      step and column, beside the paths there were before on the same handle: nvec calls of cvr_pcg_device (its step time; per column it is the
      same for every nvec) and, at block_size = 1, cvr_cg_multi_device with minv_dev = the exported W (the fused three-launch step)
  (b) the apply alone: cvr_precond_apply_multi_device between two events, GB/s over the bytes it must move (R and Z of nvec columns, W once), beside
      nvec launches of cvr_precond_apply_device on vectors of the same length and cvr_device_copy_bench; the launches go round several (object, R, Z)
      triples of 768 MiB together, so none finds its data in the last-level cache.
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
from cvr_amd import capi, synth    # noqa: E402
from pcg_probe import matrix        # noqa: E402

BLOCK_SIZES = (1, 8, 32)
NVECS = (1, 2, 4, 8)
SPREAD = 768 << 20


def median_of(fn, reps):
    fn()
    return statistics.median(fn() for _ in range(reps))


def timed(launches, count):
    """seconds per launch of `launches()` (which enqueues `count` of them on the current stream)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launches(torch.cuda.current_stream().cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="banded1000000,blockdiag1000000")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    copy_gbs = capi.device_copy_gbs()
    rows = []
    for shape in args.shapes.split(","):
        for dtype in (np.float64, np.float32):
            n, _, rp, ci, va = matrix(shape, dtype)
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            vsz = np.dtype(dtype).itemsize
            A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
            B = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 8)).astype(dtype)).cuda()
            out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp[-1]), iters=args.iters, reps=args.reps, copy_gbs=copy_gbs, cells=[])
            for bs in BLOCK_SIZES:
                wbytes = -(-n // bs) * bs * bs * vsz
                nsets = {k: min(64, max(2, -(-SPREAD // (2 * n * k * vsz + wbytes)))) for k in NVECS}
                objs = [capi.Precond.block_jacobi(rp, ci, va, bs) for _ in range(max(nsets.values()))]
                P = objs[0]
                minv = torch.from_numpy(P.export().reshape(-1)).cuda() if bs == 1 else None

                def step_us(solve):
                    def once():
                        res = solve()
                        return res.seconds / max(res.iterations, 1)
                    return median_of(once, args.reps) * 1e6

                b1, x1 = B[:, 0].contiguous(), torch.zeros(n, dtype=tdt, device="cuda")

                def single():
                    x1.zero_()
                    torch.cuda.synchronize()
                    return A.pcg(P, b1.data_ptr(), x1.data_ptr(), rtol=0.0, max_iters=args.iters)
                single_us = step_us(single)

                # the single apply over vectors that do not stay in the last-level cache
                sets = nsets[1]
                rs, zs = [b1.clone() for _ in range(sets)], [torch.zeros(n, dtype=tdt, device="cuda") for _ in range(sets)]
                apply1 = median_of(lambda: timed(lambda st: [Q.apply(r_.data_ptr(), z_.data_ptr(), stream=st) for _ in range(2) for Q, r_, z_ in zip(objs, rs, zs)], 2 * sets), args.reps)
                del rs, zs
                for nvec in NVECS:
                    Bk, Xk = B[:, :nvec].contiguous(), torch.zeros((n, nvec), dtype=tdt, device="cuda")

                    def multi():
                        Xk.zero_()
                        torch.cuda.synchronize()
                        return A.pcg_multi(P, Bk.data_ptr(), nvec, Xk.data_ptr(), nvec, nvec, rtol=0.0, max_iters=args.iters)[0]

                    def diag():
                        Xk.zero_()
                        torch.cuda.synchronize()
                        return A.cg_multi(Bk.data_ptr(), nvec, Xk.data_ptr(), nvec, nvec, rtol=0.0, max_iters=args.iters, minv_ptr=minv.data_ptr())[0]
                    cell = dict(bs=bs, nvec=nvec, step_us=step_us(multi), singles_step_us=single_us * nvec)
                    cell["step_us_per_column"] = cell["step_us"] / nvec
                    if bs == 1:
                        cell["cg_multi_diag_step_us"] = step_us(diag)
                    sets = nsets[nvec]
                    nbytes = 2 * n * nvec * vsz + wbytes
                    Rs, Zs = [Bk.clone() for _ in range(sets)], [torch.zeros((n, nvec), dtype=tdt, device="cuda") for _ in range(sets)]
                    t = median_of(lambda: timed(lambda st: [Q.apply_multi(r_.data_ptr(), nvec, z_.data_ptr(), nvec, nvec, stream=st) for _ in range(2) for Q, r_, z_ in zip(objs, Rs, Zs)], 2 * sets), args.reps)
                    del Rs, Zs
                    cell.update(apply_us=t * 1e6, apply_gbs=nbytes / t / 1e9, apply_sets=sets, apply_bytes_per_column=nbytes / nvec,
                                singles_apply_us=apply1 * 1e6 * nvec, singles_apply_gbs=(2 * n * vsz + wbytes) / apply1 / 1e9)
                    out["cells"].append(cell)
                for Q in objs:
                    Q.close()
            print(json.dumps(out), flush=True)
            rows.append(out)
            A.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print("\n| shape | type | bs | nvec | us / step | us / step / column | nvec x cvr_pcg_device, us / step | cg_multi + diag, us / step | apply us | nvec x single apply us | apply GB/s | single apply GB/s | copy GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        for c in o["cells"]:
            d = f"{c['cg_multi_diag_step_us']:.1f}" if "cg_multi_diag_step_us" in c else ""
            print(f"| {o['shape']} | {o['prec']} | {c['bs']} | {c['nvec']} | {c['step_us']:.1f} | {c['step_us_per_column']:.1f} | {c['singles_step_us']:.1f} | {d} | {c['apply_us']:.1f} | "
                  f"{c['singles_apply_us']:.1f} | {c['apply_gbs']:.0f} | {c['singles_apply_gbs']:.0f} | {o['copy_gbs']:.0f} |")


if __name__ == "__main__":
    main()
