#!/usr/bin/env python3
"""tools/gmres_probe.py [--restart 30] [--reps 5] [--c 0.95] [--scale 1.0] -- what a GMRES(m) step costs on the device, by column (needs a GPU).

On the bench's web-Google-shaped matrix, made nonsymmetric and diagonally dominant by synth.nonsym_from_pattern (c close to 1, so that a cycle does
not reach the rounding floor), in fp64 and fp32:
  (a) the step with column j, for j = 0, 7, 8, 15, 16 and m - 1: cvr_gmres_device with rtol = 0 and check_every = max_iters (one batch, one read-back),
      seconds at max_iters = j + 1 minus seconds at max_iters = j -- both end with the same x pass but over one column more, which the difference
      keeps (a step's cost is the SpMV, the five vector launches and its share of forming x);
  (b) the SpMV alone on the same handle (cvr_spmv_bench);
  (c) the vector bytes the step moves, counted from the kernels' passes over vectors of n values: each of the two Gram-Schmidt passes reads the
      j + 1 columns twice (the sums, the update) and w once per group of 8 columns in the sums, and reads and writes w in the update; the finish reads
      w and writes v_(j+1): (4 (j + 1) + 2 ceil((j + 1) / 8) + 6) n sizeof(T) -- beside the rate of cvr_device_copy_bench.  (The partial sums every
      workgroup adds up, 8 KiB per column and workgroup, come from the cache and are not counted.)
Each figure is the median of --reps runs after one warm-up run.  Prints one JSON line per precision and a table in Markdown."""
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


def vector_bytes(j, n, itemsize):
    return (4 * (j + 1) + 2 * -(-(j + 1) // 8) + 6) * n * itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--c", type=float, default=0.95)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    m = args.restart
    cols = sorted({j for j in (0, 7, 8, 15, 16, m - 1) if 0 <= j < m})
    copy_gbs = capi.device_copy_gbs(0, 1 << 30, 10)
    n, _, rp, ci, _ = synth.web_google_like(scale=args.scale)
    n, _, rp2, ci2, va64 = synth.nonsym_from_pattern(n, rp, ci, c=args.c)
    rows = []
    for dtype in (np.float64, np.float32):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va64.astype(dtype))
        bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
        xt = torch.zeros(n, dtype=tdt, device="cuda")
        out = dict(prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), restart=m, copy_gbs=copy_gbs)
        A.bench(20, 20)
        out["spmv_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6

        def seconds(k):
            ts = []
            for rep in range(args.reps + 1):
                xt.zero_()
                torch.cuda.synchronize()
                _, res = A.gmres(bt, x0=xt, restart=m, rtol=0.0, max_iters=k, check_every=max(k, 1))
                if res.iterations != k:
                    raise SystemExit(f"stopped after {res.iterations} of {k} steps, status {res.status}")
                if rep:
                    ts.append(res.seconds)
            return statistics.median(ts)
        for j in cols:
            step = seconds(j + 1) - seconds(j)
            mb = vector_bytes(j, n, np.dtype(dtype).itemsize) / 1e6
            out[f"step_us_col_{j}"] = step * 1e6
            out[f"vector_mb_col_{j}"] = mb
            out[f"vector_gbs_col_{j}"] = mb / 1e3 / max(step - out["spmv_us"] * 1e-6, 1e-9)
        print(json.dumps(out), flush=True)
        rows.append(out)
        A.close()
    print(f"\ncopy kernel: {copy_gbs:.0f} GB/s (cvr_device_copy_bench, 1 GiB, read + write)\n")
    print("| type | SpMV alone | column j | step | step - SpMV | vector bytes | their rate over step - SpMV |")
    print("|---|---|---|---|---|---|---|")
    for o in rows:
        for j in cols:
            print(f"| {o['prec']} | {o['spmv_us']:.1f} us | {j} | {o[f'step_us_col_{j}']:.1f} us | {o[f'step_us_col_{j}'] - o['spmv_us']:.1f} us | "
                  f"{o[f'vector_mb_col_{j}']:.0f} MB | {o[f'vector_gbs_col_{j}']:.0f} GB/s |")


if __name__ == "__main__":
    main()
