#!/usr/bin/env python3
"""tools/cg_multi_probe.py [--shapes web,banded,lj] [--iters 64] [--reps 5] [--nvecs 2,4,8] -- what a conjugate-gradient step costs per
right-hand side when the columns are solved together (needs a GPU).

For each shape (web-Google-like, banded 2 M rows, soc-LiveJournal1-like), made SPD by synth.spd_from_pattern, in fp64 and fp32, with rtol = 0 and
max_iters = --iters (every run does the same work, no column stops early) at the default check_every, per step and per column:
  (a) cvr_cg_multi_device with nvec columns on a handle made with nvec = 8 (the plain layout);
  (b) nvec calls of cvr_cg_device, one after the other, on that same handle;
  (c) nvec calls of cvr_cg_device on a handle made with default options (the layout the rules pick for one vector).
(b) and (c) are the single solver as it is: the yardstick.  Each figure is the solver's own `seconds` (HIP events around everything enqueued,
summed over the calls of (b) and (c)) / (iterations * nvec), the median of --reps runs after one warm-up run.
Prints one JSON line per (shape, precision, nvec) and a table in Markdown."""
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
    elif shape == "lj":
        n, _, rp, ci, _ = synth.livejournal_like()
    else:
        raise SystemExit(f"unknown shape {shape}")
    return n, rp, ci


def median_of(run, reps):
    run()
    return statistics.median(run() for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="web,banded,lj")
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nvecs", default="2,4,8")
    args = ap.parse_args()
    it = args.iters
    rows = []
    for shape in args.shapes.split(","):
        n, rp, ci = pattern(shape)
        n, _, rp2, ci2, va64 = synth.spd_from_pattern(n, rp, ci)
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            va = va64.astype(dtype)
            P = cvr_amd.CvrMatrix(n, n, rp2, ci2, va, nvec=8)
            D = cvr_amd.CvrMatrix(n, n, rp2, ci2, va)
            B = np.random.default_rng(1).standard_normal((n, 8)).astype(dtype)
            B[:, 0] = synth.x_rand(n)
            cols = [torch.from_numpy(np.ascontiguousarray(B[:, j])).cuda() for j in range(8)]
            xt = torch.zeros(n, dtype=tdt, device="cuda")

            def singles(A, k):
                total = 0.0
                for j in range(k):
                    xt.zero_()
                    torch.cuda.synchronize()
                    res = A.cg(cols[j].data_ptr(), xt.data_ptr(), rtol=0.0, max_iters=it)
                    assert res.iterations == it, (res.iterations, res.status)
                    total += res.seconds
                return total / (it * k)

            for k in (int(v) for v in args.nvecs.split(",")):
                Bt = torch.from_numpy(np.ascontiguousarray(B[:, :k])).cuda()
                Xt = torch.zeros((n, k), dtype=tdt, device="cuda")

                def block():
                    Xt.zero_()
                    torch.cuda.synchronize()
                    res = P.cg_multi(Bt.data_ptr(), k, Xt.data_ptr(), k, k, rtol=0.0, max_iters=it)
                    assert all(r.iterations == it for r in res), [(r.iterations, r.status) for r in res]
                    return res[0].seconds / (it * k)

                out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), nvec=k, iters=it,
                           default_layout=dict(col_panels=D.info.col_panels, col_phases=D.info.col_phases, interleave=D.info.interleave),
                           multi_us=median_of(block, args.reps) * 1e6,
                           singles_same_handle_us=median_of(lambda: singles(P, k), args.reps) * 1e6,
                           singles_default_handle_us=median_of(lambda: singles(D, k), args.reps) * 1e6)
                print(json.dumps(out), flush=True)
                rows.append(out)
            P.close()
            D.close()
    print("\n| shape | type | nvec | (a) cg_multi, us per step and column | (b) singles, same handle | (c) singles, default handle | (b) / (a) | (c) / (a) |")
    print("|---|---|---|---|---|---|---|---|")
    for o in rows:
        a, b, c = o["multi_us"], o["singles_same_handle_us"], o["singles_default_handle_us"]
        print(f"| {o['shape']} | {o['prec']} | {o['nvec']} | {a:.1f} | {b:.1f} | {c:.1f} | {b / a:.2f} | {c / a:.2f} |")


if __name__ == "__main__":
    main()
