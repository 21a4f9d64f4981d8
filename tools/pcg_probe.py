#!/usr/bin/env python3
"""tools/pcg_probe.py [--shapes banded2000000,blockdiag2000000] [--iters 32] [--reps 5] [--json FILE] -- what block-Jacobi costs per step and what it
saves in steps (needs a GPU).

Shapes: banded<rows> (synth.banded_sym made SPD by synth.spd_from_pattern: kappa <= 3, nothing for a preconditioner to win) and blockdiag<rows>
(synth.block_diag_spd with blocks of 8 and condition 1e3: the case block-Jacobi is for).  For each, in fp64 and fp32, and for
  cg        cvr_cg_device without a preconditioner
  cg+diag   cvr_cg_device with minv_dev = the inverse diagonal (the block_size = 1 object's exported W)
  pcg bs    cvr_pcg_device at block_size = 1, 4, 8, 16, 32
it measures
  (a) seconds per step: rtol = 0 and max_iters = --iters, so every run does the same work; res.seconds / iterations
  (b) iterations and seconds to rtol = 1e-8 (max_iters = 1000)
  (c) the build: wall seconds of cvr_precond_block_jacobi from host arrays (the copies of the CSR included)
  (d) the plain apply: cvr_precond_apply_device between two events, GB/s over the bytes it must move (r, z and W once), beside cvr_device_copy_bench;
      the launches go round several (object, r, z) triples of 768 MiB together, so none finds its data in the last-level cache.
Each figure is the median of --reps runs after one warm-up run.  "pcg 1 / cg+diag" is the ratio of (a): the four-launch step against the fused
three-launch one on the same handle in the same process.  Prints one JSON line per (shape, precision) and a table in Markdown."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvr_amd                      # noqa: E402
from cvr_amd import capi, synth    # noqa: E402

BLOCK_SIZES = (1, 4, 8, 16, 32)


def matrix(shape, dtype):
    m = re.fullmatch(r"(banded|blockdiag)(\d+)", shape)
    if not m:
        raise SystemExit(f"unknown shape {shape}: banded<rows> or blockdiag<rows>")
    rows = int(m.group(2))
    if m.group(1) == "banded":
        n, _, rp, ci, _ = synth.banded_sym(rows)
        return synth.spd_from_pattern(n, rp, ci, dtype=dtype)
    return synth.block_diag_spd(rows, 8, cond=1e3, dtype=dtype)


def median_of(fn, reps):
    fn()
    return statistics.median(fn() for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="banded2000000,blockdiag2000000")
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
            A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
            bt = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(shape=shape, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp[-1]), iters=args.iters, reps=args.reps, copy_gbs=copy_gbs, variants={})

            def solve(P, minv, **kw):
                xt.zero_()
                torch.cuda.synchronize()
                if P is not None:
                    return A.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw)
                return A.cg(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if minv is None else minv.data_ptr(), **kw)

            def measure(name, P, minv, extra):
                def step():
                    res = solve(P, minv, rtol=0.0, max_iters=args.iters)
                    return res.seconds / max(res.iterations, 1)
                v = dict(extra, step_us=median_of(step, args.reps) * 1e6)
                res = solve(P, minv, rtol=1e-8, max_iters=1000)
                v.update(iterations=res.iterations, status=res.status, solve_ms=median_of(lambda: solve(P, minv, rtol=1e-8, max_iters=1000).seconds, args.reps) * 1e3)
                out["variants"][name] = v

            measure("cg", None, None, {})
            for bs in BLOCK_SIZES:
                def build():
                    t0 = time.perf_counter()
                    P = capi.Precond.block_jacobi(rp, ci, va, bs)
                    t = time.perf_counter() - t0
                    P.close()
                    return t
                build_ms = median_of(build, min(args.reps, 3)) * 1e3
                P = capi.Precond.block_jacobi(rp, ci, va, bs)
                if bs == 1:
                    minv = torch.from_numpy(P.export().reshape(-1)).cuda()
                    measure("cg+diag", None, minv, {})

                # the apply over buffers that do not stay in the 256 MiB last-level cache between two launches: `sets` triples (object, r, z) of
                # 768 MiB together, visited in turn, so every launch reads r and W and writes z in HBM as the copy yardstick does
                nbytes = (2 * n + P.info.nblocks * bs * bs) * vsz
                sets = min(64, max(2, -(-(768 << 20) // nbytes)))
                objs = [P] + [capi.Precond.block_jacobi(rp, ci, va, bs) for _ in range(sets - 1)]
                rs = [bt.clone() for _ in range(sets)]
                zs = [torch.zeros(n, dtype=tdt, device="cuda") for _ in range(sets)]

                def apply_s():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    st = torch.cuda.current_stream().cuda_stream
                    e0.record()
                    for _ in range(2):
                        for Q, r_, z_ in zip(objs, rs, zs):
                            Q.apply(r_.data_ptr(), z_.data_ptr(), stream=st)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1) * 1e-3 / (2 * sets)
                apply = median_of(apply_s, args.reps)
                for Q in objs[1:]:
                    Q.close()
                del rs, zs, objs
                measure(f"pcg {bs}", P, None, dict(build_ms=build_ms, identity_blocks=int(P.info.identity_blocks), apply_us=apply * 1e6, apply_gbs=nbytes / apply / 1e9, apply_sets=sets))
                P.close()
            out["pcg1_over_cg_diag"] = out["variants"]["pcg 1"]["step_us"] / out["variants"]["cg+diag"]["step_us"]
            print(json.dumps(out), flush=True)
            rows.append(out)
            A.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print("\n| shape | type | variant | us / step | steps to 1e-8 | solve ms | build ms | apply us | apply GB/s | copy GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        for name, v in o["variants"].items():
            b = f"{v['build_ms']:.1f} | {v['apply_us']:.1f} | {v['apply_gbs']:.0f}" if "build_ms" in v else "| |"
            print(f"| {o['shape']} | {o['prec']} | {name} | {v['step_us']:.1f} | {v['iterations']} | {v['solve_ms']:.2f} | {b} | {o['copy_gbs']:.0f} |")
        print(f"| {o['shape']} | {o['prec']} | pcg 1 / cg+diag, us / step | {o['pcg1_over_cg_diag']:.3f} | | | | | | |")


if __name__ == "__main__":
    main()
