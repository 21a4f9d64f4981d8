#!/usr/bin/env python3
"""tools/amg_block_probe.py [--grid 1000] [--ks 2,4,8] [--setups plain,smoothed,mis2] [--reps 15] [--no-solves] [--out profiles/amg_block_probe.log]
-- what one V-cycle for k right-hand sides costs beside k cycles for one (needs a GPU; fp64, one process).

On the 5-point Laplacian of a grid x grid mesh (synth.laplacian_2d), for each set-up and each k it reports
  (a) one k-wide apply (cvr_precond_apply_multi_device on a cvr_precond_amg_block object built with nvec = k, level 0 a handle of the plain layout)
      beside k applies in a row of the ordinary object of the same set-up on a handle with the default options (cvr_precond_apply_device on
      cvr_precond_amg*: the path there was before);
  (b) cvr_pcg_multi_device to rtol 1e-8 from X = 0 for k right-hand sides beside k cvr_pcg_device solves with the ordinary object (the results' own
      `seconds`, which the library takes with device events around the enqueued work; the k single solves are added);
  (c) a single-vector apply of the block object beside the ordinary object's: the price of the plain layout and of the pad launch.
Applies are timed with device events around the enqueued calls only: the median of --reps timings after two warm-up rounds.
Prints one JSON line per measurement and two tables in Markdown; everything printed also goes to --out."""
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

RTOL = 1e-8
MAX_ITERS = 2000
ORDINARY = {"plain": capi.Precond.amg, "smoothed": capi.Precond.amg_smoothed, "mis2": capi.Precond.amg_mis2}


def device_us(enqueue, reps):
    """microseconds of enqueue() on the device: the median of `reps` event timings behind two warm-up rounds"""
    for _ in range(2):
        enqueue()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enqueue()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--setups", default="plain,smoothed,mis2")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "amg_block_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    ks = [int(k) for k in args.ks.split(",")]
    say(f"# tools/amg_block_probe.py --grid {args.grid} --ks {args.ks} --setups {args.setups} --reps {args.reps}: {cvr_amd.version()}, "
        f"{torch.cuda.get_device_name(0)}; fp64, rtol {RTOL:g}, X0 = 0; medians of {args.reps} device-event timings behind 2 warm-up rounds")
    n, _, rp, ci, va = synth.laplacian_2d(args.grid)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)                   # the default options: the ordinary objects' level 0
    A8 = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)          # the plain layout: the block objects' level 0
    rng = np.random.default_rng(1)
    kmax = max(ks)
    Rh = rng.standard_normal((n, kmax))
    cols = [torch.from_numpy(np.ascontiguousarray(Rh[:, c])).cuda() for c in range(kmax)]
    zcols = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(kmax)]
    applies, solves = [], []
    for setup in args.setups.split(","):
        O = ORDINARY[setup](A, rp, ci, va)
        info = O.amg_info()
        base = dict(setup=setup, n=int(n), levels=[int(info.n[l]) for l in range(info.levels)])
        one_us = device_us(lambda: O.apply(cols[0].data_ptr(), zcols[0].data_ptr()), args.reps)
        singles = []
        if not args.no_solves:
            for c in range(kmax):
                ts, res = [], None
                for rep in range(args.reps + 1):
                    zcols[c].zero_()
                    torch.cuda.synchronize()
                    res = A.pcg(O, cols[c].data_ptr(), zcols[c].data_ptr(), rtol=RTOL, max_iters=MAX_ITERS)
                    if rep:
                        ts.append(res.seconds * 1e3)
                singles.append((statistics.median(ts), res.iterations, res.status))
        for k in ks:
            B = capi.Precond.amg_block(A8, rp, ci, va, k, setup=setup)
            Rt = torch.from_numpy(np.ascontiguousarray(Rh[:, :k])).cuda()
            Zt = torch.zeros((n, k), dtype=torch.float64, device="cuda")

            def k_ordinary():
                for c in range(k):
                    O.apply(cols[c].data_ptr(), zcols[c].data_ptr())

            out = dict(base, k=k, block_apply_us=device_us(lambda: B.apply_multi(Rt.data_ptr(), k, Zt.data_ptr(), k, k), args.reps),
                       k_ordinary_applies_us=device_us(k_ordinary, args.reps), ordinary_apply_us=one_us,
                       block_single_apply_us=device_us(lambda: B.apply(cols[0].data_ptr(), zcols[0].data_ptr()), args.reps),
                       buffer_bytes=int(B.amg_block_info().buffer_bytes))
            out["ratio"] = out["k_ordinary_applies_us"] / out["block_apply_us"]
            say(json.dumps(out))
            applies.append(out)
            if not args.no_solves:
                ts, res = [], None
                for rep in range(args.reps + 1):
                    Zt.zero_()
                    torch.cuda.synchronize()
                    res = A8.pcg_multi(B, Rt.data_ptr(), k, Zt.data_ptr(), k, k, rtol=RTOL, max_iters=MAX_ITERS)
                    if rep:
                        ts.append(res[0].seconds * 1e3)
                out = dict(base, k=k, pcg_multi_ms=statistics.median(ts), pcg_multi_steps=[r.iterations for r in res], pcg_multi_status=[r.status for r in res],
                           k_pcg_ms=sum(s[0] for s in singles[:k]), pcg_steps=[s[1] for s in singles[:k]], pcg_status=[s[2] for s in singles[:k]])
                out["ratio"] = out["k_pcg_ms"] / out["pcg_multi_ms"]
                say(json.dumps(out))
                solves.append(out)
            B.close()
        O.close()
    A.close()
    A8.close()
    say()
    say("| set-up | k | one k-wide apply | k ordinary applies | ratio | single-vector apply, block object | ordinary object |")
    say("|---|---|---|---|---|---|---|")
    for o in applies:
        say(f"| {o['setup']} | {o['k']} | {o['block_apply_us']:.1f} us | {o['k_ordinary_applies_us']:.1f} us | {o['ratio']:.2f} | {o['block_single_apply_us']:.1f} us | "
            f"{o['ordinary_apply_us']:.1f} us |")
    if solves:
        say()
        say("| set-up | k | cvr_pcg_multi to 1e-8 | steps | k cvr_pcg solves | steps | ratio |")
        say("|---|---|---|---|---|---|---|")
        for o in solves:
            say(f"| {o['setup']} | {o['k']} | {o['pcg_multi_ms']:.2f} ms | {max(o['pcg_multi_steps'])} | {o['k_pcg_ms']:.2f} ms | {max(o['pcg_steps'])} | {o['ratio']:.2f} |")
    log.close()


if __name__ == "__main__":
    main()
