#!/usr/bin/env python3
"""tools/eig_probe.py [--ncv 30] [--reps 5] [--scale 1.0] [--log profiles/eig_probe.log] -- what the thick-restart Lanczos eigensolver costs on the
device, by column (needs a GPU).

On the bench's web-Google-shaped matrix made symmetric (synth.spd_from_pattern: I + c D^-1/2 W D^-1/2) and on a banded symmetric one of the same order,
in fp64 and fp32:
  (a) the step with column j: cvr_eigsh_device with nev = 1, tol = 0, max_restarts = 0 and no vectors is one cycle of ncv steps and one read-back, so
      seconds at ncv = j + 1 minus seconds at ncv = j is the step with column j (the SpMV and the five vector launches), for every j from 3 on;
  (b) the SpMV alone on the same handle (cvr_spmv_bench), and GMRES's step at the same column on the same handle (tools/gmres_probe.py's difference:
      cvr_gmres_device with rtol = 0 and one batch, seconds at max_iters = j + 1 minus at max_iters = j);
  (c) a cycle behind a restart, seconds at max_restarts = 2 minus at max_restarts = 1 (the restart product, its two copies, the steps k .. ncv - 1, the
      read-back and the projected problem on the host), and the restart alone: that cycle minus the sum of its steps from (a) (columns below 3 are
      taken as column 3);
  (d) what cvr_chebyshev_bounds returns next to the extreme eigenvalues cvr_eigsh finds on the same handle (tol = 1e-6, nev = 1 at either end).
Each figure is the median of --reps runs after one warm-up run.  Prints one JSON line per matrix and precision and a table in Markdown; --log writes
the same text to a file."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncv", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    m = args.ncv
    cols = sorted({j for j in (3, 7, 8, 15, 16, m - 1) if 3 <= j < m})
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    n, _, rp, ci, _ = synth.web_google_like(scale=args.scale)
    graph = synth.spd_from_pattern(n, rp, ci)
    band = synth.spd_from_pattern(n, *synth.banded_sym(n, half_band=13)[2:4])
    rows = []
    for name, (n, _, rp2, ci2, va64) in (("web-Google-like, symmetric", graph), ("banded, half band 13", band)):
        for dtype in (np.float64, np.float32):
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va64.astype(dtype))
            v0 = torch.from_numpy(synth.x_rand(n).astype(dtype)).cuda()
            xt = torch.zeros(n, dtype=tdt, device="cuda")
            out = dict(matrix=name, prec=np.dtype(dtype).name, n=int(n), nnz=int(rp2[-1]), ncv=m)
            A.bench(20, 20)
            out["spmv_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6

            def cycle(ncv, restarts=0):
                ts = []
                for rep in range(args.reps + 1):
                    _, _, res = A.eigsh(1, "LA", ncv=ncv, tol=0.0, v0=v0, max_restarts=restarts, vectors=False)
                    if res.status != capi.EIG_MAX_RESTARTS or res.restarts != restarts:
                        raise SystemExit(f"ncv = {ncv}: status {res.status} after {res.restarts} restarts")
                    if rep:
                        ts.append(res.seconds)
                return statistics.median(ts)

            def gmres(k):
                ts = []
                for rep in range(args.reps + 1):
                    xt.zero_()
                    torch.cuda.synchronize()
                    _, res = A.gmres(v0, x0=xt, restart=m, rtol=0.0, max_iters=k, check_every=max(k, 1))
                    if res.iterations != k:
                        raise SystemExit(f"GMRES stopped after {res.iterations} of {k} steps, status {res.status}")
                    if rep:
                        ts.append(res.seconds)
                return statistics.median(ts)

            t = {c: cycle(c) for c in range(3, m + 1)}
            step = {j: t[j + 1] - t[j] for j in range(3, m)}
            for j in cols:
                out[f"step_us_col_{j}"] = step[j] * 1e6
                out[f"gmres_step_us_col_{j}"] = (gmres(j + 1) - gmres(j)) * 1e6
            later = cycle(m, 2) - cycle(m, 1)          # k = 1 kept column at tol = 0: the steps 1 .. m - 1
            out["cycle_us"] = t[m] * 1e6
            out["later_cycle_us"] = later * 1e6
            out["restart_us"] = (later - sum(step[max(j, 3)] for j in range(1, m))) * 1e6
            lo, hi = A.chebyshev_bounds()
            la, _, ra = A.eigsh(1, "LA", tol=1e-6, vectors=False)
            sa, _, rs = A.eigsh(1, "SA", tol=1e-6, vectors=False)
            out.update(cheb_lmin=lo, cheb_lmax=hi, eig_max=float(la[0]) if len(la) else None, eig_min=float(sa[0]) if len(sa) else None,
                       eig_max_status=ra.status, eig_min_status=rs.status, eig_max_steps=ra.spmv_count, eig_min_steps=rs.spmv_count)
            say(json.dumps(out))
            rows.append(out)
            A.close()
    say()
    say("| matrix | type | SpMV alone | column j | Lanczos step | GMRES step | ratio |")
    say("|---|---|---|---|---|---|---|")
    for o in rows:
        for j in cols:
            a, g = o[f"step_us_col_{j}"], o[f"gmres_step_us_col_{j}"]
            say(f"| {o['matrix']} | {o['prec']} | {o['spmv_us']:.1f} us | {j} | {a:.1f} us | {g:.1f} us | {a / g:.2f} |")
    say()
    say(f"| matrix | type | first cycle ({m} steps) | cycle behind a restart | restart alone | Chebyshev bounds | eigenvalues found (steps) |")
    say("|---|---|---|---|---|---|---|")
    for o in rows:
        say(f"| {o['matrix']} | {o['prec']} | {o['cycle_us']:.0f} us | {o['later_cycle_us']:.0f} us | {o['restart_us']:.0f} us | "
            f"[{o['cheb_lmin']:.4g}, {o['cheb_lmax']:.4g}] | [{o['eig_min']:.6g} ({o['eig_min_steps']}), {o['eig_max']:.6g} ({o['eig_max_steps']})] |")
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
