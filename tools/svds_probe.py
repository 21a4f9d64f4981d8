#!/usr/bin/env python3
"""tools/svds_probe.py [--ncv 20] [--reps 5] [--scale 1.0] [--gram-scale 0.1] [--log profiles/svds_probe.log] -- what the thick-restart
Golub-Kahan-Lanczos solver costs on the device (needs a GPU).  Recorded, not gated.

On the bench's web-Google-shaped matrix (synth.web_google_like, nonsymmetric, square) and on a rectangular banded one (synth.rect_banded, twice as
many rows as columns), in fp64 and fp32, with the second handle made by transpose = 1:
  (a) the step with column j: cvr_svds_device with nev = 1, tol = 0, max_restarts = 0 and no vectors is one cycle of ncv steps and one read-back, so
      seconds at ncv = j + 1 minus seconds at ncv = j is step j (two SpMVs and ten vector launches), for a few j from 3 on;
  (b) the two SpMVs alone, one per handle (cvr_spmv_bench);
  (c) the nev = 4 solve to tol = 1e-6 with its restarts and products;
  (d) the same four values by the route the solver replaces, on the web-Google shape at --gram-scale: A^T A formed by the device SpGEMM, a handle of
      it, and cvr_eigsh (largest, nev = 4, tol = 1e-12: the eigenvalues are the squares, so the tolerance is squared too); the fill nnz(A^T A) / nnz(A),
      the time to form it (host wall clock around the creation, a median after a warm-up like the rest) and the time of either solve (HIP events),
      and the largest difference of the values.
Each time is the median of --reps runs after one warm-up run.  Prints one JSON line per matrix and precision and a table in Markdown; --log writes
the same text to a file."""
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
from cvr_amd import capi, synth    # noqa: E402


def transpose_csr(nr, nc, rp, ci, va):
    rows = np.repeat(np.arange(nr), np.diff(rp))
    order = np.lexsort((rows, ci))
    rpt = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(rpt, np.asarray(ci, dtype=np.int64) + 1, 1)
    return nc, nr, np.cumsum(rpt), rows[order].astype(np.int32), np.asarray(va)[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncv", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--gram-scale", type=float, default=0.1)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    m = args.ncv
    cols = sorted({j for j in (3, 7, 8, 15, m - 1) if 3 <= j < m})
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def median_seconds(fn):
        ts = []
        for rep in range(args.reps + 1):
            t = fn()
            if rep:
                ts.append(t)
        return statistics.median(ts)

    graph = synth.web_google_like(scale=args.scale)
    nb = int(graph[0])
    band = synth.rect_banded(2 * nb, nb, half_band=6)
    rows = []
    for name, (nr, nc, rp, ci, va) in (("web-Google-like", graph), ("rectangular band, half band 6", band)):
        for dtype in (np.float64, np.float32):
            vals = np.asarray(va).astype(dtype)
            A = cvr_amd.CvrMatrix(nr, nc, rp, ci, vals)
            AT = cvr_amd.CvrMatrix(nr, nc, rp, ci, vals, transpose=1)
            v0 = torch.from_numpy(synth.x_rand(nc).astype(dtype)).cuda()
            out = dict(matrix=name, prec=np.dtype(dtype).name, nrows=int(nr), ncols=int(nc), nnz=int(rp[-1]), ncv=m)
            for H in (A, AT):
                H.bench(20, 20)
            out["spmv_a_us"] = statistics.median(A.bench(5, 50) for _ in range(args.reps)) * 1e6
            out["spmv_at_us"] = statistics.median(AT.bench(5, 50) for _ in range(args.reps)) * 1e6

            def cycle(ncv):
                def once():
                    _, _, _, res = A.svds(AT, v0, 1, ncv, 0.0, 0, vectors=False)
                    if res.status != capi.EIG_MAX_RESTARTS:
                        raise SystemExit(f"ncv = {ncv}: status {res.status}")
                    return res.seconds
                return median_seconds(once)

            need = sorted({c for j in cols for c in (j, j + 1)})
            t = {c: cycle(c) for c in need}
            for j in cols:
                out[f"step_us_col_{j}"] = (t[j + 1] - t[j]) * 1e6
            sv, _, _, res = A.svds(AT, v0, 4, m, 1e-6, 200)
            out.update(solve_status=res.status, solve_restarts=res.restarts, solve_products=res.spmv_count, svals=[float(s) for s in sv],
                       solve_ms=median_seconds(lambda: A.svds(AT, v0, 4, m, 1e-6, 200)[3].seconds) * 1e3)
            say(json.dumps(out))
            rows.append(out)
            A.close()
            AT.close()

    # (d) the route through A^T A
    gram = dict(gram_scale=args.gram_scale)
    nr, nc, rp, ci, va = synth.web_google_like(scale=args.gram_scale)
    vals = np.asarray(va).astype(np.float64)
    A = cvr_amd.CvrMatrix(nr, nc, rp, ci, vals)
    AT = cvr_amd.CvrMatrix(nr, nc, rp, ci, vals, transpose=1)
    v0 = torch.from_numpy(synth.x_rand(nc)).cuda()
    sv, _, _, res = A.svds(AT, v0, 4, m, 1e-6, 200)
    gram.update(nrows=int(nr), nnz=int(rp[-1]), svds_status=res.status, svds_restarts=res.restarts, svds_products=res.spmv_count,
                svds_ms=median_seconds(lambda: A.svds(AT, v0, 4, m, 1e-6, 200)[3].seconds) * 1e3, svals=[float(s) for s in sv])
    try:
        at_csr, a_csr = transpose_csr(nr, nc, rp, ci, vals), (nr, nc, rp, ci, vals)

        def form():          # host wall clock around the whole creation (upload, symbolic and numeric step); the last product is kept
            nonlocal G
            if G is not None:
                G.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            G = capi.SpGemm.create(at_csr, a_csr)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        G = None
        gram["spgemm_ms"] = median_seconds(form) * 1e3
        grp, gci, gva = G.export()
        G.close()
        gram["gram_nnz"] = int(grp[-1])
        gram["fill"] = float(grp[-1]) / float(rp[-1])
        N = cvr_amd.CvrMatrix(nc, nc, grp, gci, gva)
        ev, _, eres = N.eigsh(4, "LA", ncv=m, tol=1e-12, v0=v0, max_restarts=200, vectors=False)
        gram.update(eigsh_status=eres.status, eigsh_restarts=eres.restarts, eigsh_products=eres.spmv_count,
                    eigsh_ms=median_seconds(lambda: N.eigsh(4, "LA", ncv=m, tol=1e-12, v0=v0, max_restarts=200, vectors=False)[2].seconds) * 1e3,
                    sqrt_evals=[float(np.sqrt(max(e, 0.0))) for e in ev[::-1]])
        if len(ev) == len(sv):
            gram["max_difference"] = float(np.abs(np.sqrt(np.maximum(ev[::-1], 0.0)) - sv).max())
        N.close()
    except capi.CvrError as e:
        gram["gram_error"] = f"{e}"
    A.close()
    AT.close()
    say(json.dumps(gram))

    say()
    say("| matrix | type | SpMV A + SpMV A^T alone | column j | step j | step / two SpMVs |")
    say("|---|---|---|---|---|---|")
    for o in rows:
        two = o["spmv_a_us"] + o["spmv_at_us"]
        for j in cols:
            say(f"| {o['matrix']} | {o['prec']} | {o['spmv_a_us']:.1f} + {o['spmv_at_us']:.1f} us | {j} | {o[f'step_us_col_{j}']:.1f} us | {o[f'step_us_col_{j}'] / two:.2f} |")
    say()
    say("| matrix | type | nev = 4 to 1e-6 | restarts | products | status |")
    say("|---|---|---|---|---|---|")
    for o in rows:
        say(f"| {o['matrix']} | {o['prec']} | {o['solve_ms']:.2f} ms | {o['solve_restarts']} | {o['solve_products']} | {o['solve_status']} |")
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
