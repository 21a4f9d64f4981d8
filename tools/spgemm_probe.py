#!/usr/bin/env python3
"""tools/spgemm_probe.py [--workloads laplacian,web,galerkin] [--grid 1000] [--web-scale 0.5] [--reps 3] [--out profiles/spgemm_probe.log] -- what
the sparse matrix-matrix product costs on the device (needs a GPU; fp64, one process).

Workloads: A A on the 5-point Laplacian of a grid x grid mesh; A A on a reduced web-Google-shaped matrix (synth.web_google_like: power-law rows; at
the default scale 0.5 three rows have more than 4096 products and reach the spill class, at scale 0.1 none does); P^T (A P) on the Laplacian with the aggregates of Precond.amg's level 0.  For each product it reports the shape, the
products, nnz(C) and the rows of the four classes, and the median over --reps creations from device arrays of
  (a) the symbolic step and the numeric step of cvr_spgemm_create (cvr_spgemm_info_t.symbolic_s / numeric_s: host seconds up to the read-back of
      nnz(C), and behind it),
  (b) a numeric re-run (cvr_spgemm_numeric_device with the same values, timed to the stream's idle),
beside the host twin's two calls (cvr_spgemm_host, one thread).  libcvr_cmp.so carries no rocSPARSE SpGEMM comparator: the host twin is the yardstick
here.  Under CVR_DEBUG=spgemm_limits=1:1 every non-empty row is a spill row, under =1:32 every row of the Laplacian's product a block row: the
same rows in the three classes give each class's cost per product.  Prints one JSON line per product and a table in Markdown; everything printed also goes to --out."""
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


def sorted_rows(n, ncols, rp, ci, va):
    """the same matrix with every row ascending in column and duplicates summed (B's requirement)"""
    rp, ci, va = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(va, dtype=np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    key = rows * ncols + ci
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.bincount(inv, weights=va, minlength=len(uniq))
    out_rp = np.r_[0, np.cumsum(np.bincount(uniq // ncols, minlength=n))].astype(np.int64)
    return n, ncols, out_rp, (uniq % ncols).astype(np.int32), vals


class Dev:
    def __init__(self, csr):
        self.n, self.ncols = csr[0], csr[1]
        self.t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (np.asarray(csr[2], dtype=np.int64), np.asarray(csr[3], dtype=np.int32), np.asarray(csr[4], dtype=np.float64))]
        torch.cuda.synchronize()

    def tuple(self):
        return (self.n, self.ncols) + tuple(t.data_ptr() for t in self.t)


def measure(name, a, b, reps, say, b_dev=None):
    """a, b: host tuples; returns the last object (the caller closes it)"""
    da, db = Dev(a), b_dev or Dev(b)
    bt = db.tuple()
    capi.SpGemm.from_device(da.tuple(), bt).close()
    sym, num, rerun = [], [], []
    g = None
    for _ in range(reps):
        if g is not None:
            g.close()
        torch.cuda.synchronize()
        g = capi.SpGemm.from_device(da.tuple(), bt)
        i = g.info()
        sym.append(i.symbolic_s)
        num.append(i.numeric_s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.numeric(da.t[2].data_ptr(), bt[4])
        torch.cuda.synchronize()
        rerun.append(time.perf_counter() - t0)
    host_ms = None
    if b is not None:
        t0 = time.perf_counter()
        capi.spgemm_host(a, b)
        host_ms = (time.perf_counter() - t0) * 1e3
    out = dict(product=name, m=int(i.nrows), k=int(i.inner), n=int(i.ncols), products=int(i.products), nnz=int(i.nnz), max_row_products=int(i.max_row_products),
               rows=[int(i.rows_empty), int(i.rows_group), int(i.rows_block), int(i.rows_spill)], limits=[int(i.group_limit), int(i.block_limit)],
               symbolic_ms=statistics.median(sym) * 1e3, numeric_ms=statistics.median(num) * 1e3, rerun_ms=statistics.median(rerun) * 1e3, host_ms=host_ms)
    out["rerun_ns_per_product"] = out["rerun_ms"] * 1e6 / max(out["products"], 1)
    say(json.dumps(out))
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="laplacian,web,galerkin")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--web-scale", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spgemm_probe.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"# tools/spgemm_probe.py --workloads {args.workloads} --grid {args.grid} --web-scale {args.web_scale} --reps {args.reps}: {cvr_amd.version()}, "
        f"{torch.cuda.get_device_name(0)}; fp64; CVR_DEBUG={os.environ.get('CVR_DEBUG', '')}")
    rows = []
    for w in args.workloads.split(","):
        if w == "laplacian":
            a = synth.laplacian_2d(args.grid)
            g, o = measure(f"A A, Laplacian {args.grid} x {args.grid}", a, a, args.reps, say)
            g.close()
            rows.append(o)
        elif w == "web":
            a = sorted_rows(*synth.web_google_like(scale=args.web_scale))
            g, o = measure(f"A A, web-Google-shaped at scale {args.web_scale}", a, a, args.reps, say)
            g.close()
            rows.append(o)
        elif w == "galerkin":
            n, _, rp, ci, va = synth.laplacian_2d(args.grid)
            A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
            P = capi.Precond.amg(A, rp, ci, va)
            agg, nc = P.amg_export_level(0).agg, int(P.amg_info().n[1])
            P.close()
            A.close()
            p = (n, nc, np.arange(n + 1, dtype=np.int64), agg.astype(np.int32), np.ones(n))
            pt = (nc, n, np.r_[0, np.cumsum(np.bincount(agg, minlength=nc))].astype(np.int64), np.argsort(agg, kind="stable").astype(np.int32), np.ones(n))
            ap_obj, o = measure(f"A P, Laplacian {args.grid} x {args.grid}, {nc} aggregates", (n, n, rp, ci, va), p, args.reps, say)
            rows.append(o)

            class View:          # A P stays on the device: its view is the next product's B
                def tuple(self):
                    return ap_obj.csr_device()
            g, o = measure("P^T (A P)", pt, None, args.reps, say, b_dev=View())
            g.close()
            ap_obj.close()
            rows.append(o)
        else:
            raise SystemExit(f"unknown workload {w}")
    say()
    say("| product | m x k x n | products | nnz(C) | rows empty / group / block / spill | symbolic | numeric | numeric re-run | per product | host twin |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for o in rows:
        host = "-" if o["host_ms"] is None else f"{o['host_ms']:.1f} ms"
        say(f"| {o['product']} | {o['m']} x {o['k']} x {o['n']} | {o['products']} | {o['nnz']} | {' / '.join(map(str, o['rows']))} | {o['symbolic_ms']:.2f} ms | "
            f"{o['numeric_ms']:.2f} ms | {o['rerun_ms']:.2f} ms | {o['rerun_ns_per_product']:.2f} ns | {host} |")
    log.close()


if __name__ == "__main__":
    main()
