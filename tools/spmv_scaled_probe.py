#!/usr/bin/env python3
"""tools/spmv_scaled_probe.py -- the scaled product y = alpha A x + beta y: what the fused write-out costs against the plain SpMV and the two-pass form.

For each shape (web-Google with the default layout, soc-LiveJournal1 with the default layout -- gang panels --, a banded matrix of 2 M rows in the
plain layout) and precision (fp64, fp32), alternated in `--rounds` rounds inside one process:
  spmv       cvr_spmv_device
  b0         cvr_spmv_scaled_device, alpha = 2.5, beta = 0 (y not read)
  resid      cvr_spmv_scaled_device, alpha = -1, beta = 1 (r = b - A x)
  resid 2p   the same on a handle made under CVR_DEBUG=scaled_two_pass: the plain product into a buffer, then an elementwise pass
The median of the rounds is printed per variant.  Kernel times are taken as bench.py takes them: HIP events on a stream of its own around `reps`
back-to-back launches, behind untimed launches worth ~30 ms.  The table also goes to profiles/r07_spmv_scaled_probe.log (--out).

  python tools/spmv_scaled_probe.py [--shapes webgoogle,livejournal,banded] [--precisions fp64,fp32] [--reps 50] [--rounds 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libcvr_amd.so: INTEGRATION.md)
import numpy as np  # noqa: E402

import cvr_amd  # noqa: E402
from cvr_amd import synth  # noqa: E402

PLAIN = dict(col_panels=1, col_phases=0, hub_table=0, interleave=0, gang=0)


def shape(name):
    if name == "webgoogle":
        return synth.web_google_like(), {}
    if name == "livejournal":
        return synth.livejournal_like(), {}
    if name == "banded":
        return synth.banded_sym(2_000_000, 13), PLAIN
    raise ValueError(name)


def timed(launch, stream, reps, warm_ms):
    """seconds per call of launch(), HIP events on `stream` around `reps` back-to-back calls behind ~warm_ms of untimed ones"""
    launch()
    torch.cuda.synchronize()
    if warm_ms > 0:
        t0 = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        one = max(time.perf_counter() - t0, 1e-6)
        for _ in range(min(2000, int(warm_ms * 1e-3 / one))):
            launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        launch()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="webgoogle,livejournal,banded")
    ap.add_argument("--precisions", default="fp64,fp32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_spmv_scaled_probe.log"))
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    emit(f"# spmv_scaled_probe: reps {args.reps}, rounds {args.rounds} (variants alternated, median shown), warm-up ~{args.warm_ms:g} ms, "
         f"{torch.cuda.get_device_name(0)}, {cvr_amd.version()}")
    emit(f"# {'shape':<12} {'prec':<5} {'spmv us':>9} {'b0 us':>9} {'resid us':>9} {'resid 2p us':>12} {'resid-spmv':>11} {'2p-spmv':>9} {'2p/resid':>9}  layout")
    for name in args.shapes.split(","):
        (n, nc, rp, ci, va64), opts = shape(name)
        for prec in args.precisions.split(","):
            va = va64.astype(np.float32) if prec == "fp32" else va64
            tdt = torch.float32 if prec == "fp32" else torch.float64
            os.environ.pop("CVR_DEBUG", None)
            F = cvr_amd.CvrMatrix(n, nc, rp, ci, va, **opts)
            os.environ["CVR_DEBUG"] = "scaled_two_pass"
            T = cvr_amd.CvrMatrix(n, nc, rp, ci, va, **opts)
            os.environ.pop("CVR_DEBUG", None)
            d = F.info
            lay = f"phases {d.col_phases} panels {d.col_panels} wpb {d.waves_per_block} window {d.x_window} hub {d.hub_entries} ilv {d.interleave} gang {d.gang}"
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.rand(nc + 1, generator=g, device=dev, dtype=torch.float64).to(tdt) * 2 - 1
            x[nc] = 0
            y = torch.rand(max(d.yext_elems, T.info.yext_elems, 1), generator=g, device=dev, dtype=torch.float64).to(tdt)
            torch.cuda.synchronize()
            variants = {
                "spmv": lambda: F.spmv_device(x.data_ptr(), y.data_ptr(), sp),
                "b0": lambda: F.spmv_scaled_device(x.data_ptr(), y.data_ptr(), 2.5, 0.0, sp),
                "resid": lambda: F.spmv_scaled_device(x.data_ptr(), y.data_ptr(), -1.0, 1.0, sp),
                "resid2p": lambda: T.spmv_scaled_device(x.data_ptr(), y.data_ptr(), -1.0, 1.0, sp),
            }
            ts = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, f in variants.items():
                    y.uniform_(-1, 1)          # (resid over and over would grow y without bound)
                    ts[k].append(timed(f, st, args.reps, args.warm_ms))
            m = {k: float(np.median(v)) * 1e6 for k, v in ts.items()}
            emit(f"  {name:<12} {prec:<5} {m['spmv']:>9.2f} {m['b0']:>9.2f} {m['resid']:>9.2f} {m['resid2p']:>12.2f} {m['resid'] - m['spmv']:>+11.2f} "
                 f"{m['resid2p'] - m['spmv']:>+9.2f} {m['resid2p'] / m['resid']:>8.2f}x  {lay}")
            spread = {k: (min(v) * 1e6, max(v) * 1e6) for k, v in ts.items()}
            emit("    spread (min - max over rounds): " + ", ".join(f"{k} {a:.2f}-{b:.2f}" for k, (a, b) in spread.items()))
            F.close()
            T.close()
            del x, y
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
