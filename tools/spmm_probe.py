#!/usr/bin/env python3
"""tools/spmm_probe.py -- several vectors at once: what one cvr_spmm_device costs against nvec single-vector SpMVs.

For each shape (web-Google, a banded KKT-like matrix, soc-LiveJournal1), precision (fp64, fp32) and nvec in {1, 2, 4, 8, 16}:
  spmm      kernel time of one cvr_spmm_device on a handle created with nvec = 16 (the plain layout), X / Y packed (ldx = ldy = nvec)
  k x spmv  nvec x cvr_spmv_device on that same handle (nvec different x vectors, back to back)
  k x best  nvec x cvr_spmv_device on a default-options handle: the layout the library's rules pick for one vector
  GF/s/vec  per-vector GFLOP/s of the spmm (2 nnz flops per vector)
Kernel times are taken as bench.py takes them: HIP events on a stream of its own around `reps` back-to-back launches, behind untimed
launches worth ~30 ms.  Under `rocprofv3 --kernel-trace --stats` pass --reps 3 --warm-ms 0 to see the kernels one by one.

  python tools/spmm_probe.py [--shapes webgoogle,banded,livejournal] [--precisions fp64,fp32] [--nvecs 1,2,4,8,16] [--reps 20]
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


def shape(name):
    if name == "webgoogle":
        return synth.web_google_like()
    if name == "banded":
        return synth.banded_sym(2_000_000, 13)
    if name == "livejournal":
        return synth.livejournal_like()
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
    ap.add_argument("--shapes", default="webgoogle,banded,livejournal")
    ap.add_argument("--precisions", default="fp64,fp32")
    ap.add_argument("--nvecs", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=30.0)
    args = ap.parse_args()
    nvecs = [int(v) for v in args.nvecs.split(",")]
    kmax = max(nvecs)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    print(f"# spmm_probe: reps {args.reps}, warm-up ~{args.warm_ms:g} ms, {torch.cuda.get_device_name(0)}, {cvr_amd.version()}")
    print(f"# {'shape':<12} {'prec':<5} {'nvec':>4} {'spmm us':>10} {'k x spmv us':>12} {'k x best us':>12} {'spmm/vec':>9} {'best/vec':>9} "
          f"{'vs same':>8} {'vs best':>8} {'GF/s/vec':>9}  layout of the best")
    for name in args.shapes.split(","):
        n, nc, rp, ci, va64 = shape(name)
        nnz = int(rp[-1])
        for prec in args.precisions.split(","):
            va = va64.astype(np.float32) if prec == "fp32" else va64
            tdt = torch.float32 if prec == "fp32" else torch.float64
            P = cvr_amd.CvrMatrix(n, nc, rp, ci, va, nvec=kmax)
            D = cvr_amd.CvrMatrix(n, nc, rp, ci, va)
            i, d = P.info, D.info
            best = f"phases {d.col_phases} panels {d.col_panels} wpb {d.waves_per_block} window {d.x_window} hub {d.hub_entries} ilv {d.interleave} gang {d.gang}"
            g = torch.Generator(device=dev).manual_seed(7)
            Xall = torch.rand((nc + 1, kmax), generator=g, device=dev, dtype=torch.float64).to(tdt) * 2 - 1
            Xall[nc] = 0
            xs = [Xall[:, j].contiguous() for j in range(kmax)]
            ys = [torch.zeros(max(i.yext_elems, d.yext_elems, 1), dtype=tdt, device=dev) for _ in range(kmax)]
            torch.cuda.synchronize()
            for k in nvecs:
                X = Xall[:, :k].contiguous()
                Y = torch.zeros((max(i.yext_elems, 1), k), dtype=tdt, device=dev)
                torch.cuda.synchronize()
                t_mm = timed(lambda: P.spmm_device(X.data_ptr(), k, Y.data_ptr(), k, k, sp), st, args.reps, args.warm_ms)

                def k_spmv(A):
                    for j in range(k):
                        A.spmv_device(xs[j].data_ptr(), ys[j].data_ptr(), sp)
                t_same = timed(lambda: k_spmv(P), st, args.reps, args.warm_ms)
                t_best = timed(lambda: k_spmv(D), st, args.reps, args.warm_ms)
                gfs = 2.0 * nnz / (t_mm / k) / 1e9
                print(f"  {name:<12} {prec:<5} {k:>4} {t_mm * 1e6:>10.1f} {t_same * 1e6:>12.1f} {t_best * 1e6:>12.1f} {t_mm * 1e6 / k:>9.2f} {t_best * 1e6 / k:>9.2f} "
                      f"{t_same / t_mm:>7.2f}x {t_best / t_mm:>7.2f}x {gfs:>9.1f}  {best}", flush=True)
                del X, Y
            P.close()
            D.close()
            del Xall, xs, ys
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
