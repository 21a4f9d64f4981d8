#!/usr/bin/env python3
"""tools/update_values_probe.py [--shapes web_google,livejournal,banded] [--reps N] -- what new values cost (cvr_update_values_device) against
converting again, and what a mutable handle's SpMV gives up.

Per shape and precision (CSR arrays on the device, as a GPU-resident caller holds them):
  update     one cvr_update_values_device, HIP events around `reps` back-to-back updates behind a warm-up; the bytes it moves per slot
             (map 4 + value stored + value gathered for the slots that have one) over that time, against cvr_device_copy_bench's rate
  create     cvr_create + cvr_preprocess wall time (median of 3): default options, value_dict = 0, mutable_values = 1
  spmv       cvr_spmv_bench mean of the three handles (mutable and value_dict = 0 share one image; the default may have a dictionary)
One line per measurement; the summary line per shape gives update vs create and the copy-kernel share."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cvr_amd                       # noqa: E402
from cvr_amd import capi, synth      # noqa: E402


def shape(name):
    if name == "web_google":
        return synth.web_google_like()
    if name == "livejournal":
        return synth.livejournal_like()
    if name == "banded":
        return synth.banded_sym(2_000_000, 13)
    raise SystemExit(f"unknown shape {name}")


def create(dev_arrays, nrows, ncols, f32, **kw):
    trp, tci, tva = dev_arrays
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    A = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr(), is_f32=f32, **kw)
    return A, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="web_google,livejournal,banded")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    copy_gbs = capi.device_copy_gbs(0, 1 << 30, 20)
    print(f"copy kernel: {copy_gbs:.0f} GB/s (cvr_device_copy_bench, 1 GiB, read + write)")
    for name in a.shapes.split(","):
        nrows, ncols, rp, ci, va64 = shape(name)
        for prec in ("fp64", "fp32"):
            f32 = prec == "fp32"
            dt = np.float32 if f32 else np.float64
            va = va64.astype(dt)
            dev = torch.device("cuda", 0)
            arrays = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rp.astype(np.int64), ci.astype(np.int32), va))
            t = {}
            for label, kw in (("default", {}), ("value_dict=0", dict(value_dict=0)), ("mutable", dict(mutable_values=1))):
                times = []
                for _ in range(3):
                    H, s = create(arrays, nrows, ncols, f32, **kw)
                    times.append(s)
                    H.close()
                t[label] = float(np.median(times))
            handles = {label: create(arrays, nrows, ncols, f32, **kw)[0] for label, kw in (("default", {}), ("value_dict=0", dict(value_dict=0)), ("mutable", dict(mutable_values=1)))}
            M = handles["mutable"]
            i = M.info
            v2 = torch.from_numpy(((np.arange(len(va)) % 1013) * 1e-3 + 0.5).astype(dt)).to(dev)
            stream = torch.cuda.current_stream()
            for _ in range(5):
                M.update_values_device(v2.data_ptr(), stream=stream.cuda_stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                M.update_values_device(v2.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            upd_s = e0.elapsed_time(e1) * 1e-3 / a.reps
            vsz = 4 if f32 else 8
            nbytes = i.nslots * (4 + vsz) + i.nnz * vsz
            gbs = nbytes / upd_s / 1e9
            spmv = {label: H.bench(20, 100) for label, H in handles.items()}
            for H in handles.values():
                H.close()
            print(f"{name} {prec}: nnz {i.nnz} slots {i.nslots} panels {i.col_panels} gang {i.gang} layout S={i.steps_per_chunk} wpb={i.waves_per_block} phases={i.col_phases}")
            print(f"  update            {upd_s * 1e6:9.1f} us   {nbytes / 1e6:8.1f} MB moved   {gbs:6.0f} GB/s = {gbs / copy_gbs:5.2f} of the copy kernel")
            for label in ("default", "value_dict=0", "mutable"):
                print(f"  create+preprocess {t[label] * 1e3:9.2f} ms   ({label})")
            print(f"  mutable - value_dict=0 create: {(t['mutable'] - t['value_dict=0']) * 1e3:+.2f} ms;  create / update: {t['mutable'] / upd_s:.0f} x (mutable), {t['value_dict=0'] / upd_s:.0f} x (value_dict=0)")
            for label in ("default", "value_dict=0", "mutable"):
                print(f"  spmv              {spmv[label] * 1e6:9.2f} us   ({label})")
            sys.stdout.flush()
            del arrays, v2
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
