#!/usr/bin/env python3
"""tools/transpose_probe.py -- the handle of A^T (cvr_options.transpose): what building it on the device costs against the other routes.

For each shape (web-Google, soc-LiveJournal1; fp64, default options, A's CSR already in device memory -- the GPU-resident caller of the
issue), in `--rounds` rounds inside one process, medians printed:
  T_pre(A^T)      cvr_create(transpose = 1) + cvr_preprocess from A's device arrays; upload_s of that handle = the transpose + copies
  T_pre(T)        cvr_create + cvr_preprocess of a pre-transposed T (device arrays): what the handle costs without the transpose
  host route      A's CSR to the host, the transpose there (scipy csr -> csr of A^T), T back to the device: what a caller does today
  csr2csc         rocSPARSE's csr2csc (numeric) on the same device CSR (libcvr_cmp.so), per call
  spmv A / A^T    cvr_spmv_bench of A's handle and of A^T's (default layouts)
The transpose kernels' own times come from a run of this script under `rocprofv3 --kernel-trace --stats` (--rounds 1).
The table also goes to --out (default profiles/r08_transpose_probe.log; '-' = stdout only).

  python tools/transpose_probe.py [--shapes webgoogle,livejournal] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
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
    if name == "livejournal":
        return synth.livejournal_like()
    raise ValueError(name)


def cmp_lib():
    L = C.CDLL(os.path.join(ROOT, "cvr_amd", "libcvr_cmp.so"))
    L.cmp_csr_create.argtypes = [C.POINTER(C.c_void_p), C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.cmp_csr2csc_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.cmp_csr_destroy.argtypes = [C.c_void_p]
    L.cmp_last_error.restype = C.c_char_p
    return L


def host_transpose(nrows, ncols, rp, ci, va):
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci, rp), shape=(nrows, ncols))
    T = A.transpose().tocsr()          # (a counting sort: csc of A = csr of A^T)
    return T.indptr, T.indices, T.data


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="webgoogle,livejournal")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_transpose_probe.log"))
    a = ap.parse_args()
    lines = [f"# tools/transpose_probe.py --rounds {a.rounds}  ({torch.cuda.get_device_name(0)}; fp64, default options, A in device memory)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    L = cmp_lib()
    for name in a.shapes.split(","):
        nrows, ncols, rp, ci, va = shape(name)
        nnz = int(rp[-1])
        say(f"## {name}: {nrows} x {ncols}, {nnz} non-zeros")
        trp, tci, tva = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rp.astype(np.int64), ci.astype(np.int32), va.astype(np.float64)))
        # T as numpy's stable transpose, for the pre-transposed handle
        pos = np.argsort(ci, kind="stable")
        rows = (np.searchsorted(rp, pos, side="right") - 1).astype(np.int32)
        Trp = np.zeros(ncols + 1, dtype=np.int64)
        Trp[1:] = np.cumsum(np.bincount(ci, minlength=ncols))
        Tci, Tva = torch.from_numpy(rows).cuda(), torch.from_numpy(np.ascontiguousarray(va[pos])).cuda()
        Trp_d = torch.from_numpy(Trp).cuda()
        torch.cuda.synchronize()
        res = {k: [] for k in ("pre_t", "up_t", "pre_T", "up_T", "host_d2h", "host_tr", "host_h2d", "csr2csc", "spmv_A", "spmv_At")}
        c = C.c_void_p()
        rc = L.cmp_csr_create(C.byref(c), nrows, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
        if rc:
            raise SystemExit(f"cmp_csr_create: {L.cmp_last_error()}")
        for r in range(a.rounds):
            t0 = time.perf_counter()
            H = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr(), transpose=1)
            res["pre_t"].append(time.perf_counter() - t0)
            res["up_t"].append(H.info.upload_s)
            t0 = time.perf_counter()
            R = cvr_amd.CvrMatrix.from_device(ncols, nrows, Trp_d.data_ptr(), Tci.data_ptr(), Tva.data_ptr())
            res["pre_T"].append(time.perf_counter() - t0)
            res["up_T"].append(R.info.upload_s)
            R.close()
            # the host route: A to the host, transpose there, T back
            t0 = time.perf_counter()
            hrp, hci, hva = trp.cpu().numpy(), tci.cpu().numpy(), tva.cpu().numpy()
            t1 = time.perf_counter()
            Hrp, Hci, Hva = host_transpose(nrows, ncols, hrp, hci, hva)
            t2 = time.perf_counter()
            back = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (Hrp.astype(np.int64), Hci.astype(np.int32), Hva)]
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            del back
            res["host_d2h"].append(t1 - t0)
            res["host_tr"].append(t2 - t1)
            res["host_h2d"].append(t3 - t2)
            s, last = C.c_double(), C.c_longlong()
            rc = L.cmp_csr2csc_bench(c, 2, 10, C.byref(s), C.byref(last))
            if rc:
                raise SystemExit(f"cmp_csr2csc_bench: {L.cmp_last_error()}")
            assert last.value == nnz, (last.value, nnz)
            res["csr2csc"].append(s.value)
            A = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr())
            res["spmv_A"].append(A.bench(20, 200))
            res["spmv_At"].append(H.bench(20, 200))
            if r == 0:
                say(f"  A   : layout col_panels={A.info.col_panels} col_phases={A.info.col_phases} wpb={A.info.waves_per_block} interleave={A.info.interleave} gang={A.info.gang}")
                say(f"  A^T : layout col_panels={H.info.col_panels} col_phases={H.info.col_phases} wpb={H.info.waves_per_block} interleave={H.info.interleave} gang={H.info.gang}")
            A.close()
            H.close()
        L.cmp_csr_destroy(c)
        ms = {k: median(v) * 1e3 for k, v in res.items()}
        host = ms["host_d2h"] + ms["host_tr"] + ms["host_h2d"]
        say(f"  T_pre(A^T) create+preprocess from A  {ms['pre_t']:9.2f} ms   (upload_s {ms['up_t']:.2f} ms: transpose + copies)")
        say(f"  T_pre(T)   pre-transposed T          {ms['pre_T']:9.2f} ms   (upload_s {ms['up_T']:.2f} ms)")
        say(f"  transpose on the device (difference) {ms['pre_t'] - ms['pre_T']:9.2f} ms   (upload_s difference {ms['up_t'] - ms['up_T']:.2f} ms)")
        say(f"  host route: D2H {ms['host_d2h']:.2f} + transpose {ms['host_tr']:.2f} + H2D {ms['host_h2d']:.2f} = {host:9.2f} ms (before any create)")
        say(f"  rocSPARSE csr2csc (numeric), per call  {ms['csr2csc']:9.3f} ms")
        say(f"  SpMV: A {ms['spmv_A'] * 1e3:8.1f} us   A^T {ms['spmv_At'] * 1e3:8.1f} us")
        del trp, tci, tva, Tci, Tva, Trp_d
        torch.cuda.empty_cache()
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
