"""GPU (MI355X): conjugate gradients on the device -- cvr_cg_device / cvr_cg, all through the ABI, checked by the oracle's CSR loop in fp64.

The matrices are synth.spd_from_pattern over a web-Google-like pattern, a banded one and a de-duplicated R-MAT: A = I + 0.5 D^-1/2 W D^-1/2 has its
spectrum in [0.5, 1.5], so kappa <= 3 and CG from a zero start obeys ||r_k|| / ||b|| <= 2 sqrt(kappa) rho^k with rho = (sqrt(3) - 1) / (sqrt(3) + 1):
at most 19 steps to 1e-10 and 8 to 1e-4.  The recurrence residual and the true one differ by O(eps * steps * kappa) -- below 1e-13 in fp64 and 1e-5
in fp32 --, so the true residual is held to 2 * rtol.

  * every layout in fp64 (rtol 1e-10) and fp32 (rtol 1e-4): converged, within the bound, true residual, the reported norms
  * bit for bit: call after call, check_every = 1 / 3 / max_iters, the host twin, arrays that are not 16-byte aligned
  * the diagonal preconditioner on S A S, and the same system without it
  * the stop states, the error returns with a real handle, and the neighbours: mutable, transposed, cached, fused handles, streams, no state left
  * the web-Google shape at full size
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases as K
import cvr_amd
import oraclelib as O
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUTS = K.LAYOUTS          # (the shared layout table: tests/cases.py)
ALL_LAYOUTS = K.ALL_LAYOUTS

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
BOUND = {np.float64: 19, np.float32: 8}          # steps to rtol for kappa <= 3 (module docstring)
MAX_ITERS = 40


@functools.lru_cache(maxsize=None)
def _pattern(name):
    if name == "web":
        n, _, rp, ci, _ = synth.web_google_like(scale=0.05)
    elif name == "banded":
        n, _, rp, ci, _ = synth.banded_sym(40000)
    else:
        n, _, rp, ci, _ = synth.rmat(14, dedupe=True)
    return n, rp, ci


@functools.lru_cache(maxsize=None)
def _spd(name, dtype):
    n, rp, ci = _pattern(name)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


MATRICES = ("web", "banded", "rmat")


def _tdt(H):
    return torch.float64 if H.dtype == np.float64 else torch.float32


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _solve(H, b, x0=None, minv=None, shift=0, stream=None, **kw):
    """cvr_cg_device on torch arrays of exactly nrows values (no pad, no tail), `shift` elements off the allocation's start; (x, result)"""
    n = H.nrows

    def dev(a):
        t = torch.empty(n + shift, dtype=_tdt(H), device="cuda")[shift:]
        t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=H.dtype)))
        return t
    bt = dev(b)
    xt = dev(np.zeros(n, dtype=H.dtype) if x0 is None else x0)
    mt = None if minv is None else dev(minv)
    torch.cuda.synchronize()
    res = H.cg(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), stream=stream, **kw)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), res


def _true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, x)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))


def _make(nrows, ncols, rp, ci, va, opts):
    try:
        return cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, **opts)
    except capi.CvrError:          # (a layout the options cannot build for this matrix)
        return None


def _check_converged(name, dtype, rp, ci, va, b, x, res, rtol, bound):
    true = _true_residual(rp, ci, va, x, b)
    print(f"{name} {np.dtype(dtype).name}: {res.iterations} steps, {res.spmv_count} SpMVs, residual / (rtol |b|) = {res.residual_norm / (rtol * res.b_norm):.3f}, "
          f"true / rtol = {true / rtol:.3f}, {res.seconds * 1e6:.0f} us")
    assert res.status == capi.CG_CONVERGED, (name, res.status, res.iterations)
    assert true <= 2 * rtol, (name, true)
    assert res.iterations <= bound, (name, res.iterations)
    assert res.residual_norm <= rtol * res.b_norm
    bn = float(np.linalg.norm(np.asarray(b, dtype=np.float64)))
    assert abs(res.b_norm - bn) <= 1e-12 * bn
    return true


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_every_layout_converges_within_the_bound(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    built = 0
    for name in MATRICES:
        n, _, rp, ci, va = _spd(name, dtype)
        A = _make(n, n, rp, ci, va, ALL_LAYOUTS[layout])
        if A is None:
            continue
        built += 1
        b = synth.x_rand(n).astype(dtype)
        x, res = _solve(A, b, rtol=RTOL[dtype], max_iters=MAX_ITERS)
        _check_converged(f"{layout}/{name}", dtype, rp, ci, va, b, x, res, RTOL[dtype], BOUND[dtype])
        A.close()
    assert built > 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", ["default", "panels", "hub", "gang"])
def test_bit_for_bit(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = _spd("web", dtype)
    A = _make(n, n, rp, ci, va, ALL_LAYOUTS[layout])
    assert A is not None, layout
    b = synth.x_rand(n).astype(dtype)
    rtol = RTOL[dtype]
    x, res = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED and 0 < res.iterations <= BOUND[dtype]

    def same(x2, r2):
        assert _bits_equal(x2, x)
        assert (r2.iterations, r2.status) == (res.iterations, res.status)
        assert r2.residual_norm == res.residual_norm and r2.b_norm == res.b_norm
    same(*_solve(A, b, rtol=rtol, max_iters=MAX_ITERS))                      # call after call
    counts = []
    for every in (1, 3, MAX_ITERS):
        x2, r2 = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
        same(x2, r2)
        counts.append(r2.spmv_count)
    assert counts[0] == res.iterations + 1                                   # the initial residual and one per step: nothing behind the stop
    assert counts == sorted(counts) and counts[-1] == MAX_ITERS + 1
    xh, rh = A.cg_host(b, rtol=rtol, max_iters=MAX_ITERS)                    # the host twin
    same(xh, rh)
    same(*_solve(A, b, rtol=rtol, max_iters=MAX_ITERS, shift=1))             # arrays off the 16-byte grid: the same packets, the same order
    A.close()


def test_diagonal_preconditioner():
    dtype, rtol = np.float64, 1e-10
    for name in MATRICES:
        n, rp, ci = _pattern(name)
        s = 10.0 ** (2 * np.random.default_rng(20261016).random(n))
        _, _, rp2, ci2, va = synth.spd_from_pattern(n, rp, ci, dscale=s, dtype=dtype)
        A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va)
        b = synth.x_rand(n)
        minv = 1.0 / (s * s)
        x, res = _solve(A, b, minv=minv, rtol=rtol, max_iters=MAX_ITERS)
        _check_converged(f"S A S/{name} with Jacobi", dtype, rp2, ci2, va, b, x, res, rtol, 19)
        x2, r2 = _solve(A, b, minv=minv, rtol=rtol, max_iters=MAX_ITERS, check_every=1, shift=1)
        assert _bits_equal(x2, x) and r2.iterations == res.iterations and r2.residual_norm == res.residual_norm
        # without it the same call runs out of steps (the CPU recurrence needs more than 1 000)
        x3, r3 = _solve(A, b, rtol=rtol, max_iters=19)
        print(f"S A S/{name} without: {r3.iterations} steps, residual / (rtol |b|) = {r3.residual_norm / (rtol * r3.b_norm):.3g}")
        assert r3.status == capi.CG_MAX_ITERS and r3.iterations == 19
        assert r3.residual_norm > rtol * r3.b_norm
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _spd("rmat", dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    b = synth.x_rand(n).astype(dtype)
    x0 = (np.random.default_rng(5).random(n) * 2 - 1).astype(dtype)
    # max_iters = 0: the initial residual alone
    x, res = _solve(A, b, x0=x0, rtol=rtol, max_iters=0)
    assert _bits_equal(x, x0) and res.iterations == 0 and res.status == capi.CG_MAX_ITERS and res.spmv_count == 1
    y, _ = O.csr_spmv64(rp, ci, va, x0)
    r0 = np.linalg.norm(b.astype(np.float64) - y)
    assert abs(res.residual_norm - r0) <= (1e-12 if dtype == np.float64 else 1e-5) * r0          # (r = b - A x0 is formed in the handle's type)
    # b = 0: x = 0 whatever the start
    x, res = _solve(A, np.zeros(n, dtype=dtype), x0=x0, rtol=rtol, max_iters=MAX_ITERS)
    assert not x.any() and res.iterations == 0 and res.status == capi.CG_CONVERGED and res.residual_norm == 0 and res.b_norm == 0
    # a start vector that solves the system already
    xs, res = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED
    x, res = _solve(A, b, x0=xs, rtol=1e-6 if dtype == np.float64 else 1e-3, max_iters=MAX_ITERS)
    assert _bits_equal(x, xs) and res.iterations == 0 and res.status == capi.CG_CONVERGED
    # a non-zero start vector: the same solution
    x, res = _solve(A, b, x0=x0, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED and res.iterations > 0
    assert _true_residual(rp, ci, va, x, b) <= 2 * rtol
    # max_iters reached: x is the last iterate, residual_norm its residual
    x, res = _solve(A, b, rtol=rtol, max_iters=2)
    assert res.status == capi.CG_MAX_ITERS and res.iterations == 2 and res.spmv_count == 3
    true = _true_residual(rp, ci, va, x, b) * res.b_norm
    assert abs(res.residual_norm - true) <= 1e-3 * true and res.residual_norm > rtol * res.b_norm
    A.close()
    # -A: p . A p < 0 at the first step
    N = cvr_amd.CvrMatrix(n, n, rp, ci, -va)
    x, res = _solve(N, b, x0=x0, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_BREAKDOWN and res.iterations == 0 and _bits_equal(x, x0)
    N.close()


def test_errors_with_a_real_handle():
    n, rp, ci = _pattern("rmat")
    va = np.ones(len(ci))
    R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)          # rectangular
    with pytest.raises(capi.CvrError) as e:
        _solve(R, np.ones(n), rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
    with pytest.raises(capi.CvrError) as e:
        R.cg_host(np.ones(n), rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID
    R.close()
    # before cvr_preprocess
    L = capi.lib()
    nrows, ncols, crp, cci, cva = K.cases()["uniform_2000"]
    view = capi.CsrView(nrows, ncols, crp.ctypes.data, cci.ctypes.data, cva.ctypes.data, 0)
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    bt = torch.ones(nrows, dtype=torch.float64, device="cuda")
    xt = torch.zeros(nrows, dtype=torch.float64, device="cuda")
    opt, res = capi.CgOptions(), capi.CgResult()
    L.cvr_cg_default_options(C.byref(opt))
    assert L.cvr_cg_device(h, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hb = np.ones(nrows)
    assert L.cvr_cg(h, hb.ctypes.data, hb.ctypes.data, C.byref(opt), C.byref(res)) == capi.ERR_STATE
    assert L.cvr_destroy(h) == 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_neighbours(prec, tmp_path):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _spd("web", dtype)
    b = synth.x_rand(n).astype(dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, steps_per_chunk=16)
    # no state left behind: a plain SpMV gives the same bits before and after
    xt = torch.zeros(A.info.x_elems, dtype=_tdt(A), device="cuda")
    xt[:n] = torch.from_numpy(b)

    def plain():
        yt = torch.full((A.info.yext_elems,), float("nan"), dtype=_tdt(A), device="cuda")
        torch.cuda.synchronize()
        A.spmv_device(xt.data_ptr(), yt.data_ptr())
        torch.cuda.synchronize()
        return yt[:n].cpu().numpy()
    before = plain()
    x, res = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED
    assert _bits_equal(plain(), before)
    # a torch side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    xs, rs = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS, stream=side.cuda_stream)
    assert _bits_equal(xs, x) and rs.iterations == res.iterations
    # an image-cache round trip
    path = str(tmp_path / "h.cvr")
    A.save_image(path)
    Lh = cvr_amd.CvrMatrix.from_image(path, steps_per_chunk=16)
    xl, rl = _solve(Lh, b, rtol=rtol, max_iters=MAX_ITERS)
    assert _bits_equal(xl, x) and rl.iterations == res.iterations and rl.residual_norm == res.residual_norm
    Lh.close()
    A.close()
    # a mutable handle: A, then 2 A -- half the solution (each solve's error is at most |A^-1| |r| <= 2 rtol |b| <= 3 rtol |x|; two solves, and the halves)
    M = cvr_amd.CvrMatrix(n, n, rp, ci, va, mutable_values=1)
    x1, r1 = _solve(M, b, rtol=rtol, max_iters=MAX_ITERS)
    M.update_values((2 * va).astype(dtype))
    x2, r2 = _solve(M, b, rtol=rtol, max_iters=MAX_ITERS)
    assert r1.status == r2.status == capi.CG_CONVERGED
    assert _true_residual(rp, ci, (2 * va).astype(dtype), x2, b) <= 2 * rtol
    h1, h2 = x1.astype(np.float64) / 2, x2.astype(np.float64)
    assert np.linalg.norm(h2 - h1) <= 8 * rtol * np.linalg.norm(h1)
    M.close()
    # the handle of A^T of a symmetric A solves the same system
    T = cvr_amd.CvrMatrix(n, n, rp, ci, va, transpose=1)
    xt_, rt = _solve(T, b, rtol=rtol, max_iters=MAX_ITERS)
    _check_converged("transpose", dtype, rp, ci, va, b, xt_, rt, rtol, BOUND[dtype])
    T.close()


def test_fused_one_submission_handle():
    nrows, _, prp, pci, _ = synth.web_google_like(0.5)
    n, _, rp, ci, va = synth.spd_from_pattern(nrows, prp, pci)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    b = synth.x_rand(n)
    x, res = _solve(A, b, rtol=1e-10, max_iters=MAX_ITERS)
    print("preprocess_fused", A.info.preprocess_fused, "col_phases", A.info.col_phases, "panels", A.info.col_panels)
    _check_converged("web x 0.5, default options", np.float64, rp, ci, va, b, x, res, 1e-10, 19)
    A.close()


_FULL_SIZE = r"""
import json, sys
import numpy as np
import torch
import cvr_amd
import oraclelib as O
from cvr_amd import synth
nrows, _, prp, pci, _ = synth.web_google_like()
n, _, rp, ci, va = synth.spd_from_pattern(nrows, prp, pci)
A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
b = synth.x_rand(n)
bt = torch.from_numpy(b).cuda()
xt = torch.zeros(n, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
res = A.cg(bt.data_ptr(), xt.data_ptr(), rtol=1e-10, max_iters=40)
torch.cuda.synchronize()
y, _ = O.csr_spmv64(rp, ci, va, xt.cpu().numpy())
print(json.dumps(dict(status=res.status, iterations=res.iterations, spmv_count=res.spmv_count, residual_norm=res.residual_norm, b_norm=res.b_norm,
                      seconds=res.seconds, true=float(np.linalg.norm(b - y) / np.linalg.norm(b)), np_b_norm=float(np.linalg.norm(b)),
                      col_panels=A.info.col_panels, col_phases=A.info.col_phases, nnz=int(rp[-1]))))
A.close()
"""


def test_full_size_web_google_shape():
    """the web-Google shape made SPD, default options (the rules pick the layout), fp64, rtol 1e-10; in a process of its own under a time limit"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    r = subprocess.run([sys.executable, "-c", _FULL_SIZE], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["status"] == capi.CG_CONVERGED
    assert out["iterations"] <= 19
    assert out["true"] <= 2e-10
    assert out["residual_norm"] <= 1e-10 * out["b_norm"]
    assert abs(out["b_norm"] - out["np_b_norm"]) <= 1e-12 * out["np_b_norm"]
