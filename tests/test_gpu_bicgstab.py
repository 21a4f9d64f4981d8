"""GPU (MI355X): BiCGSTAB on the device -- cvr_bicgstab_device / cvr_bicgstab, all through the ABI, checked by the oracle's CSR loop in fp64.

The matrices are synth.nonsym_from_pattern over a web-Google-like pattern, a banded one and a de-duplicated R-MAT: A = I - W with every row of W
of absolute sum c = 0.5, nonsymmetric in pattern and values, its spectrum in the disc |z - 1| <= 0.5.  BiCGSTAB has no a-priori step bound, so the
step counts are held against this file's numpy twin of the recurrence in include/cvr_amd.h (fp64 sums, every stored vector rounded to the handle's
type): the device sums in another order, which can move the stop by a step, hence twin + 2.  The recurrence residual and the true one differ by
O(eps * steps * |A| |x| / |b|) -- below 1e-13 in fp64 and 1e-5 in fp32 --, so the true residual is held to 2 * rtol.

  * every layout in fp64 (rtol 1e-10) and fp32 (rtol 1e-4): converged, within the twin's count + 2, true residual, the reported norms
  * bit for bit: call after call, check_every = 1 / 3 / max_iters, the host twin, arrays that are not 16-byte aligned
  * the diagonal preconditioner on diag(s) A, and the same system without it
  * the stop states (breakdown among them), the error returns with a real handle, and the neighbours: mutable, transposed and cached handles,
    streams, no state left, cvr_cg_device on the same handle
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cases as K
import cvr_amd
import oraclelib as O
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALL_LAYOUTS = K.ALL_LAYOUTS          # (the shared layout table: tests/cases.py)

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 60
MATRICES = ("web", "banded", "rmat")


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
def _nonsym(name, dtype):
    n, rp, ci = _pattern(name)
    return synth.nonsym_from_pattern(n, rp, ci, dtype=dtype)


def _usable(v):
    return v != 0 and math.isfinite(v)


def _twin(rp, ci, va, b, x0=None, minv=None, rtol=1e-10, max_iters=MAX_ITERS):
    """the recurrence of include/cvr_amd.h in numpy: sums in fp64, every stored vector rounded to va's type once; (x, iterations, status,
    residual norm).  The SpMV is the oracle's CSR loop in fp64, rounded."""
    T = va.dtype
    n = len(rp) - 1

    def f(a):
        return a.astype(np.float64)

    def spmv(x):
        return O.csr_spmv64(rp, ci, va, x)[0].astype(T)

    def dot(a, c):
        return float(np.dot(f(a), f(c)))
    b = np.asarray(b, dtype=T)
    x = np.zeros(n, dtype=T) if x0 is None else np.array(x0, dtype=T)
    m = None if minv is None else np.asarray(minv, dtype=T)
    r = (f(b) - f(spmv(x))).astype(T)
    bb = dot(b, b)
    bnorm, rnorm = math.sqrt(bb), math.sqrt(dot(r, r))
    if bb == 0:
        return np.zeros(n, dtype=T), 0, capi.CG_CONVERGED, 0.0
    if rnorm <= rtol * bnorm and math.isfinite(rnorm):
        return x, 0, capi.CG_CONVERGED, rnorm
    rhat, p, rho = r.copy(), r.copy(), dot(r, r)
    for k in range(max_iters):
        ph = p if m is None else (f(m) * f(p)).astype(T)
        v = spmv(ph)
        rv = dot(rhat, v)
        if not _usable(rv):
            return x, k, capi.CG_BREAKDOWN, rnorm
        alpha = rho / rv
        s = (f(r) - alpha * f(v)).astype(T)
        sh = s if m is None else (f(m) * f(s)).astype(T)
        snorm = math.sqrt(dot(s, s))
        if snorm <= rtol * bnorm and math.isfinite(snorm):
            return (f(x) + alpha * f(ph)).astype(T), k + 1, capi.CG_CONVERGED, snorm
        t = spmv(sh)
        ts, tt = dot(t, s), dot(t, t)
        omega = ts / tt if tt != 0 else float("nan")
        if not _usable(tt) or not _usable(omega):
            return x, k, capi.CG_BREAKDOWN, rnorm
        x = ((f(x) + alpha * f(ph)) + omega * f(sh)).astype(T)
        r = (f(s) - omega * f(t)).astype(T)
        rnorm = math.sqrt(dot(r, r))
        if rnorm <= rtol * bnorm and math.isfinite(rnorm):
            return x, k + 1, capi.CG_CONVERGED, rnorm
        rho1 = dot(rhat, r)
        if not _usable(rho1):
            return x, k + 1, capi.CG_BREAKDOWN, rnorm
        beta = (rho1 / rho) * (alpha / omega)
        p = (f(r) + beta * (f(p) - omega * f(v))).astype(T)
        rho = rho1
    return x, max_iters, capi.CG_MAX_ITERS, rnorm


@functools.lru_cache(maxsize=None)
def _twin_steps(name, dtype):
    """the twin's step count for A x = x_rand from a zero start at the type's tolerance: computed once, shared"""
    n, _, rp, ci, va = _nonsym(name, dtype)
    b = synth.x_rand(n).astype(dtype)
    x, steps, status, _ = _twin(rp, ci, va, b, rtol=RTOL[dtype])
    assert status == capi.CG_CONVERGED and _true_residual(rp, ci, va, x, b) <= RTOL[dtype], (name, steps, status)
    return steps


def _tdt(H):
    return torch.float64 if H.dtype == np.float64 else torch.float32


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _solve(H, b, x0=None, minv=None, shift=0, stream=None, method="bicgstab", **kw):
    """cvr_bicgstab_device on torch arrays of exactly nrows values (no pad, no tail), `shift` elements off the allocation's start; (x, result)"""
    n = H.nrows

    def dev(a):
        t = torch.empty(n + shift, dtype=_tdt(H), device="cuda")[shift:]
        t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=H.dtype)))
        return t
    bt = dev(b)
    xt = dev(np.zeros(n, dtype=H.dtype) if x0 is None else x0)
    mt = None if minv is None else dev(minv)
    torch.cuda.synchronize()
    res = getattr(H, method)(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), stream=stream, **kw)
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


def _check_converged(name, dtype, rp, ci, va, b, x, res, rtol, twin_steps):
    true = _true_residual(rp, ci, va, x, b)
    print(f"{name} {np.dtype(dtype).name}: {res.iterations} steps (twin {twin_steps}), {res.spmv_count} SpMVs, residual / (rtol |b|) = "
          f"{res.residual_norm / (rtol * res.b_norm):.3f}, true / rtol = {true / rtol:.3f}, {res.seconds * 1e6:.0f} us")
    assert res.status == capi.CG_CONVERGED, (name, res.status, res.iterations)
    assert true <= 2 * rtol, (name, true)
    assert res.iterations <= twin_steps + 2, (name, res.iterations, twin_steps)
    assert res.residual_norm <= rtol * res.b_norm
    bn = float(np.linalg.norm(np.asarray(b, dtype=np.float64)))
    assert abs(res.b_norm - bn) <= 1e-12 * bn
    return true


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_every_layout_converges_within_the_twins_count(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    built = 0
    for name in MATRICES:
        n, _, rp, ci, va = _nonsym(name, dtype)
        A = _make(n, n, rp, ci, va, ALL_LAYOUTS[layout])
        if A is None:
            continue
        built += 1
        b = synth.x_rand(n).astype(dtype)
        x, res = _solve(A, b, rtol=RTOL[dtype], max_iters=MAX_ITERS)
        _check_converged(f"{layout}/{name}", dtype, rp, ci, va, b, x, res, RTOL[dtype], _twin_steps(name, dtype))
        A.close()
    assert built > 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", ["default", "panels", "hub", "gang"])
def test_bit_for_bit(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = _nonsym("web", dtype)
    A = _make(n, n, rp, ci, va, ALL_LAYOUTS[layout])
    assert A is not None, layout
    b = synth.x_rand(n).astype(dtype)
    rtol = RTOL[dtype]
    x, res = _solve(A, b, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED and 0 < res.iterations <= _twin_steps("web", dtype) + 2

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
    assert counts[0] == 2 * res.iterations + 1                               # the initial residual and two per step: nothing behind the stop
    assert counts == sorted(counts) and counts[-1] == 2 * MAX_ITERS + 1
    xh, rh = A.bicgstab_host(b, rtol=rtol, max_iters=MAX_ITERS)              # the host entry point
    same(xh, rh)
    same(*_solve(A, b, rtol=rtol, max_iters=MAX_ITERS, shift=1))             # arrays off the 16-byte grid: the same packets, the same order
    A.close()


def test_diagonal_preconditioner():
    dtype, rtol = np.float64, 1e-10
    for name in MATRICES:
        n, rp, ci = _pattern(name)
        s = 10.0 ** (2 * np.random.default_rng(20261017).random(n))
        _, _, rp2, ci2, va = synth.nonsym_from_pattern(n, rp, ci, rscale=s, dtype=dtype)
        A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va)
        b = synth.x_rand(n)
        minv = 1.0 / s
        _, steps, status, _ = _twin(rp2, ci2, va, b, minv=minv, rtol=rtol)
        assert status == capi.CG_CONVERGED
        x, res = _solve(A, b, minv=minv, rtol=rtol, max_iters=MAX_ITERS)
        _check_converged(f"diag(s) A/{name} with Jacobi", dtype, rp2, ci2, va, b, x, res, rtol, steps)
        x2, r2 = _solve(A, b, minv=minv, rtol=rtol, max_iters=MAX_ITERS, check_every=1, shift=1)
        assert _bits_equal(x2, x) and r2.iterations == res.iterations and r2.residual_norm == res.residual_norm
        # without it the same call runs out of steps, as the twin does
        _, steps0, status0, rn0 = _twin(rp2, ci2, va, b, rtol=rtol, max_iters=25)
        assert status0 == capi.CG_MAX_ITERS and steps0 == 25
        x3, r3 = _solve(A, b, rtol=rtol, max_iters=25)
        print(f"diag(s) A/{name} without: {r3.iterations} steps, residual / (rtol |b|) = {r3.residual_norm / (rtol * r3.b_norm):.3g} (twin {rn0 / (rtol * r3.b_norm):.3g})")
        assert r3.status == capi.CG_MAX_ITERS and r3.iterations == 25
        assert r3.residual_norm > rtol * r3.b_norm
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _nonsym("rmat", dtype)
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
    assert res.status == capi.CG_MAX_ITERS and res.iterations == 2 and res.spmv_count == 5
    true = _true_residual(rp, ci, va, x, b) * res.b_norm
    assert abs(res.residual_norm - true) <= 1e-3 * true and res.residual_norm > rtol * res.b_norm
    # a NaN in b: the residual norm is not finite, r^ . v of step 0 neither
    bn = b.copy()
    bn[n // 2] = np.nan
    x, res = _solve(A, bn, x0=x0, rtol=rtol, max_iters=MAX_ITERS)
    assert res.status == capi.CG_BREAKDOWN and res.iterations == 0 and _bits_equal(x, x0)
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_breakdown_on_the_cyclic_shift(prec):
    """A = the cyclic shift (row i holds a one in column i + 1 mod n), b = e_0, zero start: r^ = p = e_0 and v = A p = e_(n-1), so r^ . v is exactly 0
    at step 0"""
    dtype = np.float64 if prec == "fp64" else np.float32
    n = 2000
    rp = np.arange(n + 1, dtype=np.int64)
    ci = ((np.arange(n) + 1) % n).astype(np.int32)
    va = np.ones(n, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    b = np.zeros(n, dtype=dtype)
    b[0] = 1
    assert _twin(rp, ci, va, b, rtol=RTOL[dtype])[1:3] == (0, capi.CG_BREAKDOWN)
    for every in (0, 1):
        x, res = _solve(A, b, rtol=RTOL[dtype], max_iters=MAX_ITERS, check_every=every)
        assert res.status == capi.CG_BREAKDOWN and res.iterations == 0
        assert _bits_equal(x, np.zeros(n, dtype=dtype))
        assert res.residual_norm == 1.0 and res.b_norm == 1.0
    x0 = np.full(n, -0.0, dtype=dtype)          # (bitwise untouched: the sign of zero survives)
    x, res = _solve(A, b, x0=x0, rtol=RTOL[dtype], max_iters=MAX_ITERS)
    assert res.status == capi.CG_BREAKDOWN and res.iterations == 0 and _bits_equal(x, x0)
    A.close()


def test_errors_with_a_real_handle():
    n, rp, ci = _pattern("rmat")
    va = np.ones(len(ci))
    R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)          # rectangular
    with pytest.raises(capi.CvrError) as e:
        _solve(R, np.ones(n), rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
    with pytest.raises(capi.CvrError) as e:
        R.bicgstab_host(np.ones(n), rtol=1e-6, max_iters=3)
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
    assert L.cvr_bicgstab_device(h, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hb = np.ones(nrows)
    assert L.cvr_bicgstab(h, hb.ctypes.data, hb.ctypes.data, C.byref(opt), C.byref(res)) == capi.ERR_STATE
    assert L.cvr_destroy(h) == 0


def _transposed_csr(n, rp, ci, va):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    order = np.lexsort((rows, ci))          # by column, then by row
    trp = np.zeros(n + 1, dtype=np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
    return trp, rows[order].astype(np.int32), va[order]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_neighbours(prec, tmp_path):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _nonsym("web", dtype)
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
    # a mutable handle: A, then 2 A -- half the solution (each solve's error is at most |A^-1| |r| <= 2 rtol |b| <= 3 rtol |x|, as |A^-1| <= 1 / (1 - c) = 2
    # and |b| <= |A| |x| <= 1.5 |x|; two solves, and the halves)
    M = cvr_amd.CvrMatrix(n, n, rp, ci, va, mutable_values=1)
    x1, r1 = _solve(M, b, rtol=rtol, max_iters=MAX_ITERS)
    M.update_values((2 * va).astype(dtype))
    x2, r2 = _solve(M, b, rtol=rtol, max_iters=MAX_ITERS)
    assert r1.status == r2.status == capi.CG_CONVERGED
    assert _true_residual(rp, ci, (2 * va).astype(dtype), x2, b) <= 2 * rtol
    h1, h2 = x1.astype(np.float64) / 2, x2.astype(np.float64)
    assert np.linalg.norm(h2 - h1) <= 8 * rtol * np.linalg.norm(h1)
    M.close()
    # the handle of A^T solves A^T x = b: the true residual against the explicitly transposed CSR (columns of A^T sum to at most c in absolute value, not
    # its rows: still in the disc, another step count -- the twin's on the transposed CSR)
    trp, tci, tva = _transposed_csr(n, rp, ci, va)
    _, tsteps, tstatus, _ = _twin(trp, tci, tva, b, rtol=rtol)
    assert tstatus == capi.CG_CONVERGED
    T = cvr_amd.CvrMatrix(n, n, rp, ci, va, transpose=1)
    xt_, rt = _solve(T, b, rtol=rtol, max_iters=MAX_ITERS)
    _check_converged("transpose", dtype, trp, tci, tva, b, xt_, rt, rtol, tsteps)
    T.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_conjugate_gradients_on_the_same_handle_unchanged(prec):
    """cvr_cg_device before and after a BiCGSTAB solve on the same handle: the same bits; and BiCGSTAB solves the SPD system too"""
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, rp, ci = _pattern("rmat")
    _, _, rp2, ci2, va = synth.spd_from_pattern(n, rp, ci, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va)
    b = synth.x_rand(n).astype(dtype)
    x1, r1 = _solve(A, b, rtol=rtol, max_iters=40, method="cg")
    xb, rb = _solve(A, b, rtol=rtol, max_iters=40)
    x2, r2 = _solve(A, b, rtol=rtol, max_iters=40, method="cg")
    assert r1.status == capi.CG_CONVERGED and 0 < r1.iterations <= (19 if dtype == np.float64 else 8)          # (tests/test_gpu_cg.py's bound)
    assert _bits_equal(x1, x2) and (r1.iterations, r1.status, r1.residual_norm, r1.b_norm) == (r2.iterations, r2.status, r2.residual_norm, r2.b_norm)
    assert rb.status == capi.CG_CONVERGED and _true_residual(rp2, ci2, va, xb, b) <= 2 * rtol
    A.close()
