"""GPU (MI355X): restarted GMRES on the device -- cvr_gmres_device / cvr_gmres through CvrMatrix.gmres / gmres_host.

  * bit for bit against the numpy model of include/cvr_amd.h (tests/gmres_model.py; tests/test_gmres_host.py shows on the CPU that the comparison
    used here rejects a wrong pass count, rotation, substitution order or restart): x byte for byte, iterations, status, residual_norm and b_norm
    equal as bits.  The model's product is the handle's own cvr_spmv_device; everything else is the model's arithmetic.  The sizes are those where
    the packet loop changes shape (a partial packet alone, one workgroup and several, more than one trip per thread), the restarts those where the
    column groups change shape (8 columns are one group, 9 cross into a second, 20 end in a partial one), and max_iters runs through a cycle, its
    end and the restart behind it.
  * convergence on every layout, with the step counts held against the model with exact sums (+ 2: the device sums in another order, which can move
    the stop by a step) and against the a-priori bound of full GMRES on A = I - W, ||r_k|| <= ||W^k|| ||r_0|| <= sqrt(n) c^k ||r_0|| per cycle.
  * the cyclic shift, where BiCGSTAB breaks down at once; the stop states; the errors with a real handle; the neighbours.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cases as K
import cvr_amd
import gmres_model as GM
import krylov_model as KM
import oraclelib as O
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
G = KM.GRID


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


class Dev:
    """a handle with the buffers of the model's product and the solver call in the model's terms"""

    def __init__(self, H):
        self.H, self.n = H, H.nrows
        self.tdt = torch.float64 if H.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(H.info.x_elems, self.n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, self.n, 1), dtype=self.tdt, device="cuda")

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a, dtype=self.H.dtype).reshape(-1)
        t = torch.empty(a.size + shift, dtype=self.tdt, device="cuda")[shift:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, b, x0, minv, m, shift=0, stream=None, **kw):
        """cvr_gmres_device on arrays of exactly nrows values, `shift` elements off the allocation's start; (Got, result)"""
        bt = self.put(b, shift)
        xt = self.put(np.zeros(self.n) if x0 is None else x0, shift)
        mt = None if minv is None else self.put(minv, shift)
        torch.cuda.synchronize()
        x, res = self.H.gmres(bt, x0=xt, restart=m, minv=mt, stream=stream, **kw)
        torch.cuda.synchronize()
        assert x is xt
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _same(got, entry, ctx):
    msg = KM.compare(got, entry)
    assert msg == "", (ctx, msg)


def _restarts_enqueued(steps, m):
    """a restart sits in front of the first step of every later cycle"""
    return (steps - 1) // m if steps > 0 else 0


# ---- against the model ----
@pytest.mark.parametrize("m", [1, 3, 8, 9, 20])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_every_max_iters_against_the_model(prec, m):
    dtype, n = _dtype(prec), 1000
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, x0, minv = KM.inputs(n, dtype)
        kmax = 2 * m + 1
        for name, start, pre in (("plain/zero", None, None), ("minv/random", x0, minv), ("plain/random", x0, None), ("minv/zero", None, minv)):
            free = GM.GmresModel(dev.product, dtype, restart=m).run(b, start, pre, rtol=0.0, max_iters=kmax)
            assert len(free.steps) > m + 1, (name, free.last)          # (behind a restart; at rtol = 0 only an estimate of exactly 0 ends a run)
            for k in range(kmax + 1):
                got, res = dev.solve(b, start, pre, m, rtol=0.0, max_iters=k, check_every=(1, 0, 3)[k % 3])
                _same(got, free.at(k), (prec, m, name, "max_iters", k))
                if k % 3 == 0 and k < len(free.steps):
                    assert res.spmv_count == 1 + k + _restarts_enqueued(k, m), (name, k, res.spmv_count)
    finally:
        A.close()


@pytest.mark.parametrize("n", [1, 2, 3, 255, 257, 4099])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_sizes_against_the_model(prec, n):
    dtype, m = _dtype(prec), 3
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, x0, minv = KM.inputs(n, dtype)
        for name, start, pre in (("plain/zero", None, None), ("minv/random", x0, minv)):
            free = GM.GmresModel(dev.product, dtype, restart=m).run(b, start, pre, rtol=0.0, max_iters=7)
            for k in (0, 1, 3, 4, 7):          # (n = 1, 2, 3: the Krylov space is exhausted on the way -- the lucky breakdown, or rho = 0 -- and the entry is terminal)
                got, _ = dev.solve(b, start, pre, m, rtol=0.0, max_iters=k)
                _same(got, free.at(k), (prec, n, name, "max_iters", k))
    finally:
        A.close()


@pytest.mark.parametrize("prec,n", [("fp64", 600_000), ("fp32", 1_100_000)])
def test_more_than_one_packet_trip_against_the_model(prec, n):
    dtype, m = _dtype(prec), 3
    assert n > G * KM.pack_of(dtype)
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, x0, minv = KM.inputs(n, dtype)
        free = GM.GmresModel(dev.product, dtype, restart=m).run(b, x0, minv, rtol=0.0, max_iters=4)
        got, _ = dev.solve(b, x0, minv, m, rtol=0.0, max_iters=4)
        _same(got, free.at(4), (prec, n))
    finally:
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_same_bits_however_it_is_called(prec):
    dtype, n, m = _dtype(prec), 1000, 8
    rtol = RTOL[dtype]
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, x0, minv = KM.inputs(n, dtype)
        full = GM.GmresModel(dev.product, dtype, restart=m).run(b, x0, minv, rtol=rtol, max_iters=60)
        assert full.last.terminal and full.last.status == KM.CONVERGED and full.last.iterations > m, full.last
        free = GM.GmresModel(dev.product, dtype, restart=m).run(b, x0, minv, rtol=0.0, max_iters=2 * m + 1)
        for entry, kw in ((full.last, dict(rtol=rtol, max_iters=60)), (free.last, dict(rtol=0.0, max_iters=2 * m + 1))):
            counts = []
            for every in (1, 3, 0):
                got, res = dev.solve(b, x0, minv, m, check_every=every, **kw)
                _same(got, entry, (prec, "check_every", every))
                counts.append(res.spmv_count)
            assert counts[0] == 1 + entry.iterations + _restarts_enqueued(entry.iterations, m), counts          # nothing behind the stop
            assert counts[0] <= counts[1] and counts[0] <= counts[2]
            _same(dev.solve(b, x0, minv, m, shift=1, **kw)[0], entry, (prec, "one element off the 16-byte grid"))
            _same(dev.solve(b, x0, minv, m, **kw)[0], entry, (prec, "call after call"))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            _same(dev.solve(b, x0, minv, m, stream=side.cuda_stream, **kw)[0], entry, (prec, "side stream"))
            mt = dev.put(minv)
            xh, rh = A.gmres_host(b, x0=x0, restart=m, minv=mt, **kw)
            _same(KM.Got(xh, rh.iterations, rh.status, rh.residual_norm, rh.b_norm), entry, (prec, "host entry point"))
    finally:
        A.close()


# ---- convergence ----
MATRICES = ("web", "banded", "rmat")
M_CONV, C_OFF = 20, 0.5


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
    return synth.nonsym_from_pattern(n, rp, ci, c=C_OFF, dtype=dtype)


def _cap(n, rtol, m=M_CONV, c=C_OFF):
    """m * ceil(ln(rtol) / ln(sqrt(n) c^m)) + m: a cycle of full GMRES on A = I - W shrinks the residual by at least sqrt(n) c^m"""
    return m * math.ceil(math.log(rtol) / math.log(math.sqrt(n) * c ** m)) + m


def _true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, x)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _model_steps(name, dtype):
    """the model's step count with exact sums (the oracle's CSR loop rounded to T as the product) for A x = x_rand from a zero start: once, shared"""
    n, _, rp, ci, va = _nonsym(name, dtype)
    b = synth.x_rand(n).astype(dtype)
    prod = lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(dtype)
    tr = GM.GmresModel(prod, dtype, sums="exact", restart=M_CONV).run(b, rtol=RTOL[dtype], max_iters=_cap(n, RTOL[dtype]))
    assert tr.last.terminal and tr.last.status == KM.CONVERGED, (name, tr.last)
    return tr.last.iterations


def _solve(H, b, x0=None, minv=None, m=M_CONV, **kw):
    return Dev(H).solve(b, x0, minv, m, **kw)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.ALL_LAYOUTS))
def test_every_layout_converges(layout, prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    built = 0
    for name in MATRICES:
        n, _, rp, ci, va = _nonsym(name, dtype)
        try:
            A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.ALL_LAYOUTS[layout])
        except capi.CvrError:          # (a layout the options cannot build for this matrix)
            continue
        built += 1
        b = synth.x_rand(n).astype(dtype)
        cap = _cap(n, rtol)
        got, res = _solve(A, b, rtol=rtol, max_iters=cap + 10)
        true = _true_residual(rp, ci, va, got.x, b)
        steps = _model_steps(name, dtype)
        print(f"{layout}/{name} {prec}: {res.iterations} steps (model {steps}, cap {cap}), {res.spmv_count} SpMVs, residual / (rtol |b|) = "
              f"{res.residual_norm / (rtol * res.b_norm):.3f}, true / rtol = {true / rtol:.3f}, {res.seconds * 1e6:.0f} us")
        assert res.status == capi.CG_CONVERGED, (name, res.status, res.iterations)
        assert res.residual_norm <= rtol * res.b_norm
        assert true <= 2 * rtol, (name, true)
        assert res.iterations <= steps + 2, (name, res.iterations, steps)
        assert res.iterations <= cap, (name, res.iterations, cap)
        A.close()
    assert built > 0


# ---- where BiCGSTAB cannot ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_cyclic_shift_where_bicgstab_breaks_down(prec):
    """row i holds a one in column i + 1 mod n, b = e_0, zero start: BiCGSTAB finds r^ . v == 0 at step 0.  The Krylov vectors e_0, e_(n-1), ... stay
    orthogonal to b until the n-th: GMRES(n) converges at step n exactly, GMRES(n / 2) never moves"""
    dtype, n = _dtype(prec), 64
    rp = np.arange(n + 1, dtype=np.int64)
    ci = ((np.arange(n) + 1) % n).astype(np.int32)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, np.ones(n, dtype=dtype))
    try:
        dev = Dev(A)
        b = np.zeros(n, dtype=dtype)
        b[0] = 1
        bt, xt = dev.put(b), dev.put(np.zeros(n))
        rb = A.bicgstab(bt.data_ptr(), xt.data_ptr(), rtol=RTOL[dtype], max_iters=100)
        assert (rb.status, rb.iterations) == (capi.CG_BREAKDOWN, 0)
        for every in (0, 1):
            got, res = dev.solve(b, None, None, n, rtol=RTOL[dtype], max_iters=100, check_every=every)
            assert (got.status, got.iterations, got.residual_norm, got.b_norm) == (capi.CG_CONVERGED, n, 0.0, 1.0)
            want = np.zeros(n, dtype=dtype)
            want[1] = 1          # A e_1 = e_0
            assert got.x.tobytes() == want.tobytes()
            got, res = dev.solve(b, None, None, n // 2, rtol=RTOL[dtype], max_iters=100, check_every=every)
            assert (got.status, got.iterations) == (capi.CG_MAX_ITERS, 100)
            assert got.residual_norm.tobytes() == got.b_norm.tobytes() and got.b_norm == 1.0
            assert not got.x.any()
    finally:
        A.close()


# ---- stop states ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    dtype = _dtype(prec)
    rtol, n = RTOL[dtype], 4099
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, x0, _ = KM.inputs(n, dtype)
        # max_iters = 0: the start only
        got, res = dev.solve(b, x0, None, 5, rtol=rtol, max_iters=0)
        assert got.x.tobytes() == x0.tobytes() and (got.iterations, got.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1)
        y, _ = O.csr_spmv64(rp, ci, va, x0)
        r0 = np.linalg.norm(b.astype(np.float64) - y)
        assert abs(got.residual_norm - r0) <= (1e-12 if dtype == np.float64 else 1e-5) * r0          # (r = b - A x0 is formed in the handle's type)
        # b = 0: x = 0 whatever the start
        got, res = dev.solve(np.zeros(n), x0, None, 5, rtol=rtol, max_iters=30)
        assert not got.x.any() and (got.iterations, got.status, got.residual_norm, got.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        # a start vector within the tolerance: x untouched
        sol, res = dev.solve(b, None, None, 5, rtol=rtol, max_iters=60)
        assert sol.status == capi.CG_CONVERGED and _true_residual(rp, ci, va, sol.x, b) <= 2 * rtol
        got, res = dev.solve(b, sol.x, None, 5, rtol=1e-6 if dtype == np.float64 else 1e-3, max_iters=60)
        assert got.x.tobytes() == sol.x.tobytes() and (got.iterations, got.status) == (0, capi.CG_CONVERGED)
        # a NaN and an Inf in b: breakdown at the start, x untouched
        for bad in (np.nan, np.inf):
            bn = b.copy()
            bn[n // 2] = bad
            for every in (0, 1):
                got, res = dev.solve(bn, x0, None, 5, rtol=rtol, max_iters=30, check_every=every)
                assert (got.status, got.iterations) == (capi.CG_BREAKDOWN, 0) and got.x.tobytes() == x0.tobytes(), (bad, every)
        # restart 1 and 64.  GMRES(1) minimises ||(I - alpha A) r|| over alpha, and alpha = 1 gives W r for A = I - W: every step shrinks the residual
        # by at least ||W||_2 <= sqrt(||W||_1 ||W||_inf) =: f (< 1 here), so ln(rtol) / ln(f) steps suffice (+ 2 for the rounding)
        rows = np.repeat(np.arange(n), np.diff(rp))
        off = np.where(rows == ci, 0.0, np.abs(va.astype(np.float64)))
        f = math.sqrt(np.bincount(ci, weights=off, minlength=n).max() * np.bincount(rows, weights=off, minlength=n).max())
        assert f < 1, f
        got, res = dev.solve(b, None, None, 1, rtol=rtol, max_iters=math.ceil(math.log(rtol) / math.log(f)) + 2)
        assert got.status == capi.CG_CONVERGED and _true_residual(rp, ci, va, got.x, b) <= 2 * rtol, (got.status, got.iterations, f)
        assert res.spmv_count >= 2 * res.iterations          # a restart in front of every step but the first
        # one cycle of GMRES(64) is full GMRES: sqrt(n) c^64 < rtol
        assert math.sqrt(n) * C_OFF ** 64 < rtol
        got, res = dev.solve(b, None, None, 64, rtol=rtol, max_iters=64)
        assert got.status == capi.CG_CONVERGED and _true_residual(rp, ci, va, got.x, b) <= 2 * rtol, (got.status, got.iterations)
        assert res.iterations <= 64
    finally:
        A.close()


# ---- errors with a real handle ----
def test_errors_with_a_real_handle():
    n, rp, ci = _pattern("rmat")
    va = np.ones(len(ci))
    R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)          # rectangular
    bt = torch.ones(n, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.CvrError) as e:
        R.gmres(bt, restart=5, rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
    with pytest.raises(capi.CvrError) as e:
        R.gmres_host(np.ones(n), restart=5, rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID
    R.close()
    # a bad restart
    _, _, rp2, ci2, va2 = KM.banded("nonsym", 100, np.float64)
    A = cvr_amd.CvrMatrix(100, 100, rp2, ci2, va2)
    bt = torch.ones(100, dtype=torch.float64, device="cuda")
    for restart in (0, -1, 65):
        with pytest.raises(capi.CvrError) as e:
            A.gmres(bt, restart=restart, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "restart" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            A.gmres_host(np.ones(100), restart=restart, max_iters=3)
        assert e.value.code == capi.ERR_INVALID
    A.close()
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
    assert L.cvr_gmres_device(h, bt.data_ptr(), xt.data_ptr(), 5, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hb = np.ones(nrows)
    assert L.cvr_gmres(h, hb.ctypes.data, hb.ctypes.data, 5, C.byref(opt), C.byref(res)) == capi.ERR_STATE
    assert L.cvr_destroy(h) == 0


# ---- neighbours ----
def _transposed_csr(n, rp, ci, va):
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    order = np.lexsort((rows, ci))          # by column, then by row
    trp = np.zeros(n + 1, dtype=np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
    return trp, rows[order].astype(np.int32), va[order]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_neighbours(prec, tmp_path):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _nonsym("web", dtype)
    b = synth.x_rand(n).astype(dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, steps_per_chunk=16)
    x, res = _solve(A, b, rtol=rtol, max_iters=100)
    assert x.status == capi.CG_CONVERGED and _true_residual(rp, ci, va, x.x, b) <= 2 * rtol
    # an image-cache round trip: the same bits
    path = str(tmp_path / "h.cvr")
    A.save_image(path)
    Lh = cvr_amd.CvrMatrix.from_image(path, steps_per_chunk=16)
    xl, _ = _solve(Lh, b, rtol=rtol, max_iters=100)
    assert KM.compare(xl, x) == ""
    Lh.close()
    A.close()
    # a mutable handle: A, then 2 A -- half the solution (tests/test_gpu_bicgstab.py's argument: each solve's error is at most 3 rtol |x|)
    M = cvr_amd.CvrMatrix(n, n, rp, ci, va, mutable_values=1)
    x1, _ = _solve(M, b, rtol=rtol, max_iters=100)
    M.update_values((2 * va).astype(dtype))
    x2, _ = _solve(M, b, rtol=rtol, max_iters=100)
    assert x1.status == x2.status == capi.CG_CONVERGED
    assert _true_residual(rp, ci, (2 * va).astype(dtype), x2.x, b) <= 2 * rtol
    h1, h2 = x1.x.astype(np.float64) / 2, x2.x.astype(np.float64)
    assert np.linalg.norm(h2 - h1) <= 8 * rtol * np.linalg.norm(h1)
    M.close()
    # the handle of A^T solves A^T x = b: the true residual against the explicitly transposed CSR
    trp, tci, tva = _transposed_csr(n, rp, ci, va)
    T = cvr_amd.CvrMatrix(n, n, rp, ci, va, transpose=1)
    xt_, _ = _solve(T, b, rtol=rtol, max_iters=200)
    assert xt_.status == capi.CG_CONVERGED and _true_residual(trp, tci, tva, xt_.x, b) <= 2 * rtol
    T.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_cg_and_bicgstab_on_the_same_handle_unchanged(prec):
    """cvr_cg_device and cvr_bicgstab_device before and after a GMRES solve on the same handle: the same bits; and GMRES solves the SPD system too"""
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    n, rp, ci = _pattern("rmat")
    _, _, rp2, ci2, va = synth.spd_from_pattern(n, rp, ci, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va)
    try:
        dev = Dev(A)
        b = synth.x_rand(n).astype(dtype)

        def other(method):
            bt, xt = dev.put(b), dev.put(np.zeros(n))
            torch.cuda.synchronize()
            r = getattr(A, method)(bt.data_ptr(), xt.data_ptr(), rtol=rtol, max_iters=40)
            torch.cuda.synchronize()
            return KM.Got(xt.cpu().numpy(), r.iterations, r.status, r.residual_norm, r.b_norm)
        before = {m: other(m) for m in ("cg", "bicgstab")}
        got, res = dev.solve(b, None, None, 20, rtol=rtol, max_iters=100)
        assert got.status == capi.CG_CONVERGED and _true_residual(rp2, ci2, va, got.x, b) <= 2 * rtol
        for m in ("cg", "bicgstab"):
            assert before[m].status == capi.CG_CONVERGED
            assert KM.compare(other(m), before[m]) == "", m
    finally:
        A.close()
