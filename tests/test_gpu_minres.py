"""GPU (MI355X): cvr_minres_device / cvr_minres step by step against the numpy model of include/cvr_amd.h (tests/minres_model.py;
tests/test_minres_model_host.py shows on the CPU that the model solves symmetric indefinite systems within its bounds and that the comparison used
here rejects a wrong sign, recurrence, shift, norm or stop test).

The model's product is the handle's own cvr_spmv_device, whose bits the header promises for q = A v; everything else -- the vector updates, the
fixed-tree sums, the rotations, the stop and breakdown tests -- is the model's own arithmetic.  The device is held to it byte for byte: x, iterations,
status, residual_norm, b_norm and cvr_minres_info, for max_iters = 0, 1, 2, 3 and up to the stop.

The shapes are those where the kernels can go wrong: n in {1, 2, 3, 5} (packet tails: 2 values in fp64, 4 in fp32; at n = 1 the beta' == 0 ending),
kkt(44, 22) and kkt(201, 100) (one and two workgroups' worth of packets, truly indefinite), and one long banded case per type just above one trip of
the packet loop.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import minres_model as MM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-10, np.float32: 1e-5}
MAX_ITERS = 400


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


class System:
    """one handle with the buffers of its product, and the solver calls in the model's terms"""

    def __init__(self, n, rp, ci, va, **options):
        self.n, self.dtype = n, va.dtype.type
        self.H = cvr_amd.CvrMatrix(n, n, rp, ci, va, **options)
        self.tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(self.H.info.x_elems, n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(self.H.info.yext_elems, n, 1), dtype=self.tdt, device="cuda")

    def close(self):
        self.H.close()

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def model(self):
        return MM.MinresModel(self.product, self.dtype)

    def put(self, a, off=0):
        a = np.ascontiguousarray(a, dtype=self.dtype).reshape(-1)
        t = torch.empty(a.size + off, dtype=self.tdt, device="cuda")[off:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, b, x0, minv=None, shift=0.0, offs=(0, 0, 0), **kw):
        """cvr_minres_device on arrays of exactly n values, `offs` values off the allocation's grid; (Got, MinresInfo, CgResult)"""
        bt = self.put(b, offs[0])
        xt = self.put(np.zeros(self.n) if x0 is None else x0, offs[1])
        mt = None if minv is None else self.put(minv, offs[2])
        torch.cuda.synchronize()
        res, info = self.H.minres(bt.data_ptr(), xt.data_ptr(), shift=shift, minv_ptr=None if mt is None else mt.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert bt.cpu().numpy().tobytes() == np.ascontiguousarray(b, dtype=self.dtype).tobytes(), "b was written"
        assert mt is None or mt.cpu().numpy().tobytes() == np.ascontiguousarray(minv, dtype=self.dtype).tobytes(), "minv was written"
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), info, res


def _same(got, info, entry, ctx):
    msg = MM.compare(got, info, entry)
    assert msg == "", (ctx, msg)


def _offs(dtype):
    return ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)) + (((2, 3, 1),) if dtype == np.float32 else ())


def _trajectory(S, b, x0, minv, shift, ctx, kmax=3, offs=None, full=None):
    """the bitwise tier for one system: max_iters = 0 .. kmax at rtol = 0, then the run to rtol, for every check_every and off the 16-byte grid"""
    rtol = RTOL[S.dtype]
    offs = _offs(S.dtype) if offs is None else offs
    if full is None:
        full = S.model().run(b, x0, minv, shift, rtol=rtol, max_iters=MAX_ITERS)
    assert full.last.terminal and full.last.status == KM.CONVERGED, (ctx, full.last)
    if len(full.steps) > kmax + 1:          # (entries that are not terminal do not depend on rtol)
        entries = full.steps[: kmax + 1]
    else:
        free = S.model().run(b, x0, minv, shift, rtol=0.0, max_iters=kmax)
        entries = [free.at(k) for k in range(kmax + 1)]
    for k in range(kmax + 1):
        got, info, res = S.solve(b, x0, minv, shift, rtol=0.0, max_iters=k, check_every=1)
        _same(got, info, entries[k], (ctx, "max_iters", k))
        if not entries[k].terminal:
            assert res.spmv_count == 1 + k, (ctx, k, res.spmv_count)
    for every in (3, 8):
        got, info, _ = S.solve(b, x0, minv, shift, rtol=0.0, max_iters=kmax, check_every=every)
        _same(got, info, entries[kmax], (ctx, "max_iters", kmax, "check_every", every))
    for o in offs:
        got, info, _ = S.solve(b, x0, minv, shift, offs=o, rtol=0.0, max_iters=kmax)
        _same(got, info, entries[kmax], (ctx, "max_iters", kmax, "offs", o))
    for every in (1, 3, 8):
        got, info, res = S.solve(b, x0, minv, shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
        _same(got, info, full.last, (ctx, "rtol", "check_every", every))
        if every == 1:
            assert res.spmv_count == 1 + max(res.iterations, 1), (ctx, res.spmv_count, res.iterations)
    for o in offs[:1]:
        got, info, _ = S.solve(b, x0, minv, shift, offs=o, rtol=rtol, max_iters=MAX_ITERS)          # (and a rerun: the same bits)
        _same(got, info, full.last, (ctx, "rtol", "offs", o))
    return full


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_packet_tails_against_the_model(n, prec):
    """banded("spd", n) - 2 I: negative definite"""
    dtype = _dtype(prec)
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    S = System(n, rp, ci, va)
    try:
        b, x0, minv = MM.shifted_inputs(n, dtype)
        for pre, start, shift in ((None, None, 2.0), (minv, x0, 2.0), (minv, None, 0.0)):
            _trajectory(S, b, start, pre, shift, ("tails", prec, n, pre is not None, start is not None, shift), offs=_offs(dtype)[:2])
        if n == 1:          # b = 2: beta' == 0 after step 0, which ends in the stop test although rtol = 0
            got, info, res = S.solve(b, None, None, 2.0, rtol=0.0, max_iters=5, check_every=1)
            assert (got.iterations, got.status, got.residual_norm, got.x.tolist()) == (1, KM.CONVERGED, 0.0, [-2.0])
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", [(44, 22), (201, 100)], ids=["kkt66", "kkt301"])
def test_kkt_against_the_model(shape, prec):
    dtype = _dtype(prec)
    n, _, rp, ci, va = MM.kkt(*shape, dtype)
    S = System(n, rp, ci, va)
    try:
        b, x0, minv = KM.inputs(n, dtype)
        for pre, start, shift in ((None, None, 0.0), (minv, x0, 0.0), (None, x0, 0.25), (minv, None, 0.25)):
            _trajectory(S, b, start, pre, shift, ("kkt", shape, prec, pre is not None, start is not None, shift))
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.ALL_LAYOUTS))
def test_every_layout_against_the_model(layout, prec):
    """the vector kernels are the same across layouts; info.x_elems, info.yext_elems, the scratch tail and the library's buffers are not.
    minres_model.banded_indefinite(2500): half of the spectrum on either side of 0 (tests/test_minres_model_host.py), and wide enough for the
    phase and window layouts to form"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = MM.banded_indefinite(2500, dtype)
    S = System(n, rp, ci, va, **K.ALL_LAYOUTS[layout])
    try:
        i = S.H.info
        if layout in ("phases", "phases_tags_pieces"):
            assert i.col_phases > 1, i.col_phases
        if layout in ("window", "phases", "phases_tags_pieces"):
            assert i.x_window > 0, i.x_window
        b, x0, minv = KM.inputs(n, dtype)
        for pre, start, shift in ((None, None, 0.0), (minv, x0, 0.25)):
            _trajectory(S, b, start, pre, shift, ("layout", layout, prec, shift), kmax=3, offs=_offs(dtype)[:1])
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_just_above_one_trip_of_the_packet_loop(prec):
    """banded - 2 I with minv, b, x and minv off the 16-byte grid too: the first 12 values of a second trip"""
    dtype = _dtype(prec)
    n = (524289 if dtype == np.float64 else 1048577) + 12
    assert KM.trips_of(n, KM.pack_of(dtype)) == 2 and KM.trips_of(n - 13, KM.pack_of(dtype)) == 1
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    S = System(n, rp, ci, va)
    try:
        b, x0, minv = KM.inputs(n, dtype)
        rtol = RTOL[dtype]
        full = S.model().run(b, x0, minv, 2.0, rtol=rtol, max_iters=MAX_ITERS)
        assert full.last.terminal and full.last.status == KM.CONVERGED and len(full.steps) > 4, full.last
        for k in (0, 1, 3):
            got, info, _ = S.solve(b, x0, minv, 2.0, rtol=0.0, max_iters=k, check_every=1)
            _same(got, info, full.steps[k], ("long", prec, "max_iters", k))
        for o, every in (((0, 0, 0), 0), ((1, 1, 1), 3)):
            got, info, _ = S.solve(b, x0, minv, 2.0, offs=o, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            _same(got, info, full.last, ("long", prec, "rtol", o, every))
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    """(a stop of the start is found at the first read-back, behind the one step check_every = 1 enqueues: spmv_count == 2; max_iters = 0 enqueues none)"""
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    n, _, rp, ci, va = MM.kkt(44, 22, dtype)
    S = System(n, rp, ci, va)
    try:
        b, x0, minv = KM.inputs(n, dtype)
        # b == 0: x = 0 whatever the start
        for o in ((0, 0, 0), (1, 1, 1)):
            got, info, res = S.solve(np.zeros(n), x0, minv, 0.0, offs=o, rtol=rtol, check_every=1)
            _same(got, info, S.model().run(np.zeros(n), x0, minv, 0.0, rtol=rtol).last, ("b = 0", prec, o))
            assert not got.x.any() and (got.iterations, got.status, res.spmv_count) == (0, KM.CONVERGED, 2)
        # a start vector within the tolerance: x untouched
        solved = S.model().run(b, None, None, 0.0, rtol=rtol / 16, max_iters=MAX_ITERS).last
        assert solved.status == KM.CONVERGED
        got, info, res = S.solve(b, solved.x, None, 0.0, rtol=rtol, check_every=1)
        _same(got, info, S.model().run(b, solved.x, None, 0.0, rtol=rtol).last, ("start within the tolerance", prec))
        assert (got.iterations, got.status, res.spmv_count) == (0, KM.CONVERGED, 2) and got.x.tobytes() == solved.x.tobytes()
        # a NaN in b: breakdown, x untouched (a NaN's payload is no part of the contract: no bitwise comparison here)
        bn = b.copy()
        bn[n // 2] = np.nan
        got, info, res = S.solve(bn, x0, None, 0.0, rtol=rtol, check_every=1)
        assert (got.iterations, got.status) == (0, KM.BREAKDOWN) and got.x.tobytes() == x0.tobytes(), ("NaN in b", prec, got.iterations, got.status)
        assert np.isnan(got.residual_norm) and np.isnan(got.b_norm) and info.anorm == 0 and info.acond == 0
        want = S.model().run(bn, x0, None, 0.0, rtol=rtol).last
        assert (want.iterations, want.status, want.terminal) == (0, KM.BREAKDOWN, True)
        # a negative entry in minv that makes r2.z negative: breakdown at the start, x untouched
        bad = minv.copy()
        i = int(np.argmax(np.abs(b)))
        bad[i] = -(1 + 4 * float((minv.astype(np.float64) * b.astype(np.float64) ** 2).sum()) / float(b[i]) ** 2)
        got, info, res = S.solve(b, None, bad, 0.0, rtol=rtol, check_every=1)
        want = S.model().run(b, None, bad, 0.0, rtol=rtol).last
        assert (want.iterations, want.status, want.terminal) == (0, KM.BREAKDOWN, True)
        assert (got.iterations, got.status) == (0, KM.BREAKDOWN) and not got.x.any() and np.isnan(got.residual_norm) and (info.anorm, info.acond) == (0, 0)
        # max_iters reached
        got, info, res = S.solve(b, x0, minv, 0.0, rtol=rtol, max_iters=7)
        _same(got, info, S.model().run(b, x0, minv, 0.0, rtol=rtol, max_iters=7).at(7), ("max_iters", prec))
        assert (got.iterations, got.status, res.spmv_count) == (7, KM.MAX_ITERS, 8)
    finally:
        S.close()
    # a singular consistent system: a zero row and column with b zero there
    n, rp, ci, va, b = MM.singular_kkt(44, 22, dtype)
    S = System(n, rp, ci, va)
    try:
        full = _trajectory(S, b, None, None, 0.0, ("singular", prec), offs=_offs(dtype)[:1])
        assert full.last.x[n - 1] == 0
    finally:
        S.close()


def test_neighbours_mutable_transposed_and_host():
    for dtype in (np.float64, np.float32):
        rtol = RTOL[dtype]
        n, _, rp, ci, va = MM.kkt(201, 100, dtype)
        b, x0, minv = KM.inputs(n, dtype)
        # a mutable handle: A, then 2 A with a shift -- each solve is the model's on the handle as it is then
        S = System(n, rp, ci, va, mutable_values=1)
        try:
            got, info, _ = S.solve(b, x0, minv, 0.0, rtol=rtol, max_iters=MAX_ITERS)
            _same(got, info, S.model().run(b, x0, minv, 0.0, rtol=rtol, max_iters=MAX_ITERS).last, ("mutable", dtype))
            S.H.update_values((2 * va).astype(dtype))
            got2, info2, _ = S.solve(b, x0, minv, 0.5, rtol=rtol, max_iters=MAX_ITERS)
            _same(got2, info2, S.model().run(b, x0, minv, 0.5, rtol=rtol, max_iters=MAX_ITERS).last, ("mutable, updated", dtype))
            assert got2.status == KM.CONVERGED and got2.x.tobytes() != got.x.tobytes()
        finally:
            S.close()
        # a transpose = 1 handle of the same symmetric matrix
        S = System(n, rp, ci, va, transpose=1)
        try:
            got, info, _ = S.solve(b, None, None, 0.0, rtol=rtol, max_iters=MAX_ITERS)
            _same(got, info, S.model().run(b, None, None, 0.0, rtol=rtol, max_iters=MAX_ITERS).last, ("transposed", dtype))
            assert got.status == KM.CONVERGED
        finally:
            S.close()
        # the host entry point, and the device one without the info
        S = System(n, rp, ci, va)
        try:
            for start in (None, x0):
                got, info, res = S.solve(b, start, None, 0.25, rtol=rtol, max_iters=MAX_ITERS)
                x, hres, hinfo = S.H.minres_host(b, start, shift=0.25, rtol=rtol, max_iters=MAX_ITERS)
                assert x.shape == (n,) and x.tobytes() == got.x.tobytes()
                assert (hres.iterations, hres.status, hres.residual_norm, hres.b_norm, hres.spmv_count) == (res.iterations, res.status, res.residual_norm, res.b_norm, res.spmv_count)
                assert (hinfo.anorm, hinfo.acond) == (info.anorm, info.acond)
                opt, r2 = S.H._cg_options(rtol, MAX_ITERS, 0, None), capi.CgResult()
                bt, xt = S.put(b), S.put(np.zeros(n) if start is None else start)
                torch.cuda.synchronize()
                assert capi.lib().cvr_minres_device(S.H._h, bt.data_ptr(), xt.data_ptr(), 0.25, C.byref(opt), C.byref(r2), None, None) == 0
                assert xt.cpu().numpy().tobytes() == got.x.tobytes() and r2.iterations == res.iterations
        finally:
            S.close()


def test_minres_converges_where_conjugate_gradients_do_not():
    """kkt(201, 100): cvr_cg_device breaks down or runs out of steps; cvr_minres_device converges, and the true residual is inside
    rtol b_norm + minres_model.residual_gap (tests/test_minres_model_host.py)"""
    for dtype in (np.float64, np.float32):
        rtol = RTOL[dtype]
        n, _, rp, ci, va = MM.kkt(201, 100, dtype)
        b, _, _ = KM.inputs(n, dtype)
        S = System(n, rp, ci, va)
        try:
            bt, xt = S.put(b), S.put(np.zeros(n))
            torch.cuda.synchronize()
            cg = S.H.cg(bt.data_ptr(), xt.data_ptr(), rtol=rtol, max_iters=MAX_ITERS)
            assert cg.status in (KM.BREAKDOWN, KM.MAX_ITERS), cg.status
            got, info, res = S.solve(b, None, None, 0.0, rtol=rtol, max_iters=MAX_ITERS)
            assert got.status == KM.CONVERGED and got.iterations <= MM.KKT_STEPS[(200, 100, "fp64" if dtype == np.float64 else "fp32", False)] + 2
            A = MM.dense_of(n, rp, ci, va)
            true = float(np.linalg.norm(b.astype(np.float64) - A @ got.x.astype(np.float64)))
            bound = rtol * float(got.b_norm) + MM.residual_gap(dtype, 2.10, got.x, b)
            print(f"kkt(201, 100) {np.dtype(dtype).name}: CG status {cg.status} after {cg.iterations}, MINRES {got.iterations} steps, true residual {true:.3g}, bound {bound:.3g}")
            assert true <= bound, (true, bound)
            # (alfa and every later beta are at most ||A||_2 <= 2.10; oldb of step 1 is the start's beta = ||b||)
            assert 1 <= info.acond < 10 and 1 < info.anorm < np.sqrt(3 * 2.10 ** 2 * got.iterations + float(got.b_norm) ** 2)
        finally:
            S.close()


def test_errors_with_a_real_handle():
    dtype = np.float64
    n, _, rp, ci, va = MM.kkt(44, 22, dtype)
    L = capi.lib()
    opt, res = capi.CgOptions(), capi.CgResult()
    L.cvr_cg_default_options(C.byref(opt))
    bt = torch.ones(n + 8, dtype=torch.float64, device="cuda")
    xt = torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    # before cvr_preprocess
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    assert L.cvr_minres_device(h, bt.data_ptr(), xt.data_ptr(), 0.0, C.byref(opt), C.byref(res), None, None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hb, hx = np.ones(n), np.zeros(n)
    assert L.cvr_minres(h, hb.ctypes.data, hx.ctypes.data, 0.0, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    L.cvr_destroy(h)
    # a matrix that is not square
    R = cvr_amd.CvrMatrix(n - 1, n, rp[:n], ci[: rp[n - 1]], va[: rp[n - 1]])
    try:
        with pytest.raises(capi.CvrError) as e:
            R.minres(bt.data_ptr(), xt.data_ptr())
        assert e.value.code == capi.ERR_INVALID and "square" in cvr_amd.last_error()
    finally:
        R.close()
    assert not xt.cpu().numpy().any()
