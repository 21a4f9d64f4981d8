"""GPU (MI355X): cvr_lsqr_device / cvr_lsqr step by step against the numpy model of include/cvr_amd.h (tests/lsqr_model.py;
tests/test_lsqr_model_host.py shows on the CPU that the model solves least-squares problems within derived bounds and that the comparison used here
rejects a wrong recurrence, sign, norm estimate or stop test).

The model's two products are the two handles' own cvr_spmv_device, whose bits the header promises for q = A v and p = A^T u^; everything else -- the
vector updates, the fixed-tree sums, the rotations, the norm estimates, the stop and breakdown tests -- is the model's own arithmetic.  The device is
held to it byte for byte: x, iterations, status, residual_norm, b_norm and cvr_lsqr_info, for max_iters = 0, 1, 2, 3 and up to the stop.

The shapes are those where the kernels can go wrong: m, n in {1, 2, 3, 5} (packet tails: 2 values in fp64, 4 in fp32), 301 x 67 and 67 x 301 (m and
n in different numbers of workgroups), the golden rect64x300_int (rank 43 of 64), a square symmetric matrix with at == a, and one long case
(600 001 x 70 001: two trips of the packet loop over m, one over n).  Nothing here reads the reference tree."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import lsqr_model as LM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = {np.float64: 1e-10, np.float32: 1e-5}
MAX_ITERS = 400


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _golden_rect(dtype):
    m = capi.load_mm(os.path.join(ROOT, "tests", "golden", "mtx", "rect64x300_int.mtx"), capi.MM_STRICT)
    return m["nrows"], m["ncols"], m["row_ptr"].astype(np.int64), m["col_idx"].astype(np.int32), m["vals"].astype(dtype)


class Side:
    """one handle with the buffers of its product"""

    def __init__(self, H):
        self.H = H
        self.tdt = torch.float64 if H.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(H.info.x_elems, H.ncols + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, H.nrows, 1), dtype=self.tdt, device="cuda")

    def product(self, p):
        self.xbuf[: self.H.ncols].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.H.nrows].cpu().numpy()


class Pair:
    """the handles of A and A^T and the solver calls in the model's terms"""

    def __init__(self, m, n, rp, ci, va, symmetric=False, explicit=False, opts_a=None, opts_at=None):
        """opts_a / opts_at: cvr_options by name for the handle of A / of A^T (None: the defaults)"""
        self.m, self.n, self.dtype = m, n, va.dtype.type
        self.A = cvr_amd.CvrMatrix(m, n, rp, ci, va, **(opts_a or {}))
        if symmetric:
            self.AT = self.A
        elif explicit:
            self.AT = cvr_amd.CvrMatrix(*LM.transpose_csr(m, n, rp, ci, va), **(opts_at or {}))
        else:
            self.AT = cvr_amd.CvrMatrix(m, n, rp, ci, va, transpose=1, **(opts_at or {}))
        assert (self.AT.nrows, self.AT.ncols) == (n, m)
        self.a, self.at = Side(self.A), (Side(self.AT) if self.AT is not self.A else None)
        if self.at is None:
            self.at = self.a
        self.tdt = self.a.tdt

    def close(self):
        if self.AT is not self.A:
            self.AT.close()
        self.A.close()

    def model(self):
        return LM.LsqrModel(self.a.product, self.at.product, self.dtype)

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a, dtype=self.dtype).reshape(-1)
        t = torch.empty(a.size + shift, dtype=self.tdt, device="cuda")[shift:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, b, x0, damp=0.0, shifts=(0, 0), **kw):
        """cvr_lsqr_device on arrays of exactly m and n values; (Got, LsqrInfo, CgResult)"""
        bt = self.put(b, shifts[0])
        xt = self.put(np.zeros(self.n) if x0 is None else x0, shifts[1])
        torch.cuda.synchronize()
        res, info = self.A.lsqr(self.AT, bt.data_ptr(), xt.data_ptr(), damp=damp, **kw)
        torch.cuda.synchronize()
        assert bt.cpu().numpy().tobytes() == np.ascontiguousarray(b, dtype=self.dtype).tobytes(), "b was written"
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), info, res


def _same(got, info, entry, ctx):
    msg = LM.compare(got, info, entry)
    assert msg == "", (ctx, msg)


def _trajectory(pair, b, x0, damp, ctx, kmax=3, shifts=((1, 1), (1, 0), (0, 1)), full=None):
    """the bitwise tier for one system: max_iters = 0 .. kmax at rtol = 0, then the run to rtol, for every check_every and off the 16-byte grid"""
    rtol = RTOL[pair.dtype]
    if full is None:
        full = pair.model().run(b, x0, damp, rtol=rtol, max_iters=MAX_ITERS)
    assert full.last.terminal and full.last.status == KM.CONVERGED, (ctx, full.last)
    if len(full.steps) > kmax + 1:          # (entries that are not terminal do not depend on rtol)
        entries = full.steps[: kmax + 1]
    else:
        free = pair.model().run(b, x0, damp, rtol=0.0, max_iters=kmax)
        entries = [free.at(k) for k in range(kmax + 1)]
    for k in range(kmax + 1):
        got, info, res = pair.solve(b, x0, damp, rtol=0.0, max_iters=k, check_every=1)
        _same(got, info, entries[k], (ctx, "max_iters", k))
        if not entries[k].terminal:
            assert res.spmv_count == 2 + 2 * k, (ctx, k, res.spmv_count)
    for every in (3, 8):
        got, info, _ = pair.solve(b, x0, damp, rtol=0.0, max_iters=kmax, check_every=every)
        _same(got, info, entries[kmax], (ctx, "max_iters", kmax, "check_every", every))
    for sh in shifts:
        got, info, _ = pair.solve(b, x0, damp, shifts=sh, rtol=0.0, max_iters=kmax)
        _same(got, info, entries[kmax], (ctx, "max_iters", kmax, "shifts", sh))
    for every in (1, 3, 8):
        got, info, res = pair.solve(b, x0, damp, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
        _same(got, info, full.last, (ctx, "rtol", "check_every", every))
        if every == 1:
            assert res.spmv_count == 2 + 2 * res.iterations, (ctx, res.spmv_count, res.iterations)
    for sh in shifts[:1]:
        got, info, _ = pair.solve(b, x0, damp, shifts=sh, rtol=rtol, max_iters=MAX_ITERS)          # (and a rerun: the same bits)
        _same(got, info, full.last, (ctx, "rtol", "shifts", sh))
    return full


def _shifts(dtype):
    return ((1, 1), (1, 0), (0, 1)) + (((2, 3),) if dtype == np.float32 else ())


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_packet_tails_against_the_model(m, prec):
    dtype = _dtype(prec)
    for n in (1, 2, 3, 5):
        pair = Pair(*LM.rect_sparse(m, n, dtype))
        try:
            rp, ci, va = LM.rect_sparse(m, n, dtype)[2:]
            b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
            for damp, start in ((0.0, None), (0.3, x0)):
                _trajectory(pair, b, start, damp, ("tails", prec, m, n, damp), shifts=_shifts(dtype)[:2])
        finally:
            pair.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["301x67", "67x301", "rect64x300_int"])
def test_rectangular_against_the_model(name, prec):
    dtype = _dtype(prec)
    m, n, rp, ci, va = _golden_rect(dtype) if name == "rect64x300_int" else LM.rect_sparse(*(int(s) for s in name.split("x")), dtype)
    pair = Pair(m, n, rp, ci, va)
    try:
        for consistent, damp, zero_start in ((False, 0.0, True), (True, 0.0, False), (False, 0.5, False)):
            b, x0 = LM.inputs(m, n, rp, ci, va, dtype, consistent)
            _trajectory(pair, b, None if zero_start else x0, damp, (name, prec, consistent, damp), shifts=_shifts(dtype))
    finally:
        pair.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_square_symmetric_with_one_handle(prec):
    """at == a: both products on the one handle, u^ in the one buffer that is its output and its input"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = KM.banded("spd", 129, dtype)
    pair = Pair(n, n, rp, ci, va, symmetric=True)
    try:
        b, x0, _ = KM.inputs(n, dtype)
        for damp, start in ((0.0, x0), (0.25, None)):
            _trajectory(pair, b, start, damp, ("symmetric", prec, damp), shifts=_shifts(dtype)[:1])
    finally:
        pair.close()


MIXED_PAIRS = {"plain+panels": ("plain", "panels"), "gang+phases": ("gang", "phases"), "hub_reorder+default": ("hub_reorder", "default"),
               "interleaved_panels+window": ("interleaved_panels", "window")}


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.ALL_LAYOUTS) + sorted(MIXED_PAIRS))
def test_layouts_against_the_model(layout, prec):
    """every layout on both handles, and four mixed pairs: u^ is A's y_ext and A^T's x_ext at once, and info.yext_elems / info.x_elems of the two
    handles differ with the layout (scratch rows of cut rows, panels, the pad element).  lsqr_model.rect_long: 701 x 449, well conditioned, rows
    and columns cut over chunks (tests/test_lsqr_model_host.py).  A layout that cannot be built for this matrix is a failure."""
    dtype = _dtype(prec)
    la, lat = MIXED_PAIRS.get(layout, (layout, layout))
    m, n, rp, ci, va = LM.rect_long(dtype)
    pair = Pair(m, n, rp, ci, va, opts_a=K.ALL_LAYOUTS[la], opts_at=K.ALL_LAYOUTS[lat])
    try:
        ia, iat = pair.A.info, pair.AT.info
        if layout == "plain":
            assert ia.nshared > 0 and iat.nshared > 0, (ia.nshared, iat.nshared)
        for name, i in ((la, ia), (lat, iat)):          # the layout really formed
            want = dict(phases=i.col_phases > 1, window=i.x_window > 0, panels=i.col_panels == 3, interleaved_panels=i.col_panels == 8 and i.interleave == 1, gang=i.gang > 0,
                        interleaved=i.interleave == 1).get(name, True)
            assert want, (name, i.col_phases, i.x_window, i.col_panels, i.interleave, i.gang)
        b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
        _trajectory(pair, b, x0, 0.5, (layout, prec), kmax=2, shifts=((1, 1),))
    finally:
        pair.close()


def test_two_trips_over_m():
    """fp64, 600 001 x 70 001, two entries per row: the longest-serving thread goes twice round the packet loop over m and once over n; b and x off
    the 16-byte grid too"""
    dtype, m, n = np.float64, 600001, 70001
    assert KM.trips_of(m, 2) == 2 and KM.trips_of(n, 2) == 1
    _, _, rp, ci, va = LM.two_per_row(m, n, dtype)
    pair = Pair(m, n, rp, ci, va)
    try:
        b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
        rtol = RTOL[dtype]
        full = pair.model().run(b, x0, 0.125, rtol=rtol, max_iters=MAX_ITERS)
        assert full.last.terminal and full.last.status == KM.CONVERGED and len(full.steps) > 4, full.last
        for k in (0, 1, 3):
            got, info, _ = pair.solve(b, x0, 0.125, rtol=0.0, max_iters=k, check_every=1)
            _same(got, info, full.steps[k], ("long", "max_iters", k))
        for sh, every in (((0, 0), 0), ((1, 1), 3)):
            got, info, res = pair.solve(b, x0, 0.125, shifts=sh, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            _same(got, info, full.last, ("long", "rtol", sh, every))
    finally:
        pair.close()


def test_transpose_option_equals_an_explicitly_transposed_csr():
    for dtype in (np.float64, np.float32):
        m, n, rp, ci, va = LM.rect_sparse(301, 67, dtype)
        b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
        out = []
        for explicit in (False, True):
            pair = Pair(m, n, rp, ci, va, explicit=explicit)
            try:
                got, info, res = pair.solve(b, x0, 0.5, rtol=RTOL[dtype], max_iters=MAX_ITERS)
                out.append((got.x.tobytes(), got.iterations, got.status, KM._bits(got.residual_norm), KM._bits(got.b_norm), KM._bits(info.arnorm), KM._bits(info.anorm),
                            info.stop_test))
                assert got.status == KM.CONVERGED
            finally:
                pair.close()
        assert out[0] == out[1]


def test_host_form_equals_device_form():
    for dtype in (np.float64, np.float32):
        for shape in ((301, 67), (67, 301)):
            m, n, rp, ci, va = LM.rect_sparse(*shape, dtype)
            b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
            pair = Pair(m, n, rp, ci, va)
            try:
                for start in (None, x0):
                    got, info, res = pair.solve(b, start, 0.5, rtol=RTOL[dtype], max_iters=MAX_ITERS)
                    x, hres, hinfo = pair.A.lsqr_host(pair.AT, b, start, damp=0.5, rtol=RTOL[dtype], max_iters=MAX_ITERS)
                    assert x.shape == (n,) and x.tobytes() == got.x.tobytes()
                    assert (hres.iterations, hres.status, hres.residual_norm, hres.b_norm, hres.spmv_count) == (res.iterations, res.status, res.residual_norm, res.b_norm, res.spmv_count)
                    assert (hinfo.arnorm, hinfo.anorm, hinfo.stop_test) == (info.arnorm, info.anorm, info.stop_test)
                    # and without the info
                    L = capi.lib()
                    opt, r2 = pair.A._cg_options(RTOL[dtype], MAX_ITERS, 0, None), capi.CgResult()
                    bt, xt = pair.put(b), pair.put(np.zeros(n) if start is None else start)
                    torch.cuda.synchronize()
                    assert L.cvr_lsqr_device(pair.A._h, pair.AT._h, bt.data_ptr(), xt.data_ptr(), 0.5, C.byref(opt), C.byref(r2), None, None) == 0
                    assert xt.cpu().numpy().tobytes() == got.x.tobytes() and r2.iterations == res.iterations
            finally:
                pair.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stops_of_the_start(prec):
    """(a stop of the start is found at the first read-back, behind the one step check_every = 1 enqueues: spmv_count == 4; max_iters = 0 enqueues none)"""
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    m, n, rp, ci, va = LM.rect_sparse(301, 67, dtype)
    pair = Pair(m, n, rp, ci, va)
    try:
        b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
        # b == 0: x = 0 whatever the start
        for sh in ((0, 0), (1, 1)):
            got, info, res = pair.solve(np.zeros(m), x0, 0.5, shifts=sh, rtol=rtol, check_every=1)
            want = pair.model().run(np.zeros(m), x0, 0.5, rtol=rtol).last
            _same(got, info, want, ("b = 0", prec, sh))
            assert not got.x.any() and (got.iterations, got.status, info.stop_test, res.spmv_count) == (0, KM.CONVERGED, 0, 4)
        # a start that satisfies test 1 already: x untouched
        bc, _ = LM.inputs(m, n, rp, ci, va, dtype, True)
        solved = pair.model().run(bc, None, 0.0, rtol=rtol / 16, max_iters=MAX_ITERS).last
        assert solved.status == KM.CONVERGED and solved.scalars["info"].stop_test == 1
        got, info, res = pair.solve(bc, solved.x, 0.0, rtol=rtol, check_every=1)
        _same(got, info, pair.model().run(bc, solved.x, 0.0, rtol=rtol).last, ("start within the tolerance", prec))
        assert (got.iterations, got.status, info.stop_test, res.spmv_count) == (0, KM.CONVERGED, 1, 4) and got.x.tobytes() == solved.x.tobytes()
        # NaN in b: breakdown, x untouched
        bn = b.copy()
        bn[m // 2] = np.nan
        got, info, res = pair.solve(bn, x0, 0.0, rtol=rtol, check_every=1)
        assert (got.iterations, got.status, info.stop_test) == (0, KM.BREAKDOWN, 0) and got.x.tobytes() == x0.tobytes(), ("NaN in b", prec, got.iterations, got.status)
        assert np.isnan(got.residual_norm) and np.isnan(got.b_norm) and info.arnorm == 0 and info.anorm == 0 and res.spmv_count == 4
        want = pair.model().run(bn, x0, 0.0, rtol=rtol).last          # (a NaN's payload is no part of the contract: no bitwise comparison here)
        assert (want.iterations, want.status, want.terminal) == (0, KM.BREAKDOWN, True)
    finally:
        pair.close()
    # A^T r0 == 0: the first two rows of A empty, b there alone: alpha == 0, test 2 at the start, x untouched
    rp2 = np.concatenate([[0, 0], rp[2:] - rp[2]]).astype(np.int64)
    pair = Pair(m, n, rp2, ci[rp[2]:], va[rp[2]:])
    try:
        e = np.zeros(m, dtype=dtype)
        e[0], e[1] = 3.0, -4.0
        got, info, res = pair.solve(e, None, 0.0, rtol=rtol, check_every=1)
        _same(got, info, pair.model().run(e, None, 0.0, rtol=rtol).last, ("A^T r0 = 0", prec))
        assert (got.iterations, got.status, info.stop_test, got.residual_norm, res.spmv_count) == (0, KM.CONVERGED, 2, 5.0, 4) and not got.x.any()
    finally:
        pair.close()


def test_handle_pair_errors():
    m, n, rp, ci, va = LM.rect_sparse(301, 67, np.float64)
    pair = Pair(m, n, rp, ci, va)
    A32 = cvr_amd.CvrMatrix(m, n, rp, ci, va.astype(np.float32), transpose=1)
    try:
        bt, xt = pair.put(np.ones(m)), pair.put(np.zeros(n))
        big = pair.put(np.zeros(m + n))
        torch.cuda.synchronize()
        # swapped handles of a non-square pair; A beside itself
        for a, at in ((pair.AT, pair.AT), (pair.A, pair.A)):
            with pytest.raises(capi.CvrError) as e:
                a.lsqr(at, big.data_ptr(), big.data_ptr())
            assert e.value.code == capi.ERR_INVALID
        # mixed value types
        with pytest.raises(capi.CvrError) as e:
            pair.A.lsqr(A32, bt.data_ptr(), xt.data_ptr())
        assert e.value.code == capi.ERR_INVALID and "type" in cvr_amd.last_error()
        # either handle before cvr_preprocess
        L = capi.lib()
        view = capi.CsrView(m, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        assert L.cvr_lsqr_device(h, pair.AT._h, bt.data_ptr(), xt.data_ptr(), 0.0, C.byref(opt), C.byref(res), None, None) == capi.ERR_STATE
        assert "cvr_preprocess" in cvr_amd.last_error()
        hb, hx = np.ones(m), np.zeros(n)
        assert L.cvr_lsqr(h, pair.AT._h, hb.ctypes.data, hx.ctypes.data, 0.0, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
        L.cvr_destroy(h)
        assert xt.cpu().numpy().tobytes() == np.zeros(n).tobytes()
    finally:
        A32.close()
        pair.close()
