"""CPU: cvr_spgemm_host through the ABI against tests/spgemm_model.py, byte for byte -- the host twin of the device product needs no device; the
two-call shape, every error return with bad_row, and the host code under AddressSanitizer + UBSan (a stand-alone program: make spgemm-asan-check)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spgemm_model as SM
from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_spgemm_create", "cvr_spgemm_get_info", "cvr_spgemm_csr_device", "cvr_spgemm_export", "cvr_spgemm_numeric_device", "cvr_spgemm_destroy", "cvr_spgemm_host"]
HOST_CASES = SM.CASE_NAMES + SM.COLLISION_NAMES + ["mixed-3000"]


def _tuple(m):
    return m.nrows, m.ncols, m.rp, m.ci, m.va


def test_symbols_struct_and_constants():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    src = open(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_spgemm.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.SpGemmInfo) == 120          # twelve int64, two int32, two doubles
    assert re.search(rf"kGroupLimit = {SM.GROUP_LIMIT}, kBlockLimit = {SM.BLOCK_LIMIT};", src) and re.search(rf"kLanes = {SM.LANES},", src)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", HOST_CASES)
def test_the_host_twin_is_the_model_byte_for_byte(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    a, b = SM.named(name, dtype)
    want = SM.spgemm(a, b)
    rp, ci, va = capi.spgemm_host(_tuple(a), _tuple(b))
    assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci), name
    assert va.dtype == dtype and va.tobytes() == want.va.tobytes(), name


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("nproducts", [SM.GROUP_LIMIT - 1, SM.GROUP_LIMIT, SM.GROUP_LIMIT + 1, SM.BLOCK_LIMIT - 1, SM.BLOCK_LIMIT, SM.BLOCK_LIMIT + 1])
@pytest.mark.parametrize("distinct", [True, False])
def test_rows_around_the_class_limits(nproducts, distinct, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    a, b = SM.limit_pair(nproducts, distinct, dtype)
    assert SM.products(a, b)[0] == nproducts
    want = SM.spgemm(a, b)
    assert want.rp[1] == (nproducts if distinct else 3)
    rp, ci, va = capi.spgemm_host(_tuple(a), _tuple(b))
    assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci) and va.tobytes() == want.va.tobytes()


def test_non_finite_values_and_the_cancelling_entry():
    a, b = SM.named("duplicates", np.float64)
    a.va[3], a.va[11] = np.inf, np.nan
    want = SM.spgemm(a, b)
    rp, ci, va = capi.spgemm_host(_tuple(a), _tuple(b))
    assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci)
    assert np.isnan(want.va).any() and np.isinf(want.va).any()
    assert np.array_equal(np.isnan(va), np.isnan(want.va)) and np.array_equal(np.isinf(va), np.isinf(want.va))
    fin = np.isfinite(want.va)
    assert va[fin].tobytes() == want.va[fin].tobytes() and np.array_equal(va[~fin & ~np.isnan(va)], want.va[~fin & ~np.isnan(va)])
    rp, ci, va = capi.spgemm_host((1, 2, [0, 2], [0, 1], np.array([1.0, -1.0])), (2, 1, [0, 1, 2], [0, 0], np.array([1.0, 1.0])))
    assert list(rp) == [0, 1] and list(ci) == [0] and va.tobytes() == np.zeros(1).tobytes()


def _views(a, b, a_dev=0, b_dev=0):
    keep = [np.ascontiguousarray(x) for x in (a.rp, a.ci, a.va, b.rp, b.ci, b.va)]
    va = capi.CsrView(a.nrows, a.ncols, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, int(a.va.dtype == np.float32), a_dev)
    vb = capi.CsrView(b.nrows, b.ncols, keep[3].ctypes.data, keep[4].ctypes.data, keep[5].ctypes.data, int(b.va.dtype == np.float32), b_dev)
    va._keep = vb._keep = keep          # (the views hold raw pointers: the arrays live as long as either of them)
    return va, vb, keep


def _host(va, vb, m, full=False):
    crp, bad = np.full(m + 1, -5, dtype=np.int64), C.c_int64(-7)
    cci, cva = np.zeros(64, dtype=np.int32), np.zeros(64)
    rc = capi.lib().cvr_spgemm_host(C.byref(va), C.byref(vb), crp.ctypes.data, cci.ctypes.data if full else None, cva.ctypes.data if full else None, C.byref(bad))
    return rc, capi.last_error(), bad.value, crp


def test_the_two_call_shape():
    a, b = SM.named("rect-7x130x5", np.float64)
    want = SM.spgemm(a, b)
    va, vb, keep = _views(a, b)
    rc, _, bad, crp = _host(va, vb, a.nrows)
    assert rc == 0 and bad == -1 and np.array_equal(crp, want.rp)          # columns and values NULL: row_ptr alone
    rc, _, bad, crp = _host(va, vb, a.nrows, full=True)
    assert rc == 0 and bad == -1 and np.array_equal(crp, want.rp)
    # a non-zero first row pointer of both inputs
    a2 = SM.Csr(a.nrows, a.ncols, a.rp + 3, np.r_[np.zeros(3, dtype=np.int32), a.ci], np.r_[np.full(3, 9.0), a.va])
    b2 = SM.Csr(b.nrows, b.ncols, b.rp + 2, np.r_[np.array([4, 4], dtype=np.int32), b.ci], np.r_[np.full(2, 9.0), b.va])
    rp, ci, vals = capi.spgemm_host(_tuple(a2), _tuple(b2))
    assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci) and vals.tobytes() == want.va.tobytes()


def test_every_error_return():
    L = capi.lib()
    a, b = SM.named("rect-7x130x5", np.float64)
    va, vb, keep = _views(a, b)
    crp, bad = np.zeros(8, dtype=np.int64), C.c_int64(-7)
    cci = np.zeros(64, dtype=np.int32)
    good = [C.byref(va), C.byref(vb), crp.ctypes.data, None, None, C.byref(bad)]
    for k in (0, 1, 2, 5):
        args = list(good)
        args[k] = None
        assert L.cvr_spgemm_host(*args) == capi.ERR_INVALID, k
    args = list(good)
    args[3] = cci.ctypes.data          # col_idx without vals
    assert L.cvr_spgemm_host(*args) == capi.ERR_INVALID and bad.value == -1
    # B out of order, and with a duplicate: the first offending row is named
    for cols, row in (([0, 2, 1, 3, 4], 1), ([0, 1, 2, 4, 4], 2)):
        bb = SM.Csr(3, 5, [0, 1, 3, 5], cols, np.ones(5))
        aa = SM.Csr(2, 3, [0, 1, 2], [0, 2], np.ones(2))
        rc, msg, badrow, _ = _host(*_views(aa, bb)[:2], 2)
        assert rc == capi.ERR_INVALID and badrow == row and f"B row {row}:" in msg and "strictly increasing" in msg, msg
        with pytest.raises(capi.CvrError) as e:
            capi.spgemm_host(_tuple(aa), _tuple(bb))
        assert e.value.code == capi.ERR_INVALID and e.value.bad_row == row
    aa = SM.Csr(2, 3, [0, 1, 2], [0, 2], np.ones(2))
    bb = SM.Csr(3, 5, [0, 1, 2, 3], [0, 1, 2], np.ones(3))
    rc, msg, badrow, _ = _host(*_views(aa, bb.astype(np.float32))[:2], 2)
    assert rc == capi.ERR_INVALID and badrow == -1 and "is_f32" in msg
    rc, msg, badrow, _ = _host(*_views(SM.Csr(2, 4, aa.rp, aa.ci, aa.va), bb)[:2], 2)
    assert rc == capi.ERR_INVALID and badrow == -1 and "inner dimensions" in msg
    for a_dev, b_dev in ((1, 0), (0, 1), (1, 1)):
        rc, msg, _, _ = _host(*_views(aa, bb, a_dev, b_dev)[:2], 2)
        assert rc == capi.ERR_INVALID and "host arrays" in msg
    rc, msg, _, _ = _host(*_views(aa, SM.Csr(3, 2 ** 31 - 1, bb.rp, bb.ci, bb.va))[:2], 2)
    assert rc == capi.ERR_INVALID and "2^31 - 1" in msg
    # malformed CSRs, as cvr_create finds them
    for broken_a, broken_b in ((SM.Csr(2, 3, [0, 2, 1], [0, 2], np.ones(2)), bb), (SM.Csr(2, 3, [0, 1, 2], [0, 3], np.ones(2)), bb), (SM.Csr(2, 3, [-1, 1, 2], [0, 2], np.ones(2)), bb),
                               (aa, SM.Csr(3, 5, [0, 1, 2, 3], [0, 5, 2], np.ones(3))), (aa, SM.Csr(3, 5, [0, 2, 1, 3], [0, 1, 2], np.ones(3)))):
        rc, msg, badrow, _ = _host(*_views(broken_a, broken_b)[:2], 2)
        assert rc == capi.ERR_INVALID and badrow == -1, msg
    # the device entry points: their argument checks come before any device work
    g = C.c_void_p()
    assert L.cvr_spgemm_create(None, C.byref(va), C.byref(vb), 0, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_create(C.byref(g), None, C.byref(vb), 0, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_create(C.byref(g), C.byref(va), None, 0, None) == capi.ERR_INVALID
    v32 = _views(aa, bb.astype(np.float32))
    assert L.cvr_spgemm_create(C.byref(g), C.byref(v32[0]), C.byref(v32[1]), 0, None) == capi.ERR_INVALID and "is_f32" in capi.last_error()
    vin = _views(SM.Csr(2, 4, aa.rp, aa.ci, aa.va), bb)
    assert L.cvr_spgemm_create(C.byref(g), C.byref(vin[0]), C.byref(vin[1]), 0, None) == capi.ERR_INVALID and "inner dimensions" in capi.last_error()
    vmix = _views(aa, bb, 0, 1)
    assert L.cvr_spgemm_create(C.byref(g), C.byref(vmix[0]), C.byref(vmix[1]), 0, None) == capi.ERR_INVALID and not g.value
    assert L.cvr_spgemm_destroy(None) == 0
    info = capi.SpGemmInfo()
    assert L.cvr_spgemm_get_info(None, C.byref(info)) == capi.ERR_INVALID and L.cvr_spgemm_export(None, None, None, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_csr_device(None, C.byref(va)) == capi.ERR_INVALID and L.cvr_spgemm_numeric_device(None, None, None, None) == capi.ERR_INVALID


def test_the_host_code_runs_clean_under_the_sanitizers():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "cvr_amd", "csrc"), "spgemm-asan-check"], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases ran clean" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
