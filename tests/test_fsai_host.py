"""CPU: cvr_fsai_factor_host through the ABI against tests/fsai_model.py, byte for byte -- the host twin of cvr_precond_fsai's set-up needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fsai_model as FM
import krylov_model as KM
from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_fsai", "cvr_precond_fsai_info", "cvr_precond_fsai_export", "cvr_fsai_factor_host"]


def test_symbols_and_struct():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.FsaiInfo) == 72          # two int64, two int32, an int64, an int32 and nine reserved
    assert "reserved[9]" in hdr and re.search(r"#define CVR_FSAI_MAX_ROW 32\b", hdr) and capi.FSAI_MAX_ROW == FM.MAX_ROW == 32


matrix, MATRICES = FM.matrix, FM.MATRICES


def _first_difference(a, b):
    u = f"u{a.itemsize}"
    d = np.flatnonzero(a.view(u) != b.view(u))
    return (int(d[0]), a[d[0]], b[d[0]], len(d)) if len(d) else None


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", MATRICES)
def test_the_host_twin_is_the_model_byte_for_byte(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = matrix(name, dtype)
    mrp, mci, mwa, mwb, mbad = FM.factor(rp, ci, va, dtype)
    assert mbad is None and np.isfinite(mwa).all() and np.isfinite(mwb).all()
    wrp, wci, wa, wb, bad = capi.fsai_factor_host(rp, ci, va)
    assert bad is None
    assert np.array_equal(wrp, mrp) and np.array_equal(wci, mci) and wci.dtype == np.int32
    assert wa.dtype == dtype and wa.tobytes() == mwa.tobytes(), (name, prec, _first_difference(wa, mwa))
    assert wb.dtype == dtype and wb.tobytes() == mwb.tobytes(), (name, prec, _first_difference(wb, mwb))
    if name == "dense-40":
        assert FM.pattern(rp, ci)[4] == 8 and int(wrp[-1]) == 32 * 33 // 2 + 8 * 32
    if name == "arrow-100":
        assert list(wci[wrp[99]: wrp[100]]) == list(range(68, 100))          # the 32 nearest the diagonal


def test_the_upper_triangle_is_not_read():
    n, _, rp, ci, va = synth.laplacian_2d(5)
    rows = np.repeat(np.arange(n), np.diff(rp))
    other = va.copy()
    other[ci > rows] = 123.0
    assert capi.fsai_factor_host(rp, ci, va)[2].tobytes() == capi.fsai_factor_host(rp, ci, other)[2].tobytes()


def test_n_zero():
    wrp, wci, wa, wb, bad = capi.fsai_factor_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert (list(wrp), len(wci), len(wa), len(wb), bad) == ([0], 0, 0, 0, None)


def _call(n, ncols, rp, ci, va=None, on_device=0):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ones(max(len(ci), 1)) if va is None else np.ascontiguousarray(va, dtype=np.float64)
    room = max(len(ci), 1)
    wrp, wci, wa, wb = np.zeros(n + 1, dtype=np.int64), np.zeros(room, dtype=np.int32), np.zeros(room), np.zeros(room)
    bad = C.c_int64(-7)
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, on_device)
    rc = L.cvr_fsai_factor_host(C.byref(view), wrp.ctypes.data, wci.ctypes.data, wa.ctypes.data, wb.ctypes.data, C.byref(bad))
    return rc, capi.last_error(), bad.value


def test_the_three_invalid_cases_name_the_row():
    rc, msg, _ = _call(3, 4, [0, 1, 2, 3], [0, 1, 2])          # not square
    assert rc == capi.ERR_INVALID and "square" in msg
    rc, msg, _ = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3])          # row 2: 2 before 1
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg, _ = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 2, 3])          # row 2: a duplicate
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg, _ = _call(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3])          # row 2 has columns 1 and 3
    assert rc == capi.ERR_INVALID and "row 2" in msg and "diagonal" in msg
    rc, msg, _ = _call(3, 3, [0, 1, 1, 2], [0, 2])          # an empty row
    assert rc == capi.ERR_INVALID and "row 1" in msg and "diagonal" in msg
    rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 5])          # cvr_create's check: a column outside the matrix
    assert rc == capi.ERR_INVALID


def test_a_bad_pivot_names_the_lowest_row():
    rc, msg, bad = _call(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])          # row 1: 1 - 2 * 2
    assert rc == capi.ERR_STATE and bad == 1 and "row 1 " in msg and "pivot" in msg
    n, _, rp, ci, va = KM.banded("spd", 300, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    for v, row in ((-1.0, 0), (0.0, 123), (np.nan, 123), (np.inf, 299)):
        broken = va.copy()
        broken[d[row]] = v
        rc, msg, bad = _call(n, n, rp, ci, broken)
        assert rc == capi.ERR_STATE and bad == row and f"row {row} " in msg, (v, rc, bad, msg)
        wrp, wci, wa, wb, b2 = capi.fsai_factor_host(rp, ci, broken)          # the wrapper: the rows before it, by the model
        m = FM.factor(rp, ci, broken, np.float64)
        assert b2 == m[4] == row and wa.tobytes() == m[2].tobytes() and wb.tobytes() == m[3].tobytes()


def test_null_arguments_and_device_arrays():
    L = capi.lib()
    rp, ci, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    wrp, wci, wa, wb = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2)
    bad = C.c_int64()
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    args = [C.byref(view), wrp.ctypes.data, wci.ctypes.data, wa.ctypes.data, wb.ctypes.data, C.byref(bad)]
    for k in range(6):
        a = list(args)
        a[k] = None
        assert L.cvr_fsai_factor_host(*a) == capi.ERR_INVALID, k
    assert L.cvr_fsai_factor_host(*args) == 0 and bad.value == -1 and list(wrp) == [0, 1, 2] and list(wa) == [1, 1] and list(wb) == [1, 1]
    null_rp = capi.CsrView(2, 2, None, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_fsai_factor_host(C.byref(null_rp), *args[1:]) == capi.ERR_INVALID
    rc, msg, _ = _call(2, 2, rp, ci, va, on_device=1)
    assert rc == capi.ERR_INVALID and "host arrays" in msg
    # without a device the constructor and its companions decline before they touch one
    p = C.c_void_p()
    assert L.cvr_precond_fsai(None, C.byref(view), 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_fsai(C.byref(p), None, 0, None) == capi.ERR_INVALID
    rect = capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_precond_fsai(C.byref(p), C.byref(rect), 0, None) == capi.ERR_INVALID and "square" in capi.last_error()
    assert L.cvr_precond_fsai_info(None, None) == capi.ERR_INVALID and L.cvr_precond_fsai_export(None, None, None, None, None) == capi.ERR_INVALID
