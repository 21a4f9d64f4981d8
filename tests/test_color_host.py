"""CPU: cvr_color_host through the ABI against tests/mcsgs_model.py, byte for byte on every case, and every error with its text -- the host twin of
the graph colouring needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcsgs_model as M
from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_color_host", "cvr_color_device", "cvr_precond_mcsgs", "cvr_precond_mcsgs_info", "cvr_precond_mcsgs_export"]


def test_symbols_and_struct():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.McSgsInfo) == 80          # two int64, seven int32, eight reserved, padded to the int64
    assert "} cvr_mcsgs_info;" in hdr
    for name in ("color_host", "color_device", "McSgsInfo"):
        assert hasattr(capi, name), name
    for name in ("mcsgs", "mcsgs_from_device", "mcsgs_info", "mcsgs_export"):
        assert hasattr(capi.Precond, name), name


@pytest.mark.parametrize("name", M.CASES)
def test_every_case_against_the_model(name):
    n, rp, ci, va, color, ncolors, rounds, perm, ptr = M.case(name)
    got = capi.color_host(rp, ci)
    assert (got[3], got[4]) == (ncolors, rounds), (name, got[3], got[4])
    assert got[0].dtype == np.int32 and got[0].tobytes() == color.tobytes(), name
    assert got[1].tobytes() == perm.tobytes() and got[2].tobytes() == ptr.tobytes(), name


def test_n_zero_and_a_shifted_first_row_pointer():
    color, perm, ptr, nc, rounds = capi.color_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    assert (len(color), len(perm), ptr.tolist(), nc, rounds) == (0, 0, [0], 0, 0)
    n, rp, ci, va, color, ncolors, rounds, perm, ptr = M.case("laplacian-24")
    got = capi.color_host(rp + 11, np.concatenate([np.full(11, 3, dtype=np.int32), ci]))          # row_ptr indexes col_idx as it stands
    assert got[0].tobytes() == color.tobytes() and got[1].tobytes() == perm.tobytes() and (got[3], got[4]) == (ncolors, rounds)


def _call(n, ncols, rp, ci, on_device=0):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    color, perm, ptr = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    a, b = C.c_int32(7), C.c_int32(7)
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, None, 0, on_device)
    rc = L.cvr_color_host(C.byref(view), color.ctypes.data, perm.ctypes.data, ptr.ctypes.data, C.byref(a), C.byref(b))
    assert rc == 0 or (a.value, b.value) == (0, 0)
    return rc, capi.last_error()


def test_every_error_and_its_text():
    rc, msg = _call(3, 4, [0, 1, 2, 3], [0, 1, 2])
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: the colouring needs a square matrix (3 x 4)"
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3])          # row 2: 2 before 1
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: row 2: the columns are not strictly increasing (1 behind 2)"
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 2, 3])          # row 2: a duplicate
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: row 2: the columns are not strictly increasing (2 behind 2)"
    rc, msg = _call(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3])          # row 2 has columns 1 and 3
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: row 2 has no diagonal entry"
    rc, msg = _call(3, 3, [0, 1, 1, 2], [0, 2])          # an empty row
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: row 1 has no diagonal entry"
    rc, msg = _call(2, 2, [0, 1, 2], [0, 5])          # cvr_create's check: a column outside the matrix
    assert rc == capi.ERR_INVALID
    rc, msg = _call(2, 2, [0, 1, 2], [0, 1], on_device=1)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: the arrays must be host arrays"


def test_an_asymmetric_pattern_names_the_lowest_row_and_its_lowest_column():
    # rows 1 and 3 both have entries without an answer; row 1 misses (2, 1) and (3, 1): row 1, column 2 is named
    rp, ci = [0, 1, 4, 5, 7, 8], [0, 1, 2, 3, 2, 3, 4, 4]
    assert M.check_pattern(rp, ci) == ("symmetric", 1, 2)
    rc, msg = _call(5, 5, rp, ci)
    assert rc == capi.ERR_INVALID
    assert msg == "cvr_color_host: row 1 has an entry in column 2, row 2 none in column 1: the off-diagonal pattern must be structurally symmetric"
    # a stored zero counts as an entry: the pattern alone decides (the values are not read, vals is NULL here)
    rc, msg = _call(2, 2, [0, 2, 4], [0, 1, 0, 1])
    assert rc == 0
    # the structure rules come first, whatever the rows' order
    rc, msg = _call(3, 3, [0, 2, 3, 4], [0, 2, 1, 1])          # row 0 has (0, 2) unanswered, row 2 has no diagonal
    assert rc == capi.ERR_INVALID and msg == "cvr_color_host: row 2 has no diagonal entry"


def test_null_arguments():
    L = capi.lib()
    rp, ci = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    color, perm, ptr = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)
    a, b = C.c_int32(), C.c_int32()
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, None, 0, 0)
    args = [C.byref(view), color.ctypes.data, perm.ctypes.data, ptr.ctypes.data, C.byref(a), C.byref(b)]
    for k in range(6):
        bad = list(args)
        bad[k] = None
        assert L.cvr_color_host(*bad) == capi.ERR_INVALID and capi.last_error() == "null argument", k
    assert L.cvr_color_host(*args) == 0 and (a.value, b.value, color.tolist(), ptr.tolist()[:2]) == (1, 1, [0, 0], [0, 2])
    null_rp = capi.CsrView(2, 2, None, ci.ctypes.data, None, 0, 0)
    assert L.cvr_color_host(C.byref(null_rp), *args[1:]) == capi.ERR_INVALID
    # without a device the other new entry points decline before they touch one
    p = C.c_void_p()
    assert L.cvr_precond_mcsgs(None, C.byref(view), 0, None) == capi.ERR_INVALID and L.cvr_precond_mcsgs(C.byref(p), None, 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_mcsgs_info(None, None) == capi.ERR_INVALID and L.cvr_precond_mcsgs_export(None, None, None, None) == capi.ERR_INVALID
    assert L.cvr_color_device(None, 0, None, None, None, None, None, None) == capi.ERR_INVALID
