"""CPU: cvr_ilu0_levels_host through the ABI against tests/ilu_model.py -- the analysis of cvr_precond_ilu0 needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilu_model as IM
import krylov_model as KM
from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_ilu0", "cvr_precond_ilu0_info", "cvr_precond_ilu0_export", "cvr_ilu0_levels_host"]


def test_symbols_and_struct():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.Ilu0Info) == 80          # two int64, eight int32, eight reserved
    assert "reserved[8]" in hdr


def _check(rp, ci):
    lo, up, nlo, nup = capi.ilu0_levels_host(rp, ci)
    mlo, mup, mnlo, mnup = IM.levels(np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64))
    assert (nlo, nup) == (mnlo, mnup)
    assert np.array_equal(lo, mlo) and np.array_equal(up, mup)
    return nlo, nup


@pytest.mark.parametrize("n", [1, 2, 65])
def test_banded(n):
    _, _, rp, ci, _ = KM.banded("spd", n, np.float64)
    assert _check(rp, ci) == (n, n)          # every row reads the one before


@pytest.mark.parametrize("m", [3, 24])
def test_laplacian(m):
    _, _, rp, ci, _ = synth.laplacian_2d(m)
    assert _check(rp, ci) == (2 * m - 1, 2 * m - 1)


def test_empty_strict_triangles_and_n_zero():
    n = 7
    rp, ci = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)          # a diagonal matrix
    assert _check(rp, ci) == (1, 1)
    # upper triangular: L's triangle is empty, U's a chain
    rows = [[i] + ([i + 1] if i + 1 < n else []) for i in range(n)]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    ci = np.concatenate(rows).astype(np.int32)
    assert _check(rp, ci) == (1, n)
    lo, up, nlo, nup = capi.ilu0_levels_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    assert (len(lo), len(up), nlo, nup) == (0, 0, 0, 0)
    _, _, rp, ci, _ = IM.wide_matrix(np.float64)
    assert _check(rp, ci) == (2, 1)


@pytest.mark.parametrize("name", list(IM.IRREGULAR))
def test_irregular(name):
    n, rp, ci, _, _, _, _, nlo, nup, _ = IM.irregular_case(name, "fp64")
    assert _check(rp, ci) == (nlo, nup) and min(nlo, nup) > 20          # rows of unrelated lengths, level-0 rows scattered through the matrix


def _call(n, ncols, rp, ci):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    lo, up = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    a, b = C.c_int32(), C.c_int32()
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, None, 0, 0)
    return L.cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, up.ctypes.data, C.byref(a), C.byref(b)), capi.last_error()


def test_the_three_invalid_cases_name_the_row():
    rc, msg = _call(3, 4, [0, 1, 2, 3], [0, 1, 2])          # not square
    assert rc == capi.ERR_INVALID and "square" in msg
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3])          # row 2: 2 before 1
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 2, 3])          # row 2: a duplicate
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg = _call(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3])          # row 2 has columns 1 and 3
    assert rc == capi.ERR_INVALID and "row 2" in msg and "diagonal" in msg
    rc, msg = _call(3, 3, [0, 1, 1, 2], [0, 2])          # an empty row
    assert rc == capi.ERR_INVALID and "row 1" in msg and "diagonal" in msg
    rc, msg = _call(2, 2, [0, 1, 2], [0, 5])          # cvr_create's check: a column outside the matrix
    assert rc == capi.ERR_INVALID


def test_null_arguments():
    L = capi.lib()
    rp, ci = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    lo, up = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    a, b = C.c_int32(), C.c_int32()
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, None, 0, 0)
    assert L.cvr_ilu0_levels_host(None, lo.ctypes.data, up.ctypes.data, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    assert L.cvr_ilu0_levels_host(C.byref(view), None, up.ctypes.data, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    assert L.cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, None, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    assert L.cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, up.ctypes.data, None, C.byref(b)) == capi.ERR_INVALID
    assert L.cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, up.ctypes.data, C.byref(a), None) == capi.ERR_INVALID
    assert L.cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, up.ctypes.data, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (1, 1)
    null_rp = capi.CsrView(2, 2, None, ci.ctypes.data, None, 0, 0)
    assert L.cvr_ilu0_levels_host(C.byref(null_rp), lo.ctypes.data, up.ctypes.data, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    on_device = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, None, 0, 1)
    assert L.cvr_ilu0_levels_host(C.byref(on_device), lo.ctypes.data, up.ctypes.data, C.byref(a), C.byref(b)) == capi.ERR_INVALID
    # without a device the constructor declines before it touches one
    p = C.c_void_p()
    assert L.cvr_precond_ilu0(None, C.byref(view), 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_ilu0(C.byref(p), None, 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_ilu0_info(None, None) == capi.ERR_INVALID and L.cvr_precond_ilu0_export(None, None) == capi.ERR_INVALID
