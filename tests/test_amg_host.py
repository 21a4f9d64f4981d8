"""CPU: cvr_amg_setup_host through the ABI against tests/amg_model.py, byte for byte -- the set-up of cvr_precond_amg is host code and needs no
device; the option and view checks of both entry points come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_model as AM
import krylov_model as KM
from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_amg_default_options", "cvr_precond_amg", "cvr_precond_amg_info", "cvr_precond_amg_export_level", "cvr_amg_setup_host", "cvr_amg_hierarchy_info",
       "cvr_amg_hierarchy_export_level", "cvr_amg_hierarchy_destroy"]


def test_symbols_structs_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.AmgOptions) == 64          # four int32, two doubles, eight reserved
    assert C.sizeof(capi.AmgInfo) == 336            # six int32, three doubles, 2 x 16 int64, eight reserved
    assert re.search(r"#define CVR_AMG_MAX_LEVELS 16\b", hdr) and re.search(r"#define CVR_AMG_MAX_COARSE 256\b", hdr)
    assert (capi.AMG_MAX_LEVELS, capi.AMG_MAX_COARSE) == (AM.MAX_LEVELS, AM.MAX_COARSE) == (16, 256)
    o = capi.AmgOptions(1, 2, 3, 4, 5.0, 6.0)
    assert L.cvr_amg_default_options(C.byref(o)) == 0
    assert dict(max_levels=o.max_levels, coarse_size=o.coarse_size, sweeps=o.sweeps, strength=o.strength, coarse_scale=o.coarse_scale) == AM.DEFAULTS
    assert o.reserved0 == 0 and not any(o.reserved)
    assert L.cvr_amg_default_options(None) == capi.ERR_INVALID


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", AM.CASES, ids=AM.case_id)
def test_the_host_setup_is_the_model_byte_for_byte(case, prec):
    name, options = case
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = AM.matrix(name, dtype)
    H = AM.setup(rp, ci, va, dtype, **options)
    assert H.bad is None
    info, levels = capi.amg_setup_host(rp, ci, va, **options)
    assert AM.same_hierarchy(H, info, levels) == "", (name, prec)
    o = dict(AM.DEFAULTS, **options)
    assert (info.sweeps, info.is_f32, info.max_levels, info.coarse_size, info.strength, info.coarse_scale) == (
        o["sweeps"], int(dtype == np.float32), o["max_levels"], o["coarse_size"], o["strength"], o["coarse_scale"])
    if name == "diagonal":
        assert (info.levels, info.coarse_direct) == (1, 0)          # a stall: one level, no direct solve
    if options.get("max_levels") == 1:
        assert (info.levels, info.coarse_direct) == (1, 0)
    if options.get("coarse_size") == 1:
        assert info.n[info.levels - 1] == 1 and info.coarse_direct == 1


def test_a_nonzero_first_row_pointer_and_n_zero():
    n, _, rp, ci, va = synth.laplacian_2d(9)
    info, lv = capi.amg_setup_host(rp, ci, va)
    info2, lv2 = capi.amg_setup_host(rp + 3, np.r_[np.zeros(3, dtype=np.int32), ci], np.r_[np.full(3, 9.0), va])
    assert info2.levels == info.levels and all(a.va.tobytes() == b.va.tobytes() and np.array_equal(a.rp, b.rp) for a, b in zip(lv, lv2))
    info, lv = capi.amg_setup_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert (info.levels, info.coarse_direct, info.n[0], info.nnz[0], info.operator_complexity) == (1, 1, 0, 0, 0.0)
    assert (list(lv[0].rp), len(lv[0].ci), len(lv[0].dinv), lv[0].agg, lv[0].winv.shape) == ([0], 0, 0, None, (0, 0))


def _call(n, ncols, rp, ci, va=None, on_device=0, opt=None):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ones(max(len(ci), 1)) if va is None else np.ascontiguousarray(va, dtype=np.float64)
    h, bl, br = C.c_void_p(), C.c_int32(-7), C.c_int64(-7)
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, on_device)
    rc = L.cvr_amg_setup_host(C.byref(h), C.byref(view), None if opt is None else C.byref(opt), C.byref(bl), C.byref(br))
    assert rc != 0 and not h.value
    return rc, capi.last_error(), (bl.value, br.value)


BAD_OPTIONS = [("max_levels", 0), ("max_levels", 17), ("coarse_size", 0), ("coarse_size", 257), ("sweeps", 0), ("sweeps", 5), ("reserved0", 1), ("strength", -0.1),
               ("strength", 1.0), ("strength", np.nan), ("coarse_scale", 0.0), ("coarse_scale", -1.0), ("coarse_scale", np.inf), ("coarse_scale", np.nan)]


def test_the_option_checks():
    for field, v in BAD_OPTIONS:
        rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], opt=capi.amg_options(**{field: v}))
        assert rc == capi.ERR_INVALID and field in msg, (field, v, msg)
    o = capi.amg_options()
    o.reserved[7] = -1
    rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], opt=o)
    assert rc == capi.ERR_INVALID and "reserved[7]" in msg


def test_the_view_checks_name_the_row():
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
    rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], on_device=1)
    assert rc == capi.ERR_INVALID and "host arrays" in msg


def test_a_bad_diagonal_and_a_singular_coarsest_matrix_report_level_and_row():
    n, _, rp, ci, va = KM.banded("spd", 300, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    for v, row in ((-1.0, 0), (0.0, 123), (np.nan, 123), (np.inf, 299)):
        broken = va.copy()
        broken[d[row]] = v
        rc, msg, bad = _call(n, n, rp, ci, broken)
        assert rc == capi.ERR_STATE and bad == (0, row) and "level 0" in msg and f"row {row} " in msg and "diagonal" in msg, (v, rc, bad, msg)
        assert AM.setup(rp, ci, broken, np.float64).bad == (0, row, "diagonal")
        with pytest.raises(capi.CvrError) as e:
            capi.amg_setup_host(rp, ci, broken)
        assert e.value.code == capi.ERR_STATE and e.value.bad == (0, row)
    rc, msg, bad = _call(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])          # row 1: 1 - 2 * 2
    assert rc == capi.ERR_STATE and bad == (0, 1) and "level 0" in msg and "row 1 " in msg and "pivot" in msg
    # singular on a coarse level: the Neumann chain (row sums 0) aggregates in pairs, and its 50 x 50 Galerkin matrix is singular again
    m = 100
    A = np.zeros((m, m))
    for i in range(m - 1):
        A[i, i] += 1
        A[i + 1, i + 1] += 1
        A[i, i + 1] = A[i + 1, i] = -1
    _, _, rp, ci, va = AM._csr_of_dense(A, np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    assert H.bad is not None and H.bad[0] >= 1 and H.bad[2] == "pivot", H.bad
    rc, msg, bad = _call(m, m, rp, ci, va)
    assert rc == capi.ERR_STATE and bad == H.bad[:2] and f"level {bad[0]}" in msg and f"row {bad[1]} " in msg and "pivot" in msg, (bad, H.bad, msg)


def test_null_arguments_and_the_constructors_checks_before_any_device_work():
    L = capi.lib()
    rp, ci, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    h, bl, br = C.c_void_p(), C.c_int32(), C.c_int64()
    args = [C.byref(h), C.byref(view), None, C.byref(bl), C.byref(br)]
    for k in (0, 1, 3, 4):
        a = list(args)
        a[k] = None
        assert L.cvr_amg_setup_host(*a) == capi.ERR_INVALID, k
    assert L.cvr_amg_setup_host(*args) == 0 and h.value and (bl.value, br.value) == (-1, -1)          # opt NULL: the defaults
    info = capi.AmgInfo()
    assert L.cvr_amg_hierarchy_info(h, C.byref(info)) == 0 and (info.levels, info.coarse_direct, info.n[0], info.sweeps, info.coarse_size) == (1, 1, 2, 1, 64)
    assert L.cvr_amg_hierarchy_info(h, None) == capi.ERR_INVALID and L.cvr_amg_hierarchy_info(None, C.byref(info)) == capi.ERR_INVALID
    o_rp, o_ci, o_va, o_d, o_w = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2), np.zeros(4)
    full = [o_rp.ctypes.data, o_ci.ctypes.data, o_va.ctypes.data, o_d.ctypes.data, None, o_w.ctypes.data]          # agg: untouched on the coarsest level
    assert L.cvr_amg_hierarchy_export_level(h, 0, *full) == 0 and list(o_w) == [1, 0, 0, 1] and list(o_d) == [1, 1]
    assert L.cvr_amg_hierarchy_export_level(h, 1, *full) == capi.ERR_INVALID and L.cvr_amg_hierarchy_export_level(h, -1, *full) == capi.ERR_INVALID
    for k in (0, 1, 2, 3, 5):
        a = list(full)
        a[k] = None
        assert L.cvr_amg_hierarchy_export_level(h, 0, *a) == capi.ERR_INVALID, k
    assert L.cvr_amg_hierarchy_export_level(None, 0, *full) == capi.ERR_INVALID
    assert L.cvr_amg_hierarchy_destroy(h) == 0 and L.cvr_amg_hierarchy_destroy(None) == 0
    # cvr_precond_amg without a device: the null checks and the options come before the handle is looked at
    p = C.c_void_p()
    fake = C.c_void_p(1)
    assert L.cvr_precond_amg(None, fake, C.byref(view), None, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg(C.byref(p), None, C.byref(view), None, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg(C.byref(p), fake, None, None, None) == capi.ERR_INVALID
    for field, v in BAD_OPTIONS:
        o = capi.amg_options(**{field: v})
        assert L.cvr_precond_amg(C.byref(p), fake, C.byref(view), C.byref(o), None) == capi.ERR_INVALID and field in capi.last_error(), field
    rect = capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_precond_amg(C.byref(p), fake, C.byref(rect), None, None) == capi.ERR_INVALID and "square" in capi.last_error()
    assert L.cvr_precond_amg_info(None, None) == capi.ERR_INVALID and L.cvr_precond_amg_export_level(None, 0, None, None, None, None, None, None) == capi.ERR_INVALID
