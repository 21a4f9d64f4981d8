"""CPU: cvr_amg_smoothed_setup_host through the ABI against tests/sa_amg_model.py, byte for byte -- levels and prolongators --, and the checks of
both smoothed entry points that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_model as AM
import krylov_model as KM
import sa_amg_model as SA
from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_amg_smoothed", "cvr_amg_smoothed_setup_host", "cvr_precond_amg_smoothed_info", "cvr_amg_hierarchy_smoothed_info",
       "cvr_precond_amg_export_prolongator", "cvr_amg_hierarchy_export_prolongator"]


def test_symbols_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.AmgSmoothedInfo) == 176          # two int32, a double, 16 int64, eight reserved
    assert C.sizeof(capi.AmgOptions) == 64 and C.sizeof(capi.AmgInfo) == 336          # the plain kind's structs are as they were
    assert SA.DEFAULT_OMEGA == 4.0 / 3.0


# (name, options, omega): the issue's cases
CASES = [("laplacian-24", {}, 0.0), ("laplacian-23", {}, 0.0), ("singletons", {}, 0.0), ("blocks", {}, 0.0), ("diagonal", {}, 0.0), ("zero-entry", {}, 0.0),
         ("laplacian-40", dict(max_levels=2), 0.0), ("laplacian-24", {}, 0.9), ("laplacian-24", dict(sweeps=2, coarse_scale=1.5, coarse_size=10), 1.9)]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]},{c[1]},omega={c[2]}")
def test_the_host_setup_is_the_model_byte_for_byte(case, prec):
    name, options, omega = case
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = SA.matrix(name, dtype)
    H = SA.cached_setup(name, dtype, omega, **options)
    assert H.bad is None
    info, sinfo, levels, pro = capi.amg_smoothed_setup_host(rp, ci, va, omega, **options)
    assert SA.same_hierarchy(H, info, sinfo, levels, pro) == "", (name, prec)
    o = dict(AM.DEFAULTS, **options)
    assert (info.sweeps, info.is_f32, info.max_levels, info.coarse_size, info.strength, info.coarse_scale) == (
        o["sweeps"], int(dtype == np.float32), o["max_levels"], o["coarse_size"], o["strength"], o["coarse_scale"])
    assert sinfo.omega == (4.0 / 3.0 if omega == 0.0 else omega)
    if name == "diagonal":          # a stall: one level, smoothed, no prolongator
        assert (info.levels, info.coarse_direct, len(pro), sinfo.products_per_apply, sinfo.p_nnz[0]) == (1, 0, 0, 1, 0)
    if options.get("max_levels") == 2:          # a coarsest level of 280 rows, smoothed and not inverted
        assert (info.levels, info.coarse_direct, info.n[1], sinfo.products_per_apply) == (2, 0, 280, 4 + 1)
    if name == "zero-entry":          # the stored 0.0 keeps its entry: P's pattern is G's, structural
        assert (pro[0].va == 0).any() and sinfo.p_nnz[0] == len(H.P[0].ci)
    for l, e in enumerate(levels[:-1]):          # agg is the tentative aggregation, and every row of P holds its column
        p = pro[l]
        assert all(e.agg[i] in p.ci[p.rp[i]: p.rp[i + 1]] for i in range(e.n))


def test_n_zero_a_nonzero_first_row_pointer_and_the_plain_hierarchy():
    L = capi.lib()
    info, sinfo, lv, pro = capi.amg_smoothed_setup_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert (info.levels, info.coarse_direct, info.n[0], info.nnz[0], sinfo.smoothed, sinfo.products_per_apply, pro) == (1, 1, 0, 0, 1, 0, [])
    n, _, rp, ci, va = synth.laplacian_2d(12)
    a = capi.amg_smoothed_setup_host(rp, ci, va)
    b = capi.amg_smoothed_setup_host(rp + 3, np.r_[np.zeros(3, dtype=np.int32), ci], np.r_[np.full(3, 9.0), va])
    assert a[0].levels == b[0].levels >= 2 and all(x.va.tobytes() == y.va.tobytes() and np.array_equal(x.rp, y.rp) for x, y in zip(a[2] + a[3], b[2] + b[3]))
    # the plain hierarchy: the info all zero, no prolongator; a smoothed one: the coarsest level and levels outside have none
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    h, s, bl, br = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int64()
    assert L.cvr_amg_setup_host(C.byref(h), C.byref(view), None, C.byref(bl), C.byref(br)) == 0
    assert L.cvr_amg_smoothed_setup_host(C.byref(s), C.byref(view), None, 0.0, C.byref(bl), C.byref(br)) == 0 and (bl.value, br.value) == (-1, -1)
    try:
        si = capi.AmgSmoothedInfo(1, 1, 1.0)
        assert L.cvr_amg_hierarchy_smoothed_info(h, C.byref(si)) == 0 and bytes(si) == bytes(C.sizeof(si))
        p0 = a[3][0]
        args = (p0.rp.ctypes.data, p0.ci.ctypes.data, p0.va.ctypes.data)
        assert L.cvr_amg_hierarchy_export_prolongator(h, 0, *args) == capi.ERR_INVALID and "plain" in capi.last_error()
        levels = a[0].levels
        assert L.cvr_amg_hierarchy_export_prolongator(s, levels - 1, *args) == capi.ERR_INVALID and "level" in capi.last_error()
        assert L.cvr_amg_hierarchy_export_prolongator(s, levels, *args) == capi.ERR_INVALID and L.cvr_amg_hierarchy_export_prolongator(s, -1, *args) == capi.ERR_INVALID
        for k in range(3):
            bad = list(args)
            bad[k] = None
            assert L.cvr_amg_hierarchy_export_prolongator(s, 0, *bad) == capi.ERR_INVALID, k
        assert L.cvr_amg_hierarchy_export_prolongator(None, 0, *args) == capi.ERR_INVALID
        assert L.cvr_amg_hierarchy_smoothed_info(s, None) == capi.ERR_INVALID and L.cvr_amg_hierarchy_smoothed_info(None, C.byref(si)) == capi.ERR_INVALID
        before = p0.va.copy()
        assert L.cvr_amg_hierarchy_export_prolongator(s, 0, *args) == 0 and p0.va.tobytes() == before.tobytes()
    finally:
        L.cvr_amg_hierarchy_destroy(h)
        L.cvr_amg_hierarchy_destroy(s)


def _call(n, ncols, rp, ci, va=None, on_device=0, opt=None, omega=0.0):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ones(max(len(ci), 1)) if va is None else np.ascontiguousarray(va, dtype=np.float64)
    h, bl, br = C.c_void_p(), C.c_int32(-7), C.c_int64(-7)
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, on_device)
    rc = L.cvr_amg_smoothed_setup_host(C.byref(h), C.byref(view), None if opt is None else C.byref(opt), omega, C.byref(bl), C.byref(br))
    assert rc != 0 and not h.value
    return rc, capi.last_error(), (bl.value, br.value)


BAD_OPTIONS = [("max_levels", 0), ("max_levels", 17), ("coarse_size", 0), ("coarse_size", 257), ("sweeps", 0), ("sweeps", 5), ("reserved0", 1), ("strength", -0.1),
               ("strength", 1.0), ("strength", np.nan), ("coarse_scale", 0.0), ("coarse_scale", -1.0), ("coarse_scale", np.inf), ("coarse_scale", np.nan)]
BAD_OMEGAS = [np.nan, -0.5, 2.0, np.inf, -np.inf, 2.5]


def test_omega_and_the_option_checks_in_the_plain_entry_points_order():
    for omega in BAD_OMEGAS:
        rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], omega=omega)
        assert rc == capi.ERR_INVALID and "omega" in msg, (omega, msg)
    for field, v in BAD_OPTIONS:          # the options come first ...
        rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], opt=capi.amg_options(**{field: v}), omega=np.nan)
        assert rc == capi.ERR_INVALID and field in msg and "omega" not in msg, (field, v, msg)
    o = capi.amg_options()
    o.reserved[7] = -1
    rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], opt=o)
    assert rc == capi.ERR_INVALID and "reserved[7]" in msg
    # ... and omega before the view
    rc, msg, _ = _call(3, 4, [0, 1, 2, 3], [0, 1, 2], omega=2.0)
    assert rc == capi.ERR_INVALID and "omega" in msg
    rc, msg, _ = _call(3, 4, [0, 1, 2, 3], [0, 1, 2])
    assert rc == capi.ERR_INVALID and "square" in msg
    rc, msg, _ = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3])
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg, _ = _call(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3])
    assert rc == capi.ERR_INVALID and "row 2" in msg and "diagonal" in msg
    rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], on_device=1)
    assert rc == capi.ERR_INVALID and "host arrays" in msg
    L = capi.lib()
    rp, ci, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    h, bl, br = C.c_void_p(), C.c_int32(), C.c_int64()
    args = [C.byref(h), C.byref(view), None, 0.0, C.byref(bl), C.byref(br)]
    for k in (0, 1, 4, 5):
        a = list(args)
        a[k] = None
        assert L.cvr_amg_smoothed_setup_host(*a) == capi.ERR_INVALID, k
    # cvr_precond_amg_smoothed without a device: nulls, options, omega and the shape come before the handle is looked at
    p, fake = C.c_void_p(), C.c_void_p(1)
    assert L.cvr_precond_amg_smoothed(None, fake, C.byref(view), None, 0.0, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg_smoothed(C.byref(p), None, C.byref(view), None, 0.0, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg_smoothed(C.byref(p), fake, None, None, 0.0, None) == capi.ERR_INVALID
    for field, v in BAD_OPTIONS:
        o = capi.amg_options(**{field: v})
        assert L.cvr_precond_amg_smoothed(C.byref(p), fake, C.byref(view), C.byref(o), np.nan, None) == capi.ERR_INVALID and field in capi.last_error(), field
    for omega in BAD_OMEGAS:
        assert L.cvr_precond_amg_smoothed(C.byref(p), fake, C.byref(view), None, omega, None) == capi.ERR_INVALID and "omega" in capi.last_error(), omega
    rect = capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_precond_amg_smoothed(C.byref(p), fake, C.byref(rect), None, 0.0, None) == capi.ERR_INVALID and "square" in capi.last_error()
    assert L.cvr_precond_amg_smoothed_info(None, None) == capi.ERR_INVALID and L.cvr_precond_amg_export_prolongator(None, 0, None, None, None) == capi.ERR_INVALID


def test_a_bad_diagonal_reports_level_and_row():
    n, _, rp, ci, va = KM.banded("spd", 300, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    for v, row in ((-1.0, 0), (0.0, 123), (np.nan, 123), (np.inf, 299)):
        broken = va.copy()
        broken[d[row]] = v
        rc, msg, bad = _call(n, n, rp, ci, broken)
        assert rc == capi.ERR_STATE and bad == (0, row) and "level 0" in msg and f"row {row} " in msg and "diagonal" in msg, (v, rc, bad, msg)
        assert SA.setup(rp, ci, broken, np.float64).bad == (0, row, "diagonal")
        with pytest.raises(capi.CvrError) as e:
            capi.amg_smoothed_setup_host(rp, ci, broken)
        assert e.value.code == capi.ERR_STATE and e.value.bad == (0, row)
    # on a coarse level: the Neumann chain (row sums 0); its Galerkin matrices stay singular, so some level's pivot is not > 0 -- wherever the
    # model finds it, the library names the same level and row
    m = 100
    A = np.zeros((m, m))
    for i in range(m - 1):
        A[i, i] += 1
        A[i + 1, i + 1] += 1
        A[i, i + 1] = A[i + 1, i] = -1
    _, _, rp, ci, va = AM._csr_of_dense(A, np.float64)
    H = SA.setup(rp, ci, va, np.float64)
    if H.bad is None:
        info, sinfo, lv, pro = capi.amg_smoothed_setup_host(rp, ci, va)
        assert SA.same_hierarchy(H, info, sinfo, lv, pro) == ""
    else:
        rc, msg, bad = _call(m, m, rp, ci, va)
        assert rc == capi.ERR_STATE and bad == H.bad[:2] and f"level {bad[0]}" in msg and f"row {bad[1]} " in msg, (bad, H.bad, msg)
