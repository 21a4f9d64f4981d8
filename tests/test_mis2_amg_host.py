"""CPU: cvr_amg_mis2_aggregate_host and cvr_amg_mis2_setup_host through the ABI against tests/mis2_amg_model.py, byte for byte -- agg, nc, rounds,
every level, dinv, winv and every prolongator --, and the checks of the new entry points that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_model as AM
import krylov_model as KM
import mis2_amg_model as M
import sa_amg_model as SA
from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_amg_mis2", "cvr_amg_mis2_setup_host", "cvr_precond_amg_mis2_info", "cvr_amg_hierarchy_mis2_info", "cvr_amg_mis2_aggregate_host",
       "cvr_amg_mis2_aggregate_device"]


def test_symbols_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert C.sizeof(capi.AmgMis2Info) == 104          # two int32, 16 int32, eight reserved
    assert C.sizeof(capi.AmgSmoothedInfo) == 176 and C.sizeof(capi.AmgOptions) == 64 and C.sizeof(capi.AmgInfo) == 336          # the others are as they were


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.AGGREGATION_CASES)
def test_the_host_aggregation_is_the_models(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = M.matrix(name, dtype)
    want, nc, rounds = M.cached_aggregate(name, dtype)
    agg, gnc, grounds = capi.amg_mis2_aggregate_host(rp, ci, va)
    assert (gnc, grounds) == (nc, rounds) and agg.dtype == np.int32 and agg.tobytes() == want.tobytes(), (name, prec)
    # a non-zero first row pointer reads the same entries
    agg2, nc2, rounds2 = capi.amg_mis2_aggregate_host(rp + 3, np.r_[np.zeros(3, dtype=np.int32), ci], np.r_[np.full(3, 9.0).astype(dtype), va])
    assert (nc2, rounds2) == (nc, rounds) and np.array_equal(agg2, want)
    if name == "chain":
        assert rounds <= 32


def test_the_host_aggregation_of_no_rows_one_row_and_other_strengths():
    assert capi.amg_mis2_aggregate_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))[1:] == (0, 0)
    agg, nc, rounds = capi.amg_mis2_aggregate_host(np.array([0, 1]), np.array([0]), np.array([2.0]))
    assert (agg.tolist(), nc, rounds) == ([0], 1, 1)
    for name, strength in (("laplacian-24", 0.0), ("lopsided", 0.2), ("lopsided", 0.5)):
        lv = M.level_of(name, np.float64)
        want = M.aggregate(lv, strength)
        got = capi.amg_mis2_aggregate_host(lv.rp, lv.ci, lv.va, strength=strength)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (name, strength)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", M.SETUP_CASES, ids=AM.case_id)
def test_the_host_setup_is_the_model_byte_for_byte(case, prec):
    name, options = case
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = M.matrix(name, dtype)
    H = M.cached_setup(name, dtype, **options)
    assert H.bad is None
    info, sinfo, levels, pro, minfo = capi.amg_mis2_setup_host(rp, ci, va, **options)
    assert SA.same_hierarchy(H, info, sinfo, levels, pro) == "", (name, prec)          # levels, dinv, agg, winv, prolongators, both infos
    assert M.same_rounds(H, minfo) == "", (name, prec)
    assert sinfo.smoothed == 1 and sinfo.omega == 4.0 / 3.0
    if name == "diagonal":          # a stall: one level, no rounds reported
        assert (info.levels, info.coarse_direct, len(pro), any(minfo.rounds)) == (1, 0, 0, False)
    if options.get("max_levels") == 2:          # a coarsest level of 233 rows, inverted directly (<= 256)
        assert (info.levels, info.coarse_direct, info.n[1], list(minfo.rounds)[:2]) == (2, 1, 233, [10, 0])
    for l, e in enumerate(levels[:-1]):          # agg is the tentative aggregation, and every row of P holds its column
        p = pro[l]
        assert all(e.agg[i] in p.ci[p.rp[i]: p.rp[i + 1]] for i in range(e.n))


def test_n_zero_omega_and_hierarchies_built_another_way():
    L = capi.lib()
    info, sinfo, lv, pro, minfo = capi.amg_mis2_setup_host(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert (info.levels, info.coarse_direct, info.n[0], sinfo.smoothed, sinfo.products_per_apply, pro, minfo.mis2, any(minfo.rounds)) == (1, 1, 0, 1, 0, [], 1, False)
    n, _, rp, ci, va = synth.laplacian_2d(24)
    H = M.cached_setup("laplacian-24", np.float64, 0.9)
    got = capi.amg_mis2_setup_host(rp, ci, va, omega=0.9)
    assert SA.same_hierarchy(H, *got[:4]) == "" and got[1].omega == 0.9
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    bl, br = C.c_int32(), C.c_int64()
    plain, smoothed, mis2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.cvr_amg_setup_host(C.byref(plain), C.byref(view), None, C.byref(bl), C.byref(br)) == 0
    assert L.cvr_amg_smoothed_setup_host(C.byref(smoothed), C.byref(view), None, 0.0, C.byref(bl), C.byref(br)) == 0
    assert L.cvr_amg_mis2_setup_host(C.byref(mis2), C.byref(view), None, 0.0, C.byref(bl), C.byref(br)) == 0 and (bl.value, br.value) == (-1, -1)
    try:
        for h in (plain, smoothed):          # built another way: all zero
            mi = capi.AmgMis2Info(1, 1)
            assert L.cvr_amg_hierarchy_mis2_info(h, C.byref(mi)) == 0 and bytes(mi) == bytes(C.sizeof(mi))
        mi, si = capi.AmgMis2Info(), capi.AmgSmoothedInfo()
        assert L.cvr_amg_hierarchy_mis2_info(mis2, C.byref(mi)) == 0 and mi.mis2 == 1 and list(mi.rounds)[:3] == [8, 5, 0]
        assert L.cvr_amg_hierarchy_smoothed_info(mis2, C.byref(si)) == 0 and si.smoothed == 1
        assert L.cvr_amg_hierarchy_mis2_info(mis2, None) == capi.ERR_INVALID and L.cvr_amg_hierarchy_mis2_info(None, C.byref(mi)) == capi.ERR_INVALID
    finally:
        for h in (plain, smoothed, mis2):
            L.cvr_amg_hierarchy_destroy(h)


def _call(n, ncols, rp, ci, va=None, on_device=0, opt=None, omega=0.0):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ones(max(len(ci), 1)) if va is None else np.ascontiguousarray(va, dtype=np.float64)
    h, bl, br = C.c_void_p(), C.c_int32(-7), C.c_int64(-7)
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, on_device)
    rc = L.cvr_amg_mis2_setup_host(C.byref(h), C.byref(view), None if opt is None else C.byref(opt), omega, C.byref(bl), C.byref(br))
    assert rc != 0 and not h.value
    return rc, capi.last_error(), (bl.value, br.value)


BAD_OPTIONS = [("max_levels", 0), ("max_levels", 17), ("coarse_size", 0), ("coarse_size", 257), ("sweeps", 0), ("sweeps", 5), ("reserved0", 1), ("strength", -0.1),
               ("strength", 1.0), ("strength", np.nan), ("coarse_scale", 0.0), ("coarse_scale", -1.0), ("coarse_scale", np.inf), ("coarse_scale", np.nan)]
BAD_OMEGAS = [np.nan, -0.5, 2.0, np.inf, -np.inf, 2.5]


def test_every_error_and_its_text_in_the_smoothed_entry_points_order():
    name = "cvr_amg_mis2_setup_host"
    for omega in BAD_OMEGAS:
        rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], omega=omega)
        assert rc == capi.ERR_INVALID and "omega" in msg and msg.startswith(name + ":"), (omega, msg)
    for field, v in BAD_OPTIONS:          # the options come first ...
        rc, msg, _ = _call(2, 2, [0, 1, 2], [0, 1], opt=capi.amg_options(**{field: v}), omega=np.nan)
        assert rc == capi.ERR_INVALID and field in msg and "omega" not in msg and msg.startswith(name + ":"), (field, v, msg)
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
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg and msg.startswith(name + ":")
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
        assert L.cvr_amg_mis2_setup_host(*a) == capi.ERR_INVALID, k
    # the aggregation alone: nulls, strength, device arrays, shape, structure
    agg, nc, rounds = np.zeros(4, dtype=np.int32), C.c_int64(), C.c_int32()
    ok = [C.byref(view), 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds)]
    for k in (0, 2, 3, 4):
        a = list(ok)
        a[k] = None
        assert L.cvr_amg_mis2_aggregate_host(*a) == capi.ERR_INVALID, k
    for s in (-0.1, 1.0, np.nan):
        assert L.cvr_amg_mis2_aggregate_host(C.byref(view), s, agg.ctypes.data, C.byref(nc), C.byref(rounds)) == capi.ERR_INVALID and "strength" in capi.last_error()
    dev = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 1)
    assert L.cvr_amg_mis2_aggregate_host(C.byref(dev), 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds)) == capi.ERR_INVALID and "host arrays" in capi.last_error()
    rect = capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_amg_mis2_aggregate_host(C.byref(rect), 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds)) == capi.ERR_INVALID and "square" in capi.last_error()
    rp4, ci4 = np.array([0, 1, 2, 4, 5], dtype=np.int64), np.array([0, 1, 1, 3, 3], dtype=np.int32)
    v4 = capi.CsrView(4, 4, rp4.ctypes.data, ci4.ctypes.data, np.ones(5).ctypes.data, 0, 0)
    assert L.cvr_amg_mis2_aggregate_host(C.byref(v4), 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds)) == capi.ERR_INVALID
    assert "row 2" in capi.last_error() and "diagonal" in capi.last_error() and capi.last_error().startswith("cvr_amg_mis2_aggregate_host:")
    assert L.cvr_amg_mis2_aggregate_device(C.byref(view), 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds), 0, None) == capi.ERR_INVALID and "device arrays" in capi.last_error()
    assert L.cvr_amg_mis2_aggregate_device(None, 0.08, agg.ctypes.data, C.byref(nc), C.byref(rounds), 0, None) == capi.ERR_INVALID
    # cvr_precond_amg_mis2 without a device: nulls, options, omega and the shape come before the handle is looked at
    p, fake = C.c_void_p(), C.c_void_p(1)
    assert L.cvr_precond_amg_mis2(None, fake, C.byref(view), None, 0.0, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg_mis2(C.byref(p), None, C.byref(view), None, 0.0, None) == capi.ERR_INVALID
    assert L.cvr_precond_amg_mis2(C.byref(p), fake, None, None, 0.0, None) == capi.ERR_INVALID
    for field, v in BAD_OPTIONS:
        o = capi.amg_options(**{field: v})
        assert L.cvr_precond_amg_mis2(C.byref(p), fake, C.byref(view), C.byref(o), np.nan, None) == capi.ERR_INVALID and field in capi.last_error(), field
        assert capi.last_error().startswith("cvr_precond_amg_mis2:")
    for omega in BAD_OMEGAS:
        assert L.cvr_precond_amg_mis2(C.byref(p), fake, C.byref(view), None, omega, None) == capi.ERR_INVALID and "omega" in capi.last_error(), omega
    assert L.cvr_precond_amg_mis2(C.byref(p), fake, C.byref(rect), None, 0.0, None) == capi.ERR_INVALID and "square" in capi.last_error()
    assert L.cvr_precond_amg_mis2_info(None, None) == capi.ERR_INVALID


def test_a_bad_diagonal_or_pivot_reports_level_and_row():
    n, _, rp, ci, va = KM.banded("spd", 300, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    for v, row in ((-1.0, 0), (0.0, 123), (np.nan, 123), (np.inf, 299)):
        broken = va.copy()
        broken[d[row]] = v
        rc, msg, bad = _call(n, n, rp, ci, broken)
        assert rc == capi.ERR_STATE and bad == (0, row) and "level 0" in msg and f"row {row} " in msg and "diagonal" in msg and msg.startswith("cvr_amg_mis2_setup_host:"), (v, rc, bad, msg)
        assert M.setup(rp, ci, broken, np.float64).bad == (0, row, "diagonal")
        with pytest.raises(capi.CvrError) as e:
            capi.amg_mis2_setup_host(rp, ci, broken)
        assert e.value.code == capi.ERR_STATE and e.value.bad == (0, row)
    # a pivot: an indefinite 3 x 3 matrix with a positive diagonal, inverted on level 0
    rp, ci, va = np.array([0, 2, 4, 5]), np.array([0, 1, 0, 1, 2]), np.array([1.0, 2.0, 2.0, 1.0, 1.0])
    assert M.setup(rp, ci, va, np.float64).bad == (0, 1, "pivot")
    rc, msg, bad = _call(3, 3, rp, ci, va)
    assert rc == capi.ERR_STATE and bad == (0, 1) and "level 0" in msg and "row 1 " in msg and "pivot" in msg
    # on a coarse level: the singular Neumann chain in fp32 -- wherever the model finds it, the library names the same level and row
    m = 100
    A = np.zeros((m, m))
    for i in range(m - 1):
        A[i, i] += 1
        A[i + 1, i + 1] += 1
        A[i, i + 1] = A[i + 1, i] = -1
    for dtype in (np.float32, np.float64):
        _, _, rp, ci, va = AM._csr_of_dense(A, dtype)
        H = M.setup(rp, ci, va, dtype)
        if H.bad is None:
            got = capi.amg_mis2_setup_host(rp, ci, va)
            assert SA.same_hierarchy(H, *got[:4]) == ""
        else:
            with pytest.raises(capi.CvrError) as e:
                capi.amg_mis2_setup_host(rp, ci, va)
            assert e.value.code == capi.ERR_STATE and e.value.bad == H.bad[:2] and f"level {H.bad[0]}" in str(e.value) and f"row {H.bad[1]} " in str(e.value)


# ---- the irregular and the large cases (M.IRREGULAR) ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.IRREGULAR_CASES)
def test_the_host_aggregation_of_the_irregular_cases_is_the_models(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = M.matrix(name, dtype)
    want, nc, rounds = M.cached_aggregate(name, dtype)
    agg, gnc, grounds = capi.amg_mis2_aggregate_host(rp, ci, va)
    assert (gnc, grounds) == (nc, rounds) and agg.dtype == np.int32 and agg.tobytes() == want.tobytes(), (name, prec, np.flatnonzero(agg != want)[:5])


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES)
def test_the_host_setup_of_the_irregular_cases_is_the_model_byte_for_byte(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n, _, rp, ci, va = M.matrix(name, dtype)
    H = M.cached_setup(name, dtype)          # (once per process: 5 to 15 s of Python SpGEMM a case and precision)
    assert H.bad is None
    info, sinfo, levels, pro, minfo = capi.amg_mis2_setup_host(rp, ci, va)
    assert SA.same_hierarchy(H, info, sinfo, levels, pro) == "", (name, prec)
    assert M.same_rounds(H, minfo) == "", (name, prec)
    if name == "irr-spd-3000":          # a coarsest level of more than 256 rows: smoothed, not inverted
        assert info.levels == 4 and info.coarse_direct == 0
