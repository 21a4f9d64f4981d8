"""GPU (MI355X): the sparse matrix-matrix product C = A B -- cvr_spgemm_create, _get_info, _csr_device, _export, _numeric_device, all through the ABI,
byte for byte against tests/spgemm_model.py.

  * the export and the info fields in fp64 and fp32, from host and from device arrays, on spgemm_model's cases, on rows around the two class limits
    (all products distinct: a table as full as it gets; all on 3 columns) and on rows whose columns all have ONE home slot under the kernel's hash,
    in every table size from 64 to 8192 slots, in the middle of the table and at its end (the probe chain wraps)
  * the same bytes under CVR_DEBUG=spgemm_limits=8:64 and =1:1 (fresh child processes), the row counts moving as the limits say
  * reproducibility: created twice, the value arrays off the 16-byte grid one at a time
  * the numeric re-run, non-finite values, C's view as the input of cvr_create, P^T (A P) against the AMG set-up's level 1, every error return"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cvr_amd
import pkrylov_gpu as G
import spgemm_model as SM
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tuple(m):
    return m.nrows, m.ncols, m.rp, m.ci, m.va


@functools.lru_cache(maxsize=None)
def _case(name, prec):
    """(A, B, the model's C, products) -- computed once, shared, never changed"""
    dtype = G.dtype_of(prec)
    a, b = SM.named(name, dtype)
    return a, b, SM.spgemm(a, b), SM.products(a, b)


class OnDevice:
    """a Csr's arrays in device memory; shift: the values start off the 16-byte grid by that many elements"""

    def __init__(self, m, shift=0):
        self.m = m
        self.rp, self.ci = torch.from_numpy(m.rp).cuda(), torch.from_numpy(np.ascontiguousarray(m.ci)).cuda()
        self.va = G.put(m.va, m.va.dtype.type, shift)
        torch.cuda.synchronize()

    def tuple(self):
        return self.m.nrows, self.m.ncols, self.rp.data_ptr(), self.ci.data_ptr(), self.va.data_ptr()


def _from_device(a, b, ashift=0, bshift=0):
    da, db = OnDevice(a, ashift), OnDevice(b, bshift)
    g = capi.SpGemm.from_device(da.tuple(), db.tuple(), is_f32=a.va.dtype == np.float32)
    del da, db          # the object keeps nothing of the caller's arrays
    return g


def _same(g, want, ctx):
    rp, ci, va = g.export()
    assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci), ctx
    assert va.dtype == want.va.dtype and va.tobytes() == want.va.tobytes(), (ctx, np.flatnonzero(va != want.va)[:5])


def _check_info(g, a, b, want, prod, ctx):
    i = g.info()
    assert (i.nrows, i.ncols, i.inner, i.nnz, i.is_f32, i.lanes_per_row) == (a.nrows, b.ncols, a.ncols, len(want.ci), int(a.va.dtype == np.float32), SM.LANES), ctx
    assert (i.products, i.max_row_products) == (int(prod.sum()), int(prod.max()) if len(prod) else 0), ctx
    assert (i.rows_empty, i.rows_group, i.rows_block, i.rows_spill) == SM.row_classes(prod, i.group_limit, i.block_limit), ctx
    assert i.symbolic_s > 0 and i.numeric_s > 0
    return i


def _both_ways(a, b, want, prod, ctx):
    for how in ("host arrays", "device arrays"):
        g = capi.SpGemm.create(_tuple(a), _tuple(b)) if how == "host arrays" else _from_device(a, b)
        try:
            _same(g, want, (ctx, how))
            i = _check_info(g, a, b, want, prod, (ctx, how))
        finally:
            g.close()
    return i


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SM.CASE_NAMES)
def test_export_and_info(name, prec):
    a, b, want, prod = _case(name, prec)
    i = _both_ways(a, b, want, prod, (name, prec))
    assert (i.group_limit, i.block_limit) == (SM.GROUP_LIMIT, SM.BLOCK_LIMIT)
    if name == "dense-row":
        assert i.rows_spill == 1 and i.rows_block == 2


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_rows_of_every_class_side_by_side(prec):
    """mixed-3000: 3000 rows whose products cycle with a period of 7, three consecutive rows to a thread of the bin and the scan kernels: a thread
    bins rows of different classes (the older mixed cases have at most 90 rows, one row a thread)"""
    a, b, want, prod = _case("mixed-3000", prec)
    assert a.nrows == 3000 and prod.tolist() == [SM.MIXED_PRODUCTS[i % 7] for i in range(3000)] and prod.sum() < 150000
    assert SM.row_classes(prod) == (857, 857, 1286, 0)          # 0, 0 | 5, 12 | 40, 100, 70 of every seven rows; 3000 = 428 * 7 + 4, the last four rows 0, 5, 40, 100
    assert all(c > 0 for c in SM.row_classes(prod, 8, 64))          # ... and under 8:64 (test_a_lowered_plan_gives_the_same_bytes) all four classes
    assert (want.terms > 1).any()
    _both_ways(a, b, want, prod, ("mixed-3000", prec))


@functools.lru_cache(maxsize=None)
def _grid_squared(prec):
    """(A, the host twin's A A) for the 513 x 513 grid matrix of mis2_amg_model -- computed once, shared, never changed"""
    import mis2_amg_model as M
    n, _, rp, ci, va = M.matrix("ties-grid-513", G.dtype_of(prec))
    a = SM.Csr(n, n, rp, ci, va)
    return a, capi.spgemm_host(_tuple(a), _tuple(a))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_more_group_rows_than_one_trip_of_the_group_kernel(prec):
    """A A for a 5-point grid of 513^2 = 263 169 rows, every one a group row (at most 25 products): the group kernel takes 4096 workgroups x 32 teams
    = 131 072 rows a trip, so its second and third trips run, and the bin and scan kernels give a thread 258 rows.  Against the host twin
    cvr_spgemm_host, byte for byte: spgemm_model.spgemm is a Python loop over 6.6 million products and would take minutes; the twin is pinned to it
    by tests/test_spgemm_host.py on every smaller case."""
    a, (rp, ci, va) = _grid_squared(prec)
    g = _from_device(a, a)
    try:
        got = g.export()
        i = g.info()
    finally:
        g.close()
    assert np.array_equal(got[0], rp) and np.array_equal(got[1], ci) and got[2].dtype == va.dtype and got[2].tobytes() == va.tobytes()
    assert (i.rows_group, i.rows_block, i.rows_spill, i.rows_empty) == (263169, 0, 0, 0) and i.nnz == len(ci) and i.products > 6500000 and i.max_row_products == 25
    assert (i.group_limit, i.block_limit) == (SM.GROUP_LIMIT, SM.BLOCK_LIMIT)


def _limits():
    one = SM.from_rows(1, 1, [[0]], np.float64)
    g = capi.SpGemm.create(_tuple(one), _tuple(one))
    i = g.info()
    g.close()
    return i.group_limit, i.block_limit


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("distinct", [True, False], ids=["distinct", "3-columns"])
@pytest.mark.parametrize("which,delta", [(w, d) for w in (0, 1) for d in (-1, 0, 1)])
def test_rows_around_the_class_limits(which, delta, distinct, prec):
    limit = _limits()[which]
    nproducts = limit + delta
    a, b = SM.limit_pair(nproducts, distinct, G.dtype_of(prec))
    want, prod = SM.spgemm(a, b), SM.products(a, b)
    assert prod[0] == nproducts and want.rp[1] == (nproducts if distinct else 3)
    i = _both_ways(a, b, want, prod, (nproducts, distinct, prec))
    assert (i.rows_group, i.rows_block, i.rows_spill) == ((1, 0, 0) if (which, delta) == (0, -1) else (0, 1, 0) if which == 0 or delta < 0 else (0, 0, 1))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SM.COLLISION_NAMES)
def test_columns_that_share_one_home_slot_in_every_table(name, prec):
    a, b, want, prod = _case(name, prec)
    ndistinct = int(name.split("-")[1])
    assert want.rp[1] == ndistinct and (want.terms[: ndistinct] >= 1).all() and want.terms.max() == 2
    # the kernel's hash (cvr_spgemm.hip, row_in_table) sends every column of a row to one slot of the row's table: the whole row is one probe chain
    sizes = set()
    for row in (0, 2):
        log2s = SM.table_log2(prod[row])
        homes = {SM.home_slot(j, log2s) for j in want.ci[want.rp[row]: want.rp[row + 1]]}
        assert len(homes) == 1 and (homes == {(1 << log2s) - 1} if name.endswith("-end") else max(homes) < (1 << log2s) - 1), (name, row, homes)
        assert want.rp[row + 1] - want.rp[row] > 1
        sizes.add(log2s)
    assert max(sizes) == SM.table_log2(3 * ndistinct // 2) and 6 <= min(sizes)
    i = _both_ways(a, b, want, prod, (name, prec))
    assert i.rows_spill == 0 and i.rows_empty == 1


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import spgemm_model as SM
from cvr_amd import capi
out = {}
for name in SM.PLAN_CASES:
    for prec, dtype in (("fp64", np.float64), ("fp32", np.float32)):
        a, b = SM.named(name, dtype)
        g = capi.SpGemm.create((a.nrows, a.ncols, a.rp, a.ci, a.va), (b.nrows, b.ncols, b.rp, b.ci, b.va))
        i = g.info()
        rp, ci, va = g.export()
        g.close()
        out[f"{name}/{prec}/rp"], out[f"{name}/{prec}/ci"], out[f"{name}/{prec}/va"] = rp, ci, va
        out[f"{name}/{prec}/info"] = np.array([i.group_limit, i.block_limit, i.rows_empty, i.rows_group, i.rows_block, i.rows_spill, i.nnz, i.products], dtype=np.int64)
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("limits", [(8, 64), (1, 1)], ids=["8:64", "1:1"])
def test_a_lowered_plan_gives_the_same_bytes(limits, tmp_path):
    path = str(tmp_path / "plan.npz")
    env = dict(os.environ, CVR_DEBUG=f"spgemm_limits={limits[0]}:{limits[1]}")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    for name in SM.PLAN_CASES:
        for prec in ("fp64", "fp32"):
            a, b, want, prod = _case(name, prec)
            key = f"{name}/{prec}/"
            assert np.array_equal(got[key + "rp"], want.rp) and np.array_equal(got[key + "ci"], want.ci), (name, prec)
            assert got[key + "va"].tobytes() == want.va.tobytes(), (name, prec)          # the model's bytes are the default plan's (test_export_and_info)
            info = got[key + "info"]
            assert tuple(info[:2]) == limits and tuple(info[2:6]) == SM.row_classes(prod, *limits), (name, prec, info)
            assert (info[6], info[7]) == (len(want.ci), prod.sum())
            if limits == (1, 1):
                assert info[3] == info[4] == 0 and info[5] == (prod > 0).sum()          # every non-empty row a spill row
            default = SM.row_classes(prod)
            assert tuple(info[2:6]) != default, (name, prec)          # the plan did move


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_reproducible_and_independent_of_alignment(prec):
    for name in ("laplacian-24", "duplicates", "dense-row"):
        a, b, want, _ = _case(name, prec)
        for ashift, bshift in ((0, 0), (0, 0), (1, 0), (0, 1), (3, 1)):
            g = _from_device(a, b, ashift, bshift)
            try:
                _same(g, want, (name, prec, ashift, bshift))
            finally:
                g.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["laplacian-24", "duplicates"])
def test_numeric_rerun(name, prec):
    dtype = G.dtype_of(prec)
    a, b, want, _ = _case(name, prec)
    a2 = SM.Csr(a.nrows, a.ncols, a.rp, a.ci, SM._values(len(a.ci), 101, dtype))
    b2 = SM.Csr(b.nrows, b.ncols, b.rp, b.ci, SM._values(len(b.ci), 102, dtype))
    want2 = SM.spgemm(a2, b2)
    fresh = capi.SpGemm.create(_tuple(a2), _tuple(b2))
    _same(fresh, want2, (name, prec, "fresh"))
    fresh.close()
    g = capi.SpGemm.create(_tuple(a), _tuple(b))
    try:
        rp0, ci0, _ = g.export()
        for av, bv, w, shift in ((a2.va, b2.va, want2, 0), (a.va, b.va, want, 1), (a2.va, b2.va, want2, 1)):
            at, bt = G.put(av, dtype, shift), G.put(bv, dtype, shift)
            torch.cuda.synchronize()
            g.numeric(at.data_ptr(), bt.data_ptr())
            torch.cuda.synchronize()
            rp, ci, va = g.export()
            assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and va.tobytes() == w.va.tobytes(), (name, prec, shift)
        L = capi.lib()
        assert L.cvr_spgemm_numeric_device(g._g, None, bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_spgemm_numeric_device(g._g, at.data_ptr(), None, None) == capi.ERR_INVALID
        _same(g, want2, (name, prec, "behind the errors"))
    finally:
        g.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_non_finite_values(prec):
    a, b, _, _ = _case("duplicates", prec)
    va = a.va.copy()
    va[3], va[11] = np.inf, np.nan
    a = SM.Csr(a.nrows, a.ncols, a.rp, a.ci, va)
    want = SM.spgemm(a, b)
    assert np.isnan(want.va).any() and np.isinf(want.va).any()
    for g in (capi.SpGemm.create(_tuple(a), _tuple(b)), _from_device(a, b)):
        rp, ci, got = g.export()
        g.close()
        assert np.array_equal(rp, want.rp) and np.array_equal(ci, want.ci)
        assert np.array_equal(np.isnan(got), np.isnan(want.va)) and np.array_equal(np.isinf(got), np.isinf(want.va))
        keep = ~np.isnan(want.va)          # the infinities with their signs, every finite entry byte for byte; NaN payloads are not compared
        assert got[keep].tobytes() == want.va[keep].tobytes()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["laplacian-24", "a-empty-rows"])
def test_the_view_feeds_the_library(name, prec):
    dtype = G.dtype_of(prec)
    a, b, want, _ = _case(name, prec)
    g = capi.SpGemm.create(_tuple(a), _tuple(b))
    Cm = A = B = None
    try:
        m, n, rp, ci, va = g.csr_device()
        Cm = cvr_amd.CvrMatrix.from_device(m, n, rp, ci, va, is_f32=dtype == np.float32)
        A, B = cvr_amd.CvrMatrix(*_tuple(a)), cvr_amd.CvrMatrix(*_tuple(b))
        x = SM._values(b.ncols, 55, dtype)
        cx = Cm.spmv(x)[0].astype(np.float64)
        abx = A.spmv(B.spmv(x)[0])[0].astype(np.float64)
        ra, rb = int(np.diff(a.rp).max()), int(np.diff(b.rp).max())
        scale = np.abs(a.dense()) @ (np.abs(b.dense()) @ np.abs(x.astype(np.float64)))
        bound = (ra + rb + 2) * float(np.finfo(dtype).eps) * scale
        assert (np.abs(cx - abx) <= bound).all(), (name, prec, (np.abs(cx - abx) / np.maximum(bound, 1e-300)).max())
        assert np.abs(cx).max() > 0
    finally:
        for h in (Cm, A, B):
            if h is not None:
                h.close()
        g.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_galerkin_product_against_the_amg_setup(prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = synth.laplacian_2d(24)
    va = np.asarray(va).astype(dtype)
    a = SM.Csr(n, n, rp, ci, va)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg(A, rp, ci, va)
    try:
        assert P.amg_info().levels >= 2
        l0, l1 = P.amg_export_level(0), P.amg_export_level(1)
    finally:
        P.close()
        A.close()
    agg, nc = l0.agg, l1.n
    p = SM.Csr(n, nc, np.arange(n + 1), agg, np.ones(n, dtype=dtype))
    order = np.argsort(agg, kind="stable")
    pt = SM.Csr(nc, n, np.r_[0, np.cumsum(np.bincount(agg, minlength=nc))], order, np.ones(n, dtype=dtype))
    ap = capi.SpGemm.create(_tuple(a), _tuple(p))
    dpt = OnDevice(pt)
    ptap = capi.SpGemm.from_device(dpt.tuple(), ap.csr_device(), is_f32=dtype == np.float32)          # the product's view is the next product's B
    try:
        crp, cci, cva = ptap.export()
    finally:
        ptap.close()
        ap.close()
    assert np.array_equal(crp, l1.rp) and np.array_equal(cci, l1.ci)
    # entry (I, J): t terms a_ij with agg[i] = I, agg[j] = J; the two summation orders differ by at most (t + 1) eps sum |a_ij|
    rows = np.repeat(np.arange(n), np.diff(rp))
    key = agg[rows].astype(np.int64) * nc + agg[ci]
    ckey = np.repeat(np.arange(nc), np.diff(crp)).astype(np.int64) * nc + cci
    pos = np.searchsorted(ckey, key)
    assert np.array_equal(ckey[pos], key)
    t = np.bincount(pos, minlength=len(cci))
    absum = np.bincount(pos, weights=np.abs(va.astype(np.float64)), minlength=len(cci))
    assert (np.abs(cva.astype(np.float64) - l1.va.astype(np.float64)) <= (t + 1) * float(np.finfo(dtype).eps) * absum).all()


def _views(a, b, dev=False):
    if dev:
        da, db = OnDevice(a), OnDevice(b)
        ta, tb = da.tuple(), db.tuple()
        va = capi.CsrView(*ta, int(a.va.dtype == np.float32), 1)
        vb = capi.CsrView(*tb, int(b.va.dtype == np.float32), 1)
        va._keep = vb._keep = (da, db)
        return va, vb
    keep = [np.ascontiguousarray(x) for x in (a.rp, a.ci, a.va, b.rp, b.ci, b.va)]
    va = capi.CsrView(a.nrows, a.ncols, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, int(a.va.dtype == np.float32), 0)
    vb = capi.CsrView(b.nrows, b.ncols, keep[3].ctypes.data, keep[4].ctypes.data, keep[5].ctypes.data, int(b.va.dtype == np.float32), 0)
    va._keep = vb._keep = keep
    return va, vb


def _create(va, vb):
    g = C.c_void_p()
    rc = capi.lib().cvr_spgemm_create(C.byref(g), C.byref(va), C.byref(vb), 0, None)
    assert (rc == 0) == bool(g.value)
    if g.value:
        capi.lib().cvr_spgemm_destroy(g)
    return rc, capi.last_error()


def test_every_error_return():
    L = capi.lib()
    aa = SM.Csr(2, 3, [0, 1, 2], [0, 2], np.ones(2))
    ok = SM.Csr(3, 5, [0, 1, 2, 3], [0, 1, 2], np.ones(3))
    for dev in (False, True):
        # a row of B out of order, and one with a duplicate: the lowest offending row is named
        for cols, row in (([0, 2, 1, 3, 4], 1), ([0, 1, 2, 4, 4], 2), ([1, 0, 2, 4, 4], 1)):
            rp = [0, 1, 3, 5] if cols[0] == 0 else [0, 0, 2, 5]
            rc, msg = _create(*_views(aa, SM.Csr(3, 5, rp, cols, np.ones(5)), dev))
            assert rc == capi.ERR_INVALID and f"B row {row}:" in msg and "strictly increasing" in msg, (dev, msg)
        rc, msg = _create(*_views(aa, ok.astype(np.float32), dev))
        assert rc == capi.ERR_INVALID and "is_f32" in msg
        rc, msg = _create(*_views(SM.Csr(2, 4, aa.rp, aa.ci, aa.va), ok, dev))
        assert rc == capi.ERR_INVALID and "inner dimensions" in msg
        rc, msg = _create(*_views(aa, SM.Csr(3, 2 ** 31 - 1, ok.rp, ok.ci, ok.va), dev))
        assert rc == capi.ERR_INVALID and "2^31 - 1" in msg
        for broken_a, broken_b in ((SM.Csr(2, 3, [0, 2, 1], [0, 2], np.ones(2)), ok), (SM.Csr(2, 3, [0, 1, 2], [0, 3], np.ones(2)), ok), (SM.Csr(2, 3, [0, 1, 2], [0, -1], np.ones(2)), ok),
                                   (aa, SM.Csr(3, 5, [0, 1, 2, 3], [0, 5, 2], np.ones(3))), (aa, SM.Csr(3, 5, [0, 2, 1, 3], [0, 1, 2], np.ones(3)))):
            rc, msg = _create(*_views(broken_a, broken_b, dev))
            assert rc == capi.ERR_INVALID, (dev, msg)
        rc, msg = _create(*_views(aa, ok, dev))          # the library still works behind the errors
        assert rc == 0
    va, vb = _views(aa, ok)
    vb.arrays_on_device = 1          # one view of host arrays and one of device arrays
    assert _create(va, vb)[0] == capi.ERR_INVALID
    g = C.c_void_p()
    assert L.cvr_spgemm_create(None, C.byref(va), C.byref(va), 0, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_create(C.byref(g), None, C.byref(va), 0, None) == capi.ERR_INVALID and L.cvr_spgemm_create(C.byref(g), C.byref(va), None, 0, None) == capi.ERR_INVALID
    vb.arrays_on_device = 0
    assert L.cvr_spgemm_create(C.byref(g), C.byref(va), C.byref(vb), 99, None) == capi.ERR_NO_DEVICE and not g.value
    assert L.cvr_spgemm_destroy(None) == 0
    info, view = capi.SpGemmInfo(), capi.CsrView()
    assert L.cvr_spgemm_get_info(None, C.byref(info)) == capi.ERR_INVALID and L.cvr_spgemm_export(None, None, None, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_csr_device(None, C.byref(view)) == capi.ERR_INVALID and L.cvr_spgemm_numeric_device(None, None, None, None) == capi.ERR_INVALID
    obj = capi.SpGemm.create(_tuple(aa), _tuple(ok))
    assert L.cvr_spgemm_get_info(obj._g, None) == capi.ERR_INVALID and L.cvr_spgemm_csr_device(obj._g, None) == capi.ERR_INVALID
    assert L.cvr_spgemm_export(obj._g, None, None, None) == 0          # each pointer may be NULL
    obj.close()
