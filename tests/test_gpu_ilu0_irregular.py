"""GPU (MI355X): cvr_precond_ilu0 where tests/test_gpu_ilu0.py's regular matrices do not reach -- against tests/ilu_model.py, byte for byte.

The cases are ilu_model.IRREGULAR (rows of unrelated lengths, level-0 rows scattered, near and far columns); tests/test_ilu_model_host.py holds them
to the conditions that make these tests mean something and shows which mutant of the sweeps and of the factorisation each tells apart.
  * every lane count: the two dense cases (rows of more than 64 entries in each triangle), the two-level wide matrix and irr-spd-700 built under
    CVR_DEBUG=ilu_lanes=1 .. 64 and ilu_wide=1, the default, 1000000: lanes_per_row, one export for all of them, the apply against the model with that
    G (in fp64 the seven G have seven different results); ilu_lanes=3, 0, 128 leave the default
  * PCG on irr-spd-700, PBiCGSTAB and PGMRES(5) on irr-nonsym-700 step by step against the model: the default G (4), ilu_lanes=16, and the threshold
    from the case's own widths (the gated sweeps through a mixed plan, GMRES's fp64 right-hand side among them)
  * irr-nonsym-2500 (merged, wide, merged by default) from arrays on the device
  * two bad pivots met out of row order: the lowest row is named, whichever level it has"""
import numpy as np
import pytest
import torch

import cvr_amd
import ilu_model as IM
import krylov_model as KM
import pkrylov_gpu as G
import test_gpu_ilu0 as B
from cvr_amd import capi

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16, 32, 64]


def _case(name, prec):
    """(n, rp, ci, va, the model's factors)"""
    dtype = G.dtype_of(prec)
    if name == "wide":
        n, _, rp, ci, va = IM.wide_matrix(dtype)
        return n, rp, ci, va, IM.factor(rp, ci, va, dtype)[0]
    return IM.irregular_case(name, prec)[:5]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["irr-dense-spd-320", "irr-dense-nonsym-320", "wide", "irr-spd-700"])
def test_every_lane_count(name, prec):
    dtype = G.dtype_of(prec)
    n, rp, ci, va, f = _case(name, prec)
    r = KM.inputs(n, dtype)[0]
    default = IM.default_lanes(n, int(rp[-1]))
    results = set()
    for g in LANES:
        want = IM.apply(rp, ci, f, r, g, dtype)
        results.add(want.tobytes())
        for wide in B.WIDES:
            P = B._build(rp, ci, va, wide, g)
            try:
                i = P.ilu0_info()
                assert (i.lanes_per_row, i.wide_threshold) == (g, IM.DEFAULT_WIDE if wide is None else wide), (name, g, wide)
                got_f = P.ilu0_export()
                assert got_f.tobytes() == f.tobytes(), (name, prec, g, wide, B._first_difference(got_f, f))          # the factors do not depend on G
                got = B._apply(P, r, dtype)
                assert got.tobytes() == want.tobytes(), (name, prec, g, wide, B._first_difference(got, want))
            finally:
                P.close()
    if prec == "fp64" and name.startswith("irr-dense"):
        assert len(results) == len(LANES)          # byte equality tells the seven lane schedules apart
    for bad in (3, 0, 128):          # not a power of two in 1 .. 64: the default stays
        P = B._build(rp, ci, va, None, bad)
        try:
            assert P.ilu0_info().lanes_per_row == default, (name, bad)
        finally:
            P.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", ["pcg", "bicgstab", "gmres5"])
def test_solvers_step_by_step_on_the_irregular_patterns(which, prec):
    dtype = G.dtype_of(prec)
    name = "irr-spd-700" if which == "pcg" else "irr-nonsym-700"
    n, rp, ci, va, f = IM.irregular_case(name, prec)[:5]
    w = IM.irregular_case(name, prec)[9]
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = G.Dev(A)
        kind = B._solver(which)
        b, x0, _ = KM.inputs(n, dtype)
        for wide, lanes in ((None, None), (None, 16), (w, None)):
            P = B._build(rp, ci, va, wide, lanes)
            try:
                i = P.ilu0_info()
                assert i.lanes_per_row == (4 if lanes is None else lanes)
                if wide is not None:
                    assert min(i.launches_lower, i.launches_upper) >= 6 and (i.launches_lower, i.launches_upper) != (i.levels_lower, i.levels_upper)
                assert P.ilu0_export().tobytes() == f.tobytes()
                ilu = IM.Ilu(rp, ci, f, i.lanes_per_row, dtype)
                tr = B._model(which, dev.product, dtype, ilu).run(b, x0, rtol=0.0, max_iters=4)
                for k in range(5):
                    if k >= len(tr.steps) and not tr.last.terminal:
                        break
                    for every in (1, 0):
                        got, res = kind.solve(A, P, b, x0, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, which, prec, "wide", wide, "lanes", lanes, "max_iters", k, "check_every", every))
                        if got.status == capi.CG_MAX_ITERS:
                            assert res.spmv_count == kind.spmvs(k), (which, k, every, res.spmv_count)
            finally:
                P.close()
    finally:
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_arrays_on_the_device_through_a_mixed_plan(prec):
    dtype = G.dtype_of(prec)
    n, rp, ci, va, f = IM.irregular_case("irr-nonsym-2500", prec)[:5]
    rt, ct, vt = torch.from_numpy(rp.copy()).cuda(), torch.from_numpy(ci.copy()).cuda(), torch.from_numpy(va.copy()).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.ilu0_from_device(n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), is_f32=dtype == np.float32)
    Q = capi.Precond.ilu0(rp, ci, va)
    try:
        for X in (P, Q):
            i = X.ilu0_info()
            assert i.launches_lower >= 3 and i.launches_upper >= 3 and i.max_level_width >= IM.DEFAULT_WIDE          # merged, wide, merged
        assert P.ilu0_export().tobytes() == Q.ilu0_export().tobytes() == f.tobytes()
        r = KM.inputs(n, dtype)[0]
        del rt, ct, vt          # the object keeps nothing of the caller's
        want = IM.apply(rp, ci, f, r, P.ilu0_info().lanes_per_row, dtype)
        assert B._apply(P, r, dtype).tobytes() == B._apply(Q, r, dtype).tobytes() == want.tobytes()
    finally:
        P.close()
        Q.close()


def _two_bad_pivots(zero_row, chain):
    """12 rows, the identity but for: row `zero_row`, diagonal only, whose diagonal is 0 (level 0); and rows chain, chain + 1, chain + 2 with
    a_(c+1,c) = 0.5, a_(c+1,c+1) = 1, a_(c+1,c+2) = 2, a_(c+2,c+1) = 1, a_(c+2,c+2) = 2: row chain + 2 has level 2 and its pivot is 2 - (1 / 1) * 2 = 0
    exactly, in fp64 and in fp32"""
    n, c = 12, chain
    rows = {i: {i: 1.0} for i in range(n)}
    rows[zero_row] = {zero_row: 0.0}
    rows[c + 1] = {c: 0.5, c + 1: 1.0, c + 2: 2.0}
    rows[c + 2] = {c + 1: 1.0, c + 2: 2.0}
    rp = np.cumsum([0] + [len(rows[i]) for i in range(n)]).astype(np.int64)
    ci = np.array([j for i in range(n) for j in sorted(rows[i])], dtype=np.int32)
    va = np.array([rows[i][j] for i in range(n) for j in sorted(rows[i])])
    return n, rp, ci, va


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("zero_row, chain, lowest", [(9, 3, 5), (2, 6, 2)])
def test_the_lowest_bad_pivot_wins(zero_row, chain, lowest, prec):
    """the bad rows are met out of row order ((9, 3): row 9 at level 0, row 5 at level 2; (2, 6): row 2 at level 0, row 8 at level 2): the row named is
    the lower one in both, under a launch per level, the default and one merged launch"""
    dtype = G.dtype_of(prec)
    n, rp, ci, va = _two_bad_pivots(zero_row, chain)
    va = va.astype(dtype)
    lo = IM.levels(rp, ci)[0]
    assert (lo[zero_row], lo[chain + 2]) == (0, 2)
    assert IM.factor(rp, ci, va, dtype)[1] == lowest
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for wide in B.WIDES:
        for _ in range(3):
            with pytest.raises(capi.CvrError) as e:
                B._build(rp, ci, va, wide)
            assert e.value.code == capi.ERR_STATE and f"row {lowest} " in str(e.value) + " " and "pivot" in str(e.value), (wide, str(e.value))
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 16 << 20          # nothing of the nine failed builds is kept
    good = va.copy()
    good[IM.diagonal_positions(rp, ci)[[zero_row, chain + 2]]] = 3.0          # ... and the next build succeeds
    P = capi.Precond.ilu0(rp, ci, good)
    try:
        assert P.ilu0_export().tobytes() == IM.factor(rp, ci, good, dtype)[0].tobytes()
    finally:
        P.close()
