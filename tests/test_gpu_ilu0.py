"""GPU (MI355X): the ILU(0) preconditioner -- cvr_precond_ilu0, cvr_precond_ilu0_info, cvr_precond_ilu0_export, and cvr_precond_apply_device /
cvr_pcg / cvr_pbicgstab / cvr_pgmres with an object of this kind, all through the ABI, against tests/ilu_model.py.

  * the factors (export) and the apply byte for byte against the model, fp64 and fp32: banded "spd" and "nonsym" at n = 1, 2, 63, 64, 65, 1025 (n levels
    of one row: the merged path), the Laplacian at m = 3, 24, 40, the two-level wide matrix (n = 4097) and its transpose (wide levels in L and in U),
    the five irregular cases of ilu_model.IRREGULAR (default G = 4, 64, 32, 2; tests/test_ilu_model_host.py holds them to their conditions), those
    also under the threshold taken from their own level widths (merged runs and wide levels in turn; irr-nonsym-2500 alternates by default);
    r and z off the 16-byte grid one at a time; every apply repeated.  tests/test_gpu_ilu0_irregular.py: every lane count, the solvers on the
    irregular patterns, the lowest bad pivot
  * every object built under CVR_DEBUG=ilu_wide=1, the default and ilu_wide=1000000: the same export and apply, launches_* by the model's plan
  * PCG, PBiCGSTAB and PGMRES (restart 5 and 30) step by step against the model: max_iters 0 .. 4 at rtol 0, a solve to 1e-8 on the 24 x 24 Laplacian;
    check_every 1, 3 and the default give the same bits; spmv_count by the block-Jacobi formulas; the host twins
  * banded ILU(0)-PCG stops after 1 iteration (no fill: the factor is exact); Laplacian-40 PCG needs at most half of cvr_cg's iterations
  * every error return, the entry points that decline this kind, the stop states"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cvr_amd
import ilu_model as IM
import krylov_model as KM
import pkrylov_gpu as G
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

WIDES = [1, None, 1000000]          # CVR_DEBUG=ilu_wide=<w> when the object is built; None: the default


def _matrix(name, dtype):
    kind, _, size = name.partition("-")
    if kind in ("spd", "nonsym"):
        return KM.banded(kind, int(size), dtype)
    if kind == "laplacian":
        return synth.laplacian_2d(int(size), dtype)
    if kind == "wide":
        return IM.wide_matrix(dtype)
    if kind == "irr":
        n, rp, ci, va = IM.irregular_case(name, "fp64" if dtype == np.float64 else "fp32")[:4]
        return n, n, rp, ci, va
    assert kind == "wideT", name
    n, _, rp, ci, va = IM.wide_matrix(dtype)
    return IM.transpose(n, rp, ci, va)


MATRICES = [f"{k}-{n}" for k in ("spd", "nonsym") for n in (1, 2, 63, 64, 65, 1025)] + ["laplacian-3", "laplacian-24", "laplacian-40", "wide", "wideT"] + list(IM.IRREGULAR)


def _thresholds(name, rp, ci):
    """WIDES, and for the irregular cases with narrow levels the threshold from their own widths: merged runs and wide levels in turn"""
    return WIDES + ([IM.width_threshold(rp, ci)] if name.startswith("irr-") and name != "irr-nonsym-2500" else [])


def _build(rp, ci, va, wide=None, lanes=None):
    """Precond.ilu0 with CVR_DEBUG=ilu_wide=<wide>,ilu_lanes=<lanes> in the environment while the object is built (the switches are read there)"""
    knobs = ([f"ilu_wide={wide}"] if wide is not None else []) + ([f"ilu_lanes={lanes}"] if lanes is not None else [])
    old = os.environ.get("CVR_DEBUG")
    try:
        if knobs:
            os.environ["CVR_DEBUG"] = ",".join(knobs)
        else:
            os.environ.pop("CVR_DEBUG", None)
        return capi.Precond.ilu0(rp, ci, va)
    finally:
        if old is None:
            os.environ.pop("CVR_DEBUG", None)
        else:
            os.environ["CVR_DEBUG"] = old


def _apply(P, r, dtype, rshift=0, zshift=0):
    rt = G.put(r, dtype, rshift)
    zt = G.put(np.full(len(r), np.nan), dtype, zshift)
    torch.cuda.synchronize()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    return zt.cpu().numpy()


def _first_difference(a, b):
    u = f"u{a.itemsize}"
    d = np.flatnonzero(a.view(u) != b.view(u))
    return (int(d[0]), a[d[0]], b[d[0]], len(d)) if len(d) else None


# ---- the factors, the apply, the plan ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", MATRICES)
def test_factors_and_apply_against_the_model_for_every_plan(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = _matrix(name, dtype)
    nnz = int(rp[-1])
    if name.startswith("irr-"):          # (factored once for all the tests that use the case)
        f, lo, up, nlo, nup = IM.irregular_case(name, prec)[4:9]
    else:
        f, bad = IM.factor(rp, ci, va, dtype)
        assert bad is None
        lo, up, nlo, nup = IM.levels(rp, ci)
    Gl = IM.default_lanes(n, nnz)
    r = KM.inputs(n, dtype)[0]
    want = IM.apply(rp, ci, f, r, Gl, dtype)
    assert np.isfinite(want).all()
    for wide in _thresholds(name, rp, ci):
        P = _build(rp, ci, va, wide)
        try:
            w = IM.DEFAULT_WIDE if wide is None else wide
            i = P.ilu0_info()
            plan_lo, plan_up = IM.plan(lo, nlo, w), IM.plan(up, nup, w)
            assert (i.n, i.nnz, i.levels_lower, i.levels_upper, i.lanes_per_row, i.wide_threshold, i.is_f32) == (n, nnz, nlo, nup, Gl, w, int(dtype == np.float32)), (name, wide)
            assert (i.launches_lower, i.launches_upper) == (len(plan_lo), len(plan_up)), (name, wide, i.launches_lower, i.launches_upper)
            assert i.max_level_width == max(IM.widths(lo, nlo).max(), IM.widths(up, nup).max()) and not any(i.reserved)
            if wide == 1:
                assert (i.launches_lower, i.launches_upper) == (nlo, nup)
            if wide == 1000000:
                assert (i.launches_lower, i.launches_upper) == (1, 1)
            pi = P.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks, pi.device) == (n, 0, int(dtype == np.float32), 0, 0, 0)
            got_f = P.ilu0_export()
            assert got_f.dtype == dtype and got_f.tobytes() == f.tobytes(), (name, prec, wide, _first_difference(got_f, f))
            for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind three applies)
                got = _apply(P, r, dtype, rshift, zshift)
                assert got.tobytes() == want.tobytes(), (name, prec, wide, rshift, zshift, _first_difference(got, want))
        finally:
            P.close()


def test_the_wide_matrix_takes_the_wide_kernels_by_default():
    """... and the banded ones the merged kernel: the two paths are both run by the default threshold"""
    n, _, rp, ci, va = IM.wide_matrix(np.float64)
    P = _build(rp, ci, va)
    i = P.ilu0_info()
    assert (i.levels_lower, i.launches_lower, i.levels_upper, i.launches_upper, i.max_level_width, i.wide_threshold) == (2, 2, 1, 1, 4097, IM.DEFAULT_WIDE)
    P.close()
    _, _, rp, ci, va = KM.banded("spd", 1025, np.float64)
    P = _build(rp, ci, va)
    i = P.ilu0_info()
    assert (i.levels_lower, i.launches_lower, i.levels_upper, i.launches_upper, i.max_level_width) == (1025, 1, 1025, 1, 1)
    P.close()


def test_arrays_on_the_device():
    n, _, rp, ci, va = synth.laplacian_2d(24)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.ilu0_from_device(n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr())
    Q = capi.Precond.ilu0(rp, ci, va)
    try:
        assert P.ilu0_export().tobytes() == Q.ilu0_export().tobytes() == IM.factor(rp, ci, va, np.float64)[0].tobytes()
        r = KM.inputs(n, np.float64)[0]
        del rt, ct, vt          # the object keeps nothing of the caller's
        assert _apply(P, r, np.float64).tobytes() == _apply(Q, r, np.float64).tobytes()
    finally:
        P.close()
        Q.close()
    E = capi.Precond.ilu0(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))          # n = 0 is valid
    assert (E.ilu0_info().n, E.ilu0_info().launches_lower, len(E.ilu0_export())) == (0, 0, 0)
    E.close()


# ---- the solvers, step by step ----
class _Pcg:
    name, restart = "pcg", None

    def solve(self, H, P, b, x0=None, shift=0, **kw):
        bt = G.put(b, H.dtype, shift)
        xt = G.put(np.zeros(H.nrows) if x0 is None else x0, H.dtype, shift)
        torch.cuda.synchronize()
        res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw) if P is not None else H.cg(bt.data_ptr(), xt.data_ptr(), **kw)
        torch.cuda.synchronize()
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res

    def solve_host(self, H, P, b, x0=None, **kw):
        x, r = H.pcg_host(P, b, x0=x0, **kw)
        return KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), r

    def spmvs(self, steps):
        return 1 + steps


def _solver(which):
    return _Pcg() if which == "pcg" else G.Kind(None if which == "bicgstab" else int(which[5:]))


def _model(which, product, dtype, ilu):
    if which == "pcg":
        return IM.IluPcg(product, dtype, ilu)
    if which == "bicgstab":
        return IM.IluBicgstab(product, dtype, ilu)
    return IM.IluGmres(product, dtype, ilu, restart=int(which[5:]))


SOLVERS = ["pcg", "bicgstab", "gmres5", "gmres30"]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", SOLVERS)
@pytest.mark.parametrize("name", ["banded-1025", "laplacian-24"])
def test_solvers_step_by_step_against_the_model(name, which, prec):
    dtype = G.dtype_of(prec)
    if name == "banded-1025":
        n, _, rp, ci, va = KM.banded("spd" if which == "pcg" else "nonsym", 1025, dtype)
    else:
        n, _, rp, ci, va = synth.laplacian_2d(24, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        dev = G.Dev(A)
        kind = _solver(which)
        ilu = IM.Ilu(rp, ci, P.ilu0_export(), P.ilu0_info().lanes_per_row, dtype)
        b, x0, _ = KM.inputs(n, dtype)
        for start_name, start in (("zero", None), ("random", x0)):
            tr = _model(which, dev.product, dtype, ilu).run(b, start, rtol=0.0, max_iters=4)
            for k in range(5):
                if k >= len(tr.steps) and not tr.last.terminal:
                    break
                for every in (1, 3, 0):
                    for shift in (0, 1):
                        got, res = kind.solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, which, prec, start_name, "max_iters", k, "check_every", every, "shift", shift))
                        if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop
                            assert res.spmv_count == kind.spmvs(k), (which, k, every, res.spmv_count)
        got, _ = kind.solve_host(A, P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        G.same(got, tr.at(4), (name, which, prec, "host"))
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("which", SOLVERS)
def test_laplacian_24_to_1e_8(which):
    """the model's terminal entry whatever check_every is; spmv_count by the formula with the steps enqueued (whole batches up to the stop)"""
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        kind = _solver(which)
        ilu = IM.Ilu(rp, ci, P.ilu0_export(), P.ilu0_info().lanes_per_row, np.float64)
        b = KM.inputs(n, np.float64)[0]
        last = _model(which, G.Dev(A).product, np.float64, ilu).run(b, None, rtol=1e-8, max_iters=200).last
        assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < 60, last
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = kind.solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, (which, "check_every", every))
            assert res.spmv_count == kind.spmvs(enqueued), (which, every, res.spmv_count, enqueued)
        print(f"{which}: {last.iterations} steps on laplacian_2d(24)")
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_banded_pcg_stops_after_one_iteration(prec):
    """no fill: L U = A up to rounding, so M^-1 A = I and the first step solves the system"""
    dtype = G.dtype_of(prec)
    n = 1025
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        b = KM.inputs(n, dtype)[0]
        got, res = _Pcg().solve(A, P, b, rtol=G.RTOL[dtype], max_iters=50)
        assert (res.status, res.iterations) == (capi.CG_CONVERGED, 1), (res.status, res.iterations, res.residual_norm / res.b_norm)
    finally:
        P.close()
        A.close()


def test_laplacian_40_pcg_needs_at_most_half_of_cgs_iterations():
    n, _, rp, ci, va = synth.laplacian_2d(40)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        b = KM.inputs(n, np.float64)[0]
        got, res = _Pcg().solve(A, P, b, rtol=1e-8, max_iters=400)
        plain, pres = _Pcg().solve(A, None, b, rtol=1e-8, max_iters=400)
        print(f"laplacian_2d(40): ILU(0)-PCG {res.iterations} steps, cvr_cg {pres.iterations}")
        assert res.status == capi.CG_CONVERGED and pres.status == capi.CG_CONVERGED
        assert 2 * res.iterations <= pres.iterations
    finally:
        P.close()
        A.close()


# ---- errors ----
def _raw_build(n, ncols, rp, ci, va, device=0):
    rp, ci, va = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=np.float64)
    p = C.c_void_p()
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    rc = capi.lib().cvr_precond_ilu0(C.byref(p), C.byref(view), device, None)
    assert rc != 0 and not p.value
    return rc, capi.last_error()


def test_invalid_views():
    rc, msg = _raw_build(3, 4, [0, 1, 2, 3], [0, 1, 2], [1, 1, 1])
    assert rc == capi.ERR_INVALID and "square" in msg
    rc, msg = _raw_build(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3], np.ones(6))
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg = _raw_build(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 2, 3], np.ones(6))
    assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
    rc, msg = _raw_build(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3], np.ones(5))
    assert rc == capi.ERR_INVALID and "row 2" in msg and "diagonal" in msg
    rc, msg = _raw_build(2, 2, [0, 1, 2], [0, 5], np.ones(2))          # cvr_create's checks hold
    assert rc == capi.ERR_INVALID
    rc, msg = _raw_build(2, 2, [0, 1, 2], [0, 1], np.ones(2), device=cvr_amd.device_count())
    assert rc == capi.ERR_NO_DEVICE
    L = capi.lib()
    assert L.cvr_precond_ilu0(None, None, 0, None) == capi.ERR_INVALID
    # the same row named when the arrays lie on the device
    rp, ci, va = np.array([0, 1, 3, 5, 6], dtype=np.int64), np.array([0, 0, 1, 2, 1, 3], dtype=np.int32), np.ones(6)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    with pytest.raises(capi.CvrError) as e:
        capi.Precond.ilu0_from_device(4, rt.data_ptr(), ct.data_ptr(), vt.data_ptr())
    assert e.value.code == capi.ERR_INVALID and "row 2" in str(e.value)


def test_bad_pivots_name_the_row_and_leak_nothing():
    rc, msg = _raw_build(3, 3, [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], [2, 1, 1, 0.5, 1, 1, 3])          # a_11 = 0.5 - (1 / 2) * 1
    assert rc == capi.ERR_STATE and "row 1" in msg and "pivot" in msg
    n = 20000
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    d = IM.diagonal_positions(rp, ci)
    nan = va.copy()
    nan[d[12345]] = np.nan
    zero = va.copy()
    zero[d[0]] = 0.0          # row 0: a zero pivot at the very start; the rows that divide by it are not finite, row 0 is the lowest
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(25):
        rc, msg = _raw_build(n, n, rp, ci, nan)
        assert rc == capi.ERR_STATE and "row 12345 " in msg + " ", msg
        rc, msg = _raw_build(n, n, rp, ci, zero)
        assert rc == capi.ERR_STATE and "row 0 " in msg + " ", msg
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    assert lost < 16 << 20, lost          # 50 failed builds of about 3 MB each would have kept 150 MB
    P = capi.Precond.ilu0(rp, ci, va)          # ... and the next build succeeds
    assert P.ilu0_info().n == n and np.isfinite(P.ilu0_export()).all()
    P.close()


def test_mismatches_of_the_pair_and_minv_beside_the_object():
    n = 250
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0(rp, ci, va)
    b = synth.x_rand(n)
    try:
        _, _, rp2, ci2, va2 = KM.banded("nonsym", n + 1, np.float64)
        Q = capi.Precond.ilu0(rp2, ci2, va2)
        F = capi.Precond.ilu0(rp, ci, va.astype(np.float32))
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        capi.lib().cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        for which in SOLVERS:
            kind = _solver(which)
            with pytest.raises(capi.CvrError) as e:
                kind.solve(A, Q, b, rtol=1e-8, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value), which
            with pytest.raises(capi.CvrError) as e:
                kind.solve(A, F, b, rtol=1e-8, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "type" in str(e.value), which
            if which == "pcg":
                rc = capi.lib().cvr_pcg_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None)
            else:
                rc = kind.raw_device_call(A._h, P._p, bt.data_ptr(), xt.data_ptr(), opt, res)
            assert rc == capi.ERR_INVALID and "minv_dev" in capi.last_error(), which
        Q.close()
        F.close()
        # r == z and null arguments of the apply, of the info and of the export
        L = capi.lib()
        assert L.cvr_precond_apply_device(P._p, bt.data_ptr(), bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_apply_device(P._p, None, bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_ilu0_info(P._p, None) == capi.ERR_INVALID and L.cvr_precond_ilu0_export(P._p, None) == capi.ERR_INVALID
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        assert L.cvr_precond_ilu0_info(J._p, C.byref(capi.Ilu0Info())) == capi.ERR_INVALID and "kind" in capi.last_error()
        assert L.cvr_precond_ilu0_export(J._p, np.zeros(len(va)).ctypes.data) == capi.ERR_INVALID and "kind" in capi.last_error()
        J.close()
        assert L.cvr_precond_chebyshev_info(P._p, C.byref(capi.ChebyshevInfo())) == capi.ERR_INVALID and "ILU(0)" in capi.last_error()
    finally:
        P.close()
        A.close()


def test_device_mismatch():
    if cvr_amd.device_count() < 2:
        pytest.skip("one device")
    n = 250
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0(rp, ci, va, device=1)
    try:
        for which in SOLVERS:
            with pytest.raises(capi.CvrError) as e:
                _solver(which).solve(A, P, synth.x_rand(n), rtol=1e-8, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "device" in str(e.value)
    finally:
        P.close()
        A.close()
        torch.cuda.set_device(0)


def test_entry_points_that_decline_this_kind():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0(rp, ci, va)
    try:
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind 2" in capi.last_error() and "ILU(0)" in capi.last_error(), (name, capi.last_error())

        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), "apply_multi")
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), "pcg_multi_device")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), "pcg_multi")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran
        assert L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 9, None) == capi.ERR_INVALID          # behind their other checks
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("which", SOLVERS)
def test_stop_states(which):
    n = 1000
    kind = _solver(which)
    _, _, rp, ci, va = KM.banded("spd" if which == "pcg" else "nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0(rp, ci, va)
    try:
        b, x0, _ = KM.inputs(n, np.float64)
        got, res = kind.solve(A, P, b, x0, rtol=1e-10, max_iters=0)          # max_iters = 0: the initial residual alone
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1)
        got, res = kind.solve(A, P, np.zeros(n), x0, rtol=1e-10, max_iters=50)          # b == 0: x = 0 whatever the start
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        bn = b.copy()
        bn[n // 2] = np.nan          # a NaN in b: breakdown with 0 iterations, x untouched
        for every in (1, 0):
            got, res = kind.solve(A, P, bn, x0, rtol=1e-10, max_iters=50, check_every=every)
            assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN), (which, every, res.iterations, res.status)
        # ... and the object is as good as new behind the NaN (y is rewritten by every apply)
        f = P.ilu0_export()
        r = KM.inputs(n, np.float64, seed=1)[0]
        assert _apply(P, r, np.float64).tobytes() == IM.apply(rp, ci, f, r, P.ilu0_info().lanes_per_row, np.float64).tobytes()
    finally:
        P.close()
        A.close()
