"""GPU (MI355X): the multicolour symmetric Gauss-Seidel preconditioner -- cvr_precond_mcsgs, cvr_precond_mcsgs_info, cvr_precond_mcsgs_export, and
cvr_precond_apply_device / cvr_pcg_device / cvr_pcg with an object of this kind, all through the ABI, against tests/mcsgs_model.py.  Every
comparison is byte for byte.

  * the colouring (export) and the apply against the model, fp64 and fp32, on every case of the model but the two large ones: r and z off the
    16-byte grid one at a time, every apply repeated, launches_per_apply == 2 * ncolors; every lane count 1 .. 64 on irr-sym-3000; grid-513 once
  * PCG step by step against the model: max_iters 0 .. 4 at rtol 0, a solve to 1e-8 on the 24 x 24 and 40 x 40 Laplacians; check_every 1, 3 and
    the default give the same bits; spmv_count by block-Jacobi's formula; the host twin; fewer steps than cvr_cg
  * a zero and a NaN diagonal, the entry points that decline this kind with their full texts, the other kinds' infos, n = 0 and n = 1, device arrays"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cvr_amd
import krylov_model as KM
import mcsgs_model as M
import pkrylov_gpu as G
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

SMALL = [c for c in M.CASES if c not in M.LARGE]


def _build(rp, ci, va, lanes=None):
    """Precond.mcsgs with CVR_DEBUG=mcsgs_lanes=<lanes> in the environment while the object is built (the switch is read there)"""
    old = os.environ.get("CVR_DEBUG")
    try:
        if lanes is not None:
            os.environ["CVR_DEBUG"] = f"mcsgs_lanes={lanes}"
        else:
            os.environ.pop("CVR_DEBUG", None)
        return capi.Precond.mcsgs(rp, ci, va)
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


def _check_export(P, name):
    n, rp, ci, _, color, ncolors, rounds, perm, ptr = M.case(name)
    got = P.mcsgs_export()
    assert got[0].tobytes() == color.tobytes() and got[1].tobytes() == perm.tobytes() and got[2].tobytes() == ptr.tobytes(), name
    return ncolors, rounds, np.diff(ptr)


# ---- the export and the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SMALL)
def test_export_and_apply_against_the_model(name, prec):
    dtype = G.dtype_of(prec)
    n, rp, ci, _, color = M.case(name)[:5]
    va = M.values(name, dtype)
    nnz = int(rp[-1])
    Gl = M.default_lanes(n, nnz)
    r = KM.inputs(n, dtype)[0]
    want = M.apply(rp, ci, va, color, r, Gl, dtype)
    assert np.isfinite(want).all()
    P = _build(rp, ci, va)
    try:
        ncolors, rounds, sizes = _check_export(P, name)
        i = P.mcsgs_info()
        assert (i.n, i.nnz, i.ncolors, i.rounds, i.launches_per_apply, i.lanes_per_row, i.is_f32) == (n, nnz, ncolors, rounds, 2 * ncolors, Gl, int(dtype == np.float32)), name
        assert (i.max_color_rows, i.min_color_rows) == (sizes.max(), sizes.min()) and not any(i.reserved)
        pi = P.info
        assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks, pi.device) == (n, 0, int(dtype == np.float32), 0, 0, 0)
        for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind three applies)
            got = _apply(P, r, dtype, rshift, zshift)
            assert got.tobytes() == want.tobytes(), (name, prec, rshift, zshift, _first_difference(got, want))
    finally:
        P.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_every_lane_count_on_the_irregular_case(prec):
    dtype = G.dtype_of(prec)
    name = "irr-sym-3000"
    n, rp, ci, _, color = M.case(name)[:5]
    va = M.values(name, dtype)
    r = KM.inputs(n, dtype)[0]
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        P = _build(rp, ci, va, lanes)
        try:
            assert P.mcsgs_info().lanes_per_row == lanes
            want = M.apply(rp, ci, va, color, r, lanes, dtype)
            for _ in range(2):
                got = _apply(P, r, dtype)
                assert got.tobytes() == want.tobytes(), (prec, lanes, _first_difference(got, want))
        finally:
            P.close()
    P = _build(rp, ci, va, 3)          # not a power of two: the default stays
    assert P.mcsgs_info().lanes_per_row == M.default_lanes(n, int(rp[-1]))
    P.close()


def test_grid_513_once():
    """more rows than one grid of 1024 x 256 threads"""
    name = "grid-513"
    n, rp, ci, va, color = M.case(name)[:5]
    P = _build(rp, ci, va)
    try:
        _check_export(P, name)
        r = KM.inputs(n, np.float64)[0]
        got = _apply(P, r, np.float64)
        want = M.apply(rp, ci, va, color, r, P.mcsgs_info().lanes_per_row, np.float64)
        assert got.tobytes() == want.tobytes(), _first_difference(got, want)
    finally:
        P.close()


def test_arrays_on_the_device_n_zero_and_n_one():
    name = "laplacian-24"
    n, rp, ci, va = M.matrix(name)
    rt, ct, vt = torch.from_numpy(np.array(rp)).cuda(), torch.from_numpy(np.array(ci)).cuda(), torch.from_numpy(np.array(va)).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.mcsgs_from_device(n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr())
    Q = capi.Precond.mcsgs(rp, ci, va)
    try:
        _check_export(P, name)
        _check_export(Q, name)
        r = KM.inputs(n, np.float64)[0]
        del rt, ct, vt          # the object keeps nothing of the caller's
        assert _apply(P, r, np.float64).tobytes() == _apply(Q, r, np.float64).tobytes()
    finally:
        P.close()
        Q.close()
    E = capi.Precond.mcsgs(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))          # n = 0 is valid
    i = E.mcsgs_info()
    color, perm, ptr = E.mcsgs_export()
    assert (i.n, i.nnz, i.ncolors, i.rounds, i.launches_per_apply, len(color), len(perm), ptr.tolist()) == (0, 0, 0, 0, 0, 0, 0, [0])
    E.close()
    for dtype in (np.float64, np.float32):
        O = capi.Precond.mcsgs(np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.array([4.0], dtype=dtype))
        i = O.mcsgs_info()
        assert (i.n, i.ncolors, i.rounds, i.launches_per_apply, i.lanes_per_row, i.max_color_rows, i.min_color_rows) == (1, 1, 1, 2, 1, 1, 1)
        z = _apply(O, np.array([3.0]), dtype)
        assert z.tobytes() == np.array([3.0 / 4.0], dtype=dtype).tobytes()
        O.close()


# ---- PCG, step by step ----
class _Pcg:
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


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["spd-1025", "laplacian-24"])
def test_pcg_step_by_step_against_the_model(name, prec):
    dtype = G.dtype_of(prec)
    n, rp, ci, _, color = M.case(name)[:5]
    va = M.values(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        dev = G.Dev(A)
        kind = _Pcg()
        obj = M.McSgs(rp, ci, va, dtype, G=P.mcsgs_info().lanes_per_row, color=color)
        b, x0, _ = KM.inputs(n, dtype)
        for start_name, start in (("zero", None), ("random", x0)):
            tr = M.McSgsPcg(dev.product, dtype, obj).run(b, start, rtol=0.0, max_iters=4)
            for k in range(5):
                if k >= len(tr.steps) and not tr.last.terminal:
                    break
                for every in (1, 3, 0):
                    for shift in (0, 1):
                        got, res = kind.solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, prec, start_name, "max_iters", k, "check_every", every, "shift", shift))
                        if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop
                            assert res.spmv_count == 1 + k, (k, every, res.spmv_count)
        got, _ = kind.solve_host(A, P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        G.same(got, tr.at(4), (name, prec, "host"))
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("name", ["laplacian-24", "laplacian-40"])
def test_laplacians_to_1e_8(name):
    """the model's terminal entry whatever check_every is; spmv_count by the formula with the steps enqueued (whole batches up to the stop); the
    step count is the model's and below plain cvr_cg's on the same system"""
    n, rp, ci, va, color = M.case(name)[:5]
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va)
    try:
        kind = _Pcg()
        obj = M.McSgs(rp, ci, va, np.float64, G=P.mcsgs_info().lanes_per_row, color=color)
        b = KM.inputs(n, np.float64)[0]
        last = M.McSgsPcg(G.Dev(A).product, np.float64, obj).run(b, None, rtol=1e-8, max_iters=300).last
        assert last.terminal and last.status == KM.CONVERGED and last.iterations > 0, last
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = kind.solve(A, P, b, rtol=1e-8, max_iters=300, check_every=every)
            G.same(got, last, (name, "check_every", every))
            assert res.iterations == last.iterations and res.spmv_count == 1 + enqueued, (every, res.spmv_count, enqueued)
        plain, pres = kind.solve(A, None, b, rtol=1e-8, max_iters=300)
        print(f"{name}: multicolour SGS PCG {last.iterations} steps, cvr_cg {pres.iterations}")
        assert pres.status == capi.CG_CONVERGED and last.iterations < pres.iterations
    finally:
        P.close()
        A.close()


# ---- the object's life cycle and the refusals ----
def _raw_build(n, ncols, rp, ci, va, device=0):
    rp, ci, va = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=np.float64)
    p = C.c_void_p()
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    rc = capi.lib().cvr_precond_mcsgs(C.byref(p), C.byref(view), device, None)
    assert rc != 0 and not p.value
    return rc, capi.last_error()


def test_invalid_views():
    rc, msg = _raw_build(3, 4, [0, 1, 2, 3], [0, 1, 2], [1, 1, 1])
    assert rc == capi.ERR_INVALID and msg == "multicolour SGS needs a square matrix (3 x 4)"
    rc, msg = _raw_build(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3], np.ones(6))
    assert rc == capi.ERR_INVALID and msg == "cvr_precond_mcsgs: row 2: the columns are not strictly increasing (1 behind 2)"
    rc, msg = _raw_build(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3], np.ones(5))
    assert rc == capi.ERR_INVALID and msg == "cvr_precond_mcsgs: row 2 has no diagonal entry"
    rc, msg = _raw_build(5, 5, [0, 1, 4, 5, 7, 8], [0, 1, 2, 3, 2, 3, 4, 4], np.ones(8))
    assert rc == capi.ERR_INVALID
    assert msg == "cvr_precond_mcsgs: row 1 has an entry in column 2, row 2 none in column 1: the off-diagonal pattern must be structurally symmetric"
    rc, msg = _raw_build(2, 2, [0, 1, 2], [0, 1], np.ones(2), device=cvr_amd.device_count())
    assert rc == capi.ERR_NO_DEVICE
    assert capi.lib().cvr_precond_mcsgs(None, None, 0, None) == capi.ERR_INVALID


def test_bad_diagonals_name_the_lowest_row_and_leak_nothing():
    n = 20000
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    d = np.flatnonzero(np.repeat(np.arange(n), np.diff(rp)) == ci)
    both = va.copy()
    both[d[12345]] = np.nan          # a NaN diagonal and, in a lower row, a zero one: the lowest is named
    both[d[777]] = 0.0
    nan = va.copy()
    nan[d[12345]] = np.nan
    assert M.bad_diagonal(rp, ci, both) == 777 and M.bad_diagonal(rp, ci, nan) == 12345
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        rc, msg = _raw_build(n, n, rp, ci, both)
        assert rc == capi.ERR_STATE and msg == "cvr_precond_mcsgs: the diagonal entry of row 777 is zero or not finite", msg
        rc, msg = _raw_build(n, n, rp, ci, nan)
        assert rc == capi.ERR_STATE and msg == "cvr_precond_mcsgs: the diagonal entry of row 12345 is zero or not finite", msg
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    assert lost < 16 << 20, lost          # 20 failed builds of about 3 MB each would have kept 60 MB
    P = capi.Precond.mcsgs(rp, ci, va)          # ... and the next build succeeds
    assert P.mcsgs_info().n == n
    P.close()


def test_entry_points_that_decline_this_kind():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.mcsgs(rp, ci, va)
    try:
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))
        only_bj = "%s: the preconditioner is of kind 5 (multicolour SGS): this entry point takes block-Jacobi objects (kind 0) only"
        bj_or_ilu = "%s: the preconditioner is of kind 5 (multicolour SGS): this entry point takes block-Jacobi and ILU(0) objects (kinds 0 and 2) only"

        def declined(rc, text):
            assert rc == capi.ERR_STATE and capi.last_error() == text, (rc, capi.last_error(), text)

        declined(L.cvr_precond_export(P._p, out.ctypes.data), only_bj % "cvr_precond_export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), only_bj % "cvr_precond_apply_multi_device")
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), only_bj % "cvr_pcg_multi")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), only_bj % "cvr_pcg_multi")
        declined(L.cvr_pbicgstab_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None), bj_or_ilu % "cvr_pbicgstab")
        declined(L.cvr_pbicgstab(A._h, P._p, hb.ctypes.data, hx.ctypes.data, C.byref(opt), C.byref(res)), bj_or_ilu % "cvr_pbicgstab")
        declined(L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 30, C.byref(opt), C.byref(res), None), bj_or_ilu % "cvr_pgmres")
        declined(L.cvr_pgmres(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 30, C.byref(opt), C.byref(res)), bj_or_ilu % "cvr_pgmres")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran
        # the other kinds' infos and exports on this kind, and this kind's on another
        for call, info in ((L.cvr_precond_chebyshev_info, capi.ChebyshevInfo()), (L.cvr_precond_ilu0_info, capi.Ilu0Info()), (L.cvr_precond_fsai_info, capi.FsaiInfo()),
                           (L.cvr_precond_amg_info, capi.AmgInfo()), (L.cvr_precond_amg_smoothed_info, capi.AmgSmoothedInfo()), (L.cvr_precond_amg_mis2_info, capi.AmgMis2Info())):
            assert call(P._p, C.byref(info)) == capi.ERR_INVALID, call.__name__
        assert L.cvr_precond_ilu0_export(P._p, out.ctypes.data) == capi.ERR_INVALID
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        i32 = np.zeros(n + 1, dtype=np.int32)
        assert L.cvr_precond_mcsgs_info(J._p, C.byref(capi.McSgsInfo())) == capi.ERR_INVALID
        assert capi.last_error() == "cvr_precond_mcsgs_info: the preconditioner is of kind 0, not a multicolour SGS object (kind 5)"
        assert L.cvr_precond_mcsgs_export(J._p, i32.ctypes.data, i32.ctypes.data, i32.ctypes.data) == capi.ERR_INVALID
        assert capi.last_error() == "cvr_precond_mcsgs_export: the preconditioner is of kind 0, not a multicolour SGS object (kind 5)"
        J.close()
        assert L.cvr_precond_mcsgs_info(P._p, None) == capi.ERR_INVALID and L.cvr_precond_mcsgs_export(P._p, i32.ctypes.data, i32.ctypes.data, None) == capi.ERR_INVALID
        assert L.cvr_precond_apply_device(P._p, bt.data_ptr(), bt.data_ptr(), None) == capi.ERR_INVALID
    finally:
        P.close()
        A.close()


def test_mismatches_of_the_pair_and_stop_states():
    n = 1000
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.mcsgs(rp, ci, va)
    kind = _Pcg()
    try:
        _, _, rp2, ci2, va2 = KM.banded("spd", n + 1, np.float64)
        Q = capi.Precond.mcsgs(rp2, ci2, va2)
        F = capi.Precond.mcsgs(rp, ci, va.astype(np.float32))
        b, x0, _ = KM.inputs(n, np.float64)
        with pytest.raises(capi.CvrError) as e:
            kind.solve(A, Q, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            kind.solve(A, F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        Q.close()
        F.close()
        got, res = kind.solve(A, P, b, x0, rtol=1e-10, max_iters=0)          # max_iters = 0: the initial residual alone
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1)
        got, res = kind.solve(A, P, np.zeros(n), x0, rtol=1e-10, max_iters=50)          # b == 0: x = 0 whatever the start
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        bn = b.copy()
        bn[n // 2] = np.nan          # a NaN in b: breakdown with 0 iterations, x untouched
        for every in (1, 0):
            got, res = kind.solve(A, P, bn, x0, rtol=1e-10, max_iters=50, check_every=every)
            assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN), (every, res.iterations, res.status)
        # ... and the object is as good as new behind the NaN (y is rewritten by every apply)
        r = KM.inputs(n, np.float64, seed=1)[0]
        color = M.coloring(rp, ci)[0]
        assert _apply(P, r, np.float64).tobytes() == M.apply(rp, ci, va, color, r, P.mcsgs_info().lanes_per_row, np.float64).tobytes()
    finally:
        P.close()
        A.close()
