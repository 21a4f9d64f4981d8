"""GPU (MI355X): the FSAI preconditioner -- cvr_precond_fsai, cvr_precond_fsai_info, cvr_precond_fsai_export, and cvr_precond_apply_device / cvr_pcg
with an object of this kind, all through the ABI, against tests/fsai_model.py.

  * the export byte for byte against the model and against the host twin, fp64 and fp32, from host and from device arrays: banded "spd" at n = 1, 2,
    63, 64, 65, 1025, the Laplacian at m = 3 and 24, dense SPD at n = 8, 32 and 40 (8 truncated rows), the arrow matrix; the info fields by the model
  * the apply byte for byte against two CvrMatrix products on handles the test makes from the exported arrays (the second with transpose=1); r and z
    off the 16-byte grid one at a time; the apply repeated
  * PCG step by step against the model (krylov_model's CG recurrence with that apply): max_iters 0 .. 4 at rtol 0, a solve to 1e-8 on the 24 x 24
    Laplacian; check_every 1, 3 and the default give the same bits; spmv_count = 1 + 2 + 3 * (steps enqueued); the host twin
  * dense SPD n = 32: PCG stops after 1 iteration (the factor is exact); Laplacian 40: at most two thirds of cvr_cg's iterations
  * every error return, the entry points that decline this kind, the stop states"""
import ctypes as C

import numpy as np
import pytest
import torch

import cvr_amd
import fsai_model as FM
import krylov_model as KM
import pkrylov_gpu as G
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

matrix, MATRICES = FM.matrix, FM.MATRICES


class Products:
    """the two handles a caller makes from an object's exported arrays, as the object makes its own: device arrays, the default options"""

    def __init__(self, P):
        n = P.info.n
        wrp, wci, wa, wb = P.fsai_export()
        t = [torch.from_numpy(a).cuda() for a in (wrp, wci, wa, wb)]
        torch.cuda.synchronize()
        f32 = P.dtype == np.float32
        self.A = cvr_amd.CvrMatrix.from_device(n, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=f32)
        self.Bt = cvr_amd.CvrMatrix.from_device(n, n, t[0].data_ptr(), t[1].data_ptr(), t[3].data_ptr(), is_f32=f32, transpose=1)
        self.a, self.bt = G.Dev(self.A).product, G.Dev(self.Bt).product

    def apply(self, r):
        return FM.apply(self.a, self.bt, r)

    def close(self):
        self.A.close()
        self.Bt.close()


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


def _same_export(got, want, ctx):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ctx
    for g, w in zip(got[2:4], want[2:4]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (ctx, _first_difference(g, w))


# ---- the set-up and the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", MATRICES)
def test_export_info_and_apply(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = matrix(name, dtype)
    model = FM.factor(rp, ci, va, dtype)
    assert model[4] is None
    _, _, _, max_row, truncated = FM.pattern(rp, ci)
    host = capi.fsai_factor_host(rp, ci, va)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.fsai(rp, ci, va)
    Q = capi.Precond.fsai_from_device(n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), is_f32=dtype == np.float32)
    del rt, ct, vt          # the object keeps nothing of the caller's
    pr = None
    try:
        for obj, how in ((P, "host arrays"), (Q, "device arrays")):
            i = obj.fsai_info()
            assert (i.n, i.nnz, i.max_row, i.lanes_per_row, i.truncated_rows, i.is_f32) == (n, int(model[0][-1]), max_row, FM.lanes(max_row), truncated, int(dtype == np.float32)), (name, how)
            assert not any(i.reserved)
            pi = obj.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks, pi.device) == (n, 0, int(dtype == np.float32), 0, 0, 0)
            got = obj.fsai_export()
            _same_export(got, model, (name, prec, how, "model"))
            _same_export(got, host, (name, prec, how, "host twin"))
        pr = Products(P)
        r = KM.inputs(n, dtype)[0]
        want = pr.apply(r)
        assert np.isfinite(want).all() and want.any()
        for obj in (P, Q):
            for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind three applies)
                got = _apply(obj, r, dtype, rshift, zshift)
                assert got.tobytes() == want.tobytes(), (name, prec, rshift, zshift, _first_difference(got, want))
    finally:
        if pr:
            pr.close()
        P.close()
        Q.close()


def test_n_zero():
    E = capi.Precond.fsai(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    i = E.fsai_info()
    assert (i.n, i.nnz, i.max_row, i.truncated_rows) == (0, 0, 0, 0)
    wrp, wci, wa, wb = E.fsai_export()
    assert (list(wrp), len(wci), len(wa), len(wb)) == ([0], 0, 0, 0)
    t = torch.zeros(4, dtype=torch.float64, device="cuda")
    E.apply(t.data_ptr(), t.data_ptr() + 16)          # enqueues nothing
    E.close()


# ---- the solver, step by step ----
def _solve(H, P, b, x0=None, shift=0, **kw):
    bt = G.put(b, H.dtype, shift)
    xt = G.put(np.zeros(H.nrows) if x0 is None else x0, H.dtype, shift)
    torch.cuda.synchronize()
    res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw) if P is not None else H.cg(bt.data_ptr(), xt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _spmvs(steps):
    return 1 + 2 + 3 * steps


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["spd-1025", "laplacian-24"])
def test_pcg_step_by_step_against_the_model(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    pr = Products(P)
    try:
        dev = G.Dev(A)
        b, x0, _ = KM.inputs(n, dtype)
        for start_name, start in (("zero", None), ("random", x0)):
            tr = FM.FsaiPcg(dev.product, dtype, pr.a, pr.bt).run(b, start, rtol=0.0, max_iters=4)
            for k in range(5):
                if k >= len(tr.steps) and not tr.last.terminal:
                    break
                for every in (1, 3, 0):
                    for shift in (0, 1):
                        got, res = _solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, prec, start_name, "max_iters", k, "check_every", every, "shift", shift))
                        if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop
                            assert res.spmv_count == _spmvs(k), (k, every, res.spmv_count)
        x, r = A.pcg_host(P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        G.same(KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), tr.at(4), (name, prec, "host"))
    finally:
        pr.close()
        P.close()
        A.close()


def test_laplacian_24_to_1e_8():
    """the model's terminal entry whatever check_every is; spmv_count by the formula with the steps enqueued (whole batches up to the stop)"""
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    pr = Products(P)
    try:
        b = KM.inputs(n, np.float64)[0]
        last = FM.FsaiPcg(G.Dev(A).product, np.float64, pr.a, pr.bt).run(b, None, rtol=1e-8, max_iters=200).last
        assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < 60, last
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = _solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, ("check_every", every))
            assert res.spmv_count == _spmvs(enqueued), (every, res.spmv_count, enqueued)
        print(f"FSAI-PCG: {last.iterations} steps on laplacian_2d(24)")
    finally:
        pr.close()
        P.close()
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_dense_spd_32_pcg_stops_after_one_iteration(prec):
    """every row's pattern is its whole lower triangle: W^T D^-1 W = A^-1 up to rounding, so the first step solves the system"""
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = FM.dense_spd(32, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    try:
        b = KM.inputs(n, dtype)[0]
        got, res = _solve(A, P, b, rtol=G.RTOL[dtype], max_iters=50)
        assert (res.status, res.iterations) == (capi.CG_CONVERGED, 1), (res.status, res.iterations, res.residual_norm / res.b_norm)
    finally:
        P.close()
        A.close()


def test_laplacian_40_pcg_needs_at_most_two_thirds_of_cgs_iterations():
    n, _, rp, ci, va = synth.laplacian_2d(40)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    try:
        b = KM.inputs(n, np.float64)[0]
        got, res = _solve(A, P, b, rtol=1e-8, max_iters=400)
        plain, pres = _solve(A, None, b, rtol=1e-8, max_iters=400)
        print(f"laplacian_2d(40): FSAI-PCG {res.iterations} steps, cvr_cg {pres.iterations}")
        assert res.status == capi.CG_CONVERGED and pres.status == capi.CG_CONVERGED
        assert 3 * res.iterations <= 2 * pres.iterations
    finally:
        P.close()
        A.close()


# ---- errors ----
def _raw_build(n, ncols, rp, ci, va, device=0):
    rp, ci, va = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=np.float64)
    p = C.c_void_p()
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    rc = capi.lib().cvr_precond_fsai(C.byref(p), C.byref(view), device, None)
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
    assert capi.lib().cvr_precond_fsai(None, None, 0, None) == capi.ERR_INVALID
    # the same row named when the arrays lie on the device
    rp, ci, va = np.array([0, 1, 3, 5, 6], dtype=np.int64), np.array([0, 0, 1, 2, 1, 3], dtype=np.int32), np.ones(6)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    with pytest.raises(capi.CvrError) as e:
        capi.Precond.fsai_from_device(4, rt.data_ptr(), ct.data_ptr(), vt.data_ptr())
    assert e.value.code == capi.ERR_INVALID and "row 2" in str(e.value)


def test_bad_pivots_name_the_row_and_leak_nothing():
    rc, msg = _raw_build(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0])          # row 1: 1 - 2 * 2
    assert rc == capi.ERR_STATE and "row 1 " in msg and "pivot" in msg
    n = 20000
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    d = rp[:-1] + np.array([np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0] for i in range(n)])
    nan = va.copy()
    nan[d[12345]] = np.nan          # the rows 12345 .. 12347 meet it: 12345 is the lowest
    neg = va.copy()
    neg[d[0]] = -1.0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        rc, msg = _raw_build(n, n, rp, ci, nan)
        assert rc == capi.ERR_STATE and "row 12345 " in msg, msg
        rc, msg = _raw_build(n, n, rp, ci, neg)
        assert rc == capi.ERR_STATE and "row 0 " in msg, msg
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    assert lost < 16 << 20, lost
    P = capi.Precond.fsai(rp, ci, va)          # ... and the next build succeeds
    assert P.fsai_info().n == n and np.isfinite(P.fsai_export()[2]).all()
    P.close()


def test_mismatches_of_the_pair_and_the_other_kinds_calls():
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    b = synth.x_rand(n)
    L = capi.lib()
    try:
        _, _, rp2, ci2, va2 = KM.banded("spd", n + 1, np.float64)
        Q = capi.Precond.fsai(rp2, ci2, va2)
        F = capi.Precond.fsai(rp, ci, va.astype(np.float32))
        with pytest.raises(capi.CvrError) as e:
            _solve(A, Q, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            _solve(A, F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        Q.close()
        F.close()
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        assert L.cvr_pcg_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_INVALID and "minv_dev" in capi.last_error()
        # r == z and null arguments of the apply, of the info and of the export
        assert L.cvr_precond_apply_device(P._p, bt.data_ptr(), bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_apply_device(P._p, None, bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_fsai_info(P._p, None) == capi.ERR_INVALID
        wrp, wci, wa, wb = P.fsai_export()
        assert L.cvr_precond_fsai_export(P._p, None, wci.ctypes.data, wa.ctypes.data, wb.ctypes.data) == capi.ERR_INVALID
        assert L.cvr_precond_fsai_export(P._p, wrp.ctypes.data, wci.ctypes.data, None, wb.ctypes.data) == capi.ERR_INVALID
        # this kind's calls on the other kinds, the other kinds' calls on this one
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        U = capi.Precond.ilu0(rp, ci, va)
        for other in (J, U):
            assert L.cvr_precond_fsai_info(other._p, C.byref(capi.FsaiInfo())) == capi.ERR_INVALID and "kind" in capi.last_error()
            assert L.cvr_precond_fsai_export(other._p, wrp.ctypes.data, wci.ctypes.data, wa.ctypes.data, wb.ctypes.data) == capi.ERR_INVALID and "kind" in capi.last_error()
        J.close()
        U.close()
        assert L.cvr_precond_ilu0_info(P._p, C.byref(capi.Ilu0Info())) == capi.ERR_INVALID and "kind 3" in capi.last_error()
        assert L.cvr_precond_ilu0_export(P._p, np.zeros(len(va)).ctypes.data) == capi.ERR_INVALID and "kind 3" in capi.last_error()
        assert L.cvr_precond_chebyshev_info(P._p, C.byref(capi.ChebyshevInfo())) == capi.ERR_INVALID and "FSAI" in capi.last_error()
    finally:
        P.close()
        A.close()


def test_entry_points_that_decline_this_kind():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    try:
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind 3" in capi.last_error() and "FSAI" in capi.last_error(), (name, capi.last_error())

        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), "apply_multi")
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), "pcg_multi_device")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), "pcg_multi")
        declined(L.cvr_pbicgstab_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None), "pbicgstab_device")
        declined(L.cvr_pbicgstab(A._h, P._p, hb.ctypes.data, hx.ctypes.data, C.byref(opt), C.byref(res)), "pbicgstab")
        declined(L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 30, C.byref(opt), C.byref(res), None), "pgmres_device")
        declined(L.cvr_pgmres(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 30, C.byref(opt), C.byref(res)), "pgmres")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran
        assert L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 9, None) == capi.ERR_INVALID          # behind their other checks
        assert L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 0, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
    finally:
        P.close()
        A.close()


def test_stop_states():
    n = 1000
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.fsai(rp, ci, va)
    pr = Products(P)
    try:
        b, x0, _ = KM.inputs(n, np.float64)
        got, res = _solve(A, P, b, x0, rtol=1e-10, max_iters=0)          # max_iters = 0: the initial residual alone, and the start's apply
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 3)
        got, res = _solve(A, P, np.zeros(n), x0, rtol=1e-10, max_iters=50)          # b == 0: x = 0 whatever the start
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        bn = b.copy()
        bn[n // 2] = np.nan          # a NaN in b: breakdown with 0 iterations, x untouched
        for every in (1, 0):
            got, res = _solve(A, P, bn, x0, rtol=1e-10, max_iters=50, check_every=every)
            assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN), (every, res.iterations, res.status)
        # ... and the object is as good as new behind the NaN (every apply rewrites its buffers)
        r = KM.inputs(n, np.float64, seed=1)[0]
        assert _apply(P, r, np.float64).tobytes() == pr.apply(r).tobytes()
    finally:
        pr.close()
        P.close()
        A.close()
