"""GPU (MI355X): the aggregation AMG preconditioner -- cvr_precond_amg, cvr_precond_amg_info, cvr_precond_amg_export_level, and
cvr_precond_apply_device / cvr_pcg with an object of this kind, all through the ABI, against tests/amg_model.py.

  * the export of every level byte for byte against the model, fp64 and fp32, from host and from device arrays, on amg_model.CASES: banded "spd" at
    n = 1, 2, 64, 65, 1025, the Laplacian at m = 3, 24, 40, singletons among coupled rows, two disconnected blocks, the diagonal matrix of 300 rows
    (a stall: one level, smoothed), max_levels = 1, coarse_size = 1, sweeps = 2 with coarse_scale = 1.5
  * the apply bit for bit against the cycle the test carries out itself: the products through CvrMatrix handles the test makes from the exported
    levels, the element-wise steps in numpy fp64; r and z off the 16-byte grid one at a time; the apply repeated.  Every product of that cycle is
    also held against the CSR loop within the bound fuzz_checks grants a product (1e-12 / 1e-5 of the row's sum |a x|): the device cycle and the
    pure-numpy one differ by nothing but their products
  * PCG step by step against the model (krylov_model's CG recurrence with that apply): max_iters 0 .. 4 at rtol 0; solves to 1e-8 on the 24 x 24 and
    40 x 40 Laplacians with the step counts within the issue's bounds; check_every 1, 3 and the default give the same bits; spmv_count = 1 + P +
    (1 + P) * (steps enqueued); the host twin
  * every error return, the entry points that decline this kind, the cross-kind calls, an object still usable behind an error"""
import ctypes as C

import numpy as np
import pytest
import torch

import amg_model as AM
import cvr_amd
import fuzz_checks as FC
import krylov_model as KM
import pkrylov_gpu as G
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu


class Levels:
    """what a caller makes of an object's exported levels: the model's Hierarchy and a handle per coarse level, made as the object makes its own
    (device arrays, the default options); level 0's product is the borrowed handle's.  check=True: every product is held against the CSR loop."""

    def __init__(self, A, P, check=False):
        info = P.amg_info()
        self.exp = [P.amg_export_level(l) for l in range(info.levels)]
        self.H = AM.from_export(info, self.exp, P.dtype)
        self.handles, self.keep, self.products = [], [], [G.Dev(A).product]
        f32 = P.dtype == np.float32
        for l, e in enumerate(self.exp[1:], 1):
            if l == info.levels - 1 and info.coarse_direct:
                self.products.append(None)
                continue
            t = [torch.from_numpy(a).cuda() for a in (e.rp, e.ci, e.va)]
            torch.cuda.synchronize()
            self.keep.append(t)
            h = cvr_amd.CvrMatrix.from_device(e.n, e.n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=f32)
            self.handles.append(h)
            self.products.append(G.Dev(h).product)
        self.count = 0
        if check:
            self.products = [None if p is None else self._checked(p, e) for p, e in zip(self.products, self.exp)]

    def _checked(self, product, e):
        def checked(x):
            y = product(x)
            self.count += 1
            FC.assert_oracle(y, e.rp, e.ci, e.va, x, ctx=("level of", e.n))
            return y
        return checked

    def apply(self, r):
        return AM.apply(self.H, self.products, r)

    def close(self):
        for h in self.handles:
            h.close()


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


# ---- the set-up and the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", AM.CASES, ids=AM.case_id)
def test_export_info_and_apply(case, prec):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = AM.matrix(name, dtype)
    model = AM.setup(rp, ci, va, dtype, **options)
    assert model.bad is None
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.amg(A, rp, ci, va, **options)
    Q = capi.Precond.amg_from_device(A, n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), is_f32=dtype == np.float32, **options)
    del rt, ct, vt          # the object keeps nothing of the caller's arrays
    lv = None
    try:
        for obj, how in ((P, "host arrays"), (Q, "device arrays")):
            info = obj.amg_info()
            got = [obj.amg_export_level(l) for l in range(info.levels)]
            assert AM.same_hierarchy(model, info, got) == "", (name, prec, how)
            o = dict(AM.DEFAULTS, **options)
            assert (info.sweeps, info.is_f32, info.max_levels, info.coarse_size, info.strength, info.coarse_scale) == (
                o["sweeps"], int(dtype == np.float32), o["max_levels"], o["coarse_size"], o["strength"], o["coarse_scale"])
            pi = obj.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks, pi.device) == (n, 0, int(dtype == np.float32), 0, 0, 0)
        lv = Levels(A, P, check=True)
        r = KM.inputs(n, dtype)[0]
        want = lv.apply(r)
        assert lv.count == model.products_per_apply()
        assert np.isfinite(want).all() and want.any()
        for obj in (P, Q):
            for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind three applies)
                got = _apply(obj, r, dtype, rshift, zshift)
                assert got.tobytes() == want.tobytes(), (name, prec, rshift, zshift, _first_difference(got, want))
    finally:
        if lv:
            lv.close()
        P.close()
        Q.close()
        A.close()


# ---- the solver, step by step ----
def _solve(H, P, b, x0=None, shift=0, **kw):
    bt = G.put(b, H.dtype, shift)
    xt = G.put(np.zeros(H.nrows) if x0 is None else x0, H.dtype, shift)
    torch.cuda.synchronize()
    res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw) if P is not None else H.cg(bt.data_ptr(), xt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _spmvs(per_apply, steps):
    return 1 + per_apply + (1 + per_apply) * steps


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", [("spd-1025", {}), ("laplacian-24", {}), ("laplacian-24", dict(max_levels=1, sweeps=2))], ids=AM.case_id)
def test_pcg_step_by_step_against_the_model(case, prec):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = AM.matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg(A, rp, ci, va, **options)
    lv = Levels(A, P)
    try:
        per_apply = lv.H.products_per_apply()
        b, x0, _ = KM.inputs(n, dtype)
        for start_name, start in (("zero", None), ("random", x0)):
            tr = AM.AmgPcg(lv.products[0], dtype, lv.H, lv.products).run(b, start, rtol=0.0, max_iters=4)
            for k in range(5):
                if k >= len(tr.steps) and not tr.last.terminal:
                    break
                for every in (1, 3, 0):
                    for shift in (0, 1):
                        got, res = _solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, prec, start_name, "max_iters", k, "check_every", every, "shift", shift))
                        if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop
                            assert res.spmv_count == _spmvs(per_apply, k), (k, every, res.spmv_count)
        x, r = A.pcg_host(P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        G.same(KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), tr.at(4), (name, prec, "host"))
    finally:
        lv.close()
        P.close()
        A.close()


@pytest.mark.parametrize("m, fsai_steps", [(24, 44), (40, 72)])
def test_laplacian_to_1e_8(m, fsai_steps):
    """the model's terminal entry whatever check_every is; at most half of cvr_cg's steps and fewer than FSAI's recorded ones; spmv_count by the
    formula with the steps enqueued (whole batches up to the stop)"""
    n, _, rp, ci, va = synth.laplacian_2d(m)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg(A, rp, ci, va)
    lv = Levels(A, P)
    try:
        per_apply = lv.H.products_per_apply()
        assert per_apply == 4 and P.amg_info().levels == 3
        b = KM.inputs(n, np.float64)[0]
        last = AM.AmgPcg(lv.products[0], np.float64, lv.H, lv.products).run(b, None, rtol=1e-8, max_iters=200).last
        plain, pres = _solve(A, None, b, rtol=1e-8, max_iters=400)
        print(f"laplacian_2d({m}): AMG-PCG {last.iterations} steps, cvr_cg {pres.iterations}, FSAI-PCG's record {fsai_steps}")
        assert last.terminal and last.status == KM.CONVERGED and pres.status == capi.CG_CONVERGED
        assert 2 * last.iterations <= pres.iterations and last.iterations < fsai_steps
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = _solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, ("check_every", every))
            assert res.spmv_count == _spmvs(per_apply, enqueued), (every, res.spmv_count, enqueued)
    finally:
        lv.close()
        P.close()
        A.close()


# ---- errors ----
def _raw_build(h, n, ncols, rp, ci, va, opt=None, f32=False):
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ascontiguousarray(va, dtype=np.float32 if f32 else np.float64)
    p = C.c_void_p()
    view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, int(f32), 0)
    rc = capi.lib().cvr_precond_amg(C.byref(p), h, C.byref(view), None if opt is None else C.byref(opt), None)
    assert rc != 0 and not p.value
    return rc, capi.last_error()


def test_invalid_arguments_and_an_object_still_usable_behind_an_error():
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg(A, rp, ci, va)
    lv = Levels(A, P)
    L = capi.lib()
    try:
        r = KM.inputs(n, np.float64)[0]
        want = lv.apply(r)
        for field, v in (("max_levels", 0), ("max_levels", 17), ("coarse_size", 0), ("coarse_size", 257), ("sweeps", 0), ("sweeps", 5), ("reserved0", 1),
                         ("strength", -0.1), ("strength", 1.0), ("strength", np.nan), ("coarse_scale", 0.0), ("coarse_scale", np.inf), ("coarse_scale", np.nan)):
            rc, msg = _raw_build(A._h, n, n, rp, ci, va, capi.amg_options(**{field: v}))
            assert rc == capi.ERR_INVALID and field in msg, (field, v, msg)
        o = capi.amg_options()
        o.reserved[3] = 1
        rc, msg = _raw_build(A._h, n, n, rp, ci, va, o)
        assert rc == capi.ERR_INVALID and "reserved[3]" in msg
        # the view against the handle, and the view's own checks
        rc, msg = _raw_build(A._h, 3, 4, [0, 1, 2, 3], [0, 1, 2], [1, 1, 1])
        assert rc == capi.ERR_INVALID and "square" in msg
        rc, msg = _raw_build(A._h, 4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 1, 2, 3], np.ones(6))
        assert rc == capi.ERR_INVALID and "nrows" in msg
        rc, msg = _raw_build(A._h, n, n, rp, ci, va, f32=True)
        assert rc == capi.ERR_INVALID and "type" in msg
        B = cvr_amd.CvrMatrix(4, 4, [0, 1, 3, 5, 6], np.array([0, 0, 1, 1, 2, 3], dtype=np.int32), np.ones(6))
        rc, msg = _raw_build(B._h, 4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3], np.ones(6))
        assert rc == capi.ERR_INVALID and "row 2" in msg and "increasing" in msg
        rc, msg = _raw_build(B._h, 4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3], np.ones(5))
        assert rc == capi.ERR_INVALID and "row 2" in msg and "diagonal" in msg
        rc, msg = _raw_build(B._h, 4, 4, [0, 1, 2, 3, 4], [0, 1, 2, 3], [1.0, 1.0, -2.0, 1.0])
        assert rc == capi.ERR_STATE and "level 0" in msg and "row 2 " in msg and "diagonal" in msg
        rc, msg = _raw_build(B._h, 4, 4, [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [1.0, 2.0, 2.0, 1.0, 1.0, 1.0])          # row 1: 1 - 2 * 2
        assert rc == capi.ERR_STATE and "level 0" in msg and "row 1 " in msg and "pivot" in msg
        # the same row named when the arrays lie on the device
        bad = [torch.from_numpy(a).cuda() for a in (np.array([0, 1, 3, 5, 6], dtype=np.int64), np.array([0, 0, 1, 2, 1, 3], dtype=np.int32), np.ones(6))]
        torch.cuda.synchronize()
        with pytest.raises(capi.CvrError) as e:
            capi.Precond.amg_from_device(B, 4, bad[0].data_ptr(), bad[1].data_ptr(), bad[2].data_ptr())
        assert e.value.code == capi.ERR_INVALID and "row 2" in str(e.value)
        B.close()
        assert L.cvr_precond_amg(None, A._h, None, None, None) == capi.ERR_INVALID
        # the apply's and the solver's own checks
        bt, xt = G.put(r, np.float64), G.put(np.zeros(n), np.float64)
        assert L.cvr_precond_apply_device(P._p, bt.data_ptr(), bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_apply_device(P._p, None, bt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_amg_info(P._p, None) == capi.ERR_INVALID
        e0 = lv.exp[0]
        assert L.cvr_precond_amg_export_level(P._p, 3, e0.rp.ctypes.data, e0.ci.ctypes.data, e0.va.ctypes.data, e0.dinv.ctypes.data, e0.agg.ctypes.data, None) == capi.ERR_INVALID
        assert "level" in capi.last_error()
        assert L.cvr_precond_amg_export_level(P._p, 0, e0.rp.ctypes.data, e0.ci.ctypes.data, e0.va.ctypes.data, e0.dinv.ctypes.data, None, None) == capi.ERR_INVALID
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        assert L.cvr_pcg_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_INVALID and "minv_dev" in capi.last_error()
        # n and type mismatches of the pair
        n2, _, rp2, ci2, va2 = synth.laplacian_2d(25)
        A2 = cvr_amd.CvrMatrix(n2, n2, rp2, ci2, va2)
        F = cvr_amd.CvrMatrix(n, n, rp, ci, va.astype(np.float32))
        with pytest.raises(capi.CvrError) as e:
            _solve(A2, P, np.ones(n2), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            _solve(F, P, np.ones(n), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        A2.close()
        F.close()
        # ... and behind all of it the object applies as before
        assert _apply(P, r, np.float64).tobytes() == want.tobytes()
        bn = r.copy()
        bn[n // 2] = np.nan          # a NaN in b: breakdown with 0 iterations; the next apply rewrites every buffer
        got, res = _solve(A, P, bn, rtol=1e-10, max_iters=20)
        assert (res.iterations, res.status) == (0, capi.CG_BREAKDOWN)
        assert _apply(P, r, np.float64).tobytes() == want.tobytes()
    finally:
        lv.close()
        P.close()
        A.close()


def test_entry_points_that_decline_this_kind_and_the_other_kinds_calls():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg(A, rp, ci, va)
    try:
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind 4 (AMG)" in capi.last_error(), (name, capi.last_error())

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
        # this kind's calls on the other kinds, the other kinds' calls on this one
        e = P.amg_export_level(0)
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        U = capi.Precond.ilu0(rp, ci, va)
        S = capi.Precond.fsai(rp, ci, va)
        for other in (J, U, S):
            assert L.cvr_precond_amg_info(other._p, C.byref(capi.AmgInfo())) == capi.ERR_INVALID and "kind" in capi.last_error()
            assert L.cvr_precond_amg_export_level(other._p, 0, e.rp.ctypes.data, e.ci.ctypes.data, e.va.ctypes.data, e.dinv.ctypes.data, None, None) == capi.ERR_INVALID
            assert "kind" in capi.last_error()
            other.close()
        assert L.cvr_precond_ilu0_info(P._p, C.byref(capi.Ilu0Info())) == capi.ERR_INVALID and "kind 4" in capi.last_error()
        assert L.cvr_precond_ilu0_export(P._p, out.ctypes.data) == capi.ERR_INVALID and "kind 4" in capi.last_error()
        assert L.cvr_precond_fsai_info(P._p, C.byref(capi.FsaiInfo())) == capi.ERR_INVALID and "kind 4" in capi.last_error()
        assert L.cvr_precond_chebyshev_info(P._p, C.byref(capi.ChebyshevInfo())) == capi.ERR_INVALID and "AMG" in capi.last_error()
    finally:
        P.close()
        A.close()
