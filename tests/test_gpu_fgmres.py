"""GPU (MI355X): flexible GMRES(m) -- cvr_fgmres_device and cvr_fgmres through the ABI (CvrMatrix.fgmres, fgmres_host), against tests/fgmres_model.py.
The model's product is the handle's own cvr_spmv_device and its apply the object's own Precond.apply on device arrays, so the tests pin the solver,
not the kinds.  Comparisons with the model and with cvr_gmres_device are byte for byte.

  1. without a preconditioner: cvr_gmres_device's bits, fp64 and fp32, on every layout
  2. step by step against the model for block-Jacobi, ILU(0), ILU(0)-Jacobi, multicolour SGS and MIS(2) AMG: every max_iters, restart 3 and 5,
     check_every 1, 3 and max_iters, b and x off the 16-byte grid, the host twin
  3. every kind solves the 40 x 40 upwind convection-diffusion system to 1e-8; ILU(0) and the AMG kinds in fewer steps than cvr_gmres_device
  4. the kinds built for symmetric positive definite matrices are taken (Chebyshev, FSAI, a block-AMG object)
  5. the callback: two objects in alternation against the model, a callback that fails, a callback that raises
  6. stop states and errors; cvr_gmres_device and cvr_pgmres_device on the same handle afterwards"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import oraclelib as O
import pkrylov_gpu as G
from cvr_amd import capi, synth
from fgmres_model import FgmresModel

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-8, np.float32: 1e-5}          # (fp32: 1e-4 is reached within one cycle of 5 on the banded cases)
MAX_ITERS = 300
GMRES = {r: G.Kind(restart=r) for r in (3, 4, 5, 20)}


def solve(H, b, x0=None, restart=5, shift=0, precond=None, apply=None, **kw):
    """cvr_fgmres_device on arrays of exactly nrows values; (Got, result)"""
    bt = G.put(b, H.dtype, shift)
    xt = G.put(np.zeros(H.nrows) if x0 is None else x0, H.dtype, shift)
    torch.cuda.synchronize()
    _, res = H.fgmres(bt, restart, precond=precond, apply=apply, x0=xt, **kw)
    torch.cuda.synchronize()
    return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


class DevApply:
    """the model's apply: the object's own cvr_precond_apply_device on device arrays"""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.r = torch.zeros(max(n, 1), dtype=G.tdt(dtype), device="cuda")
        self.z = torch.zeros(max(n, 1), dtype=G.tdt(dtype), device="cuda")

    def __call__(self, P, v):
        self.r[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=self.dtype)))
        torch.cuda.synchronize()
        P.apply(self.r.data_ptr(), self.z.data_ptr())
        torch.cuda.synchronize()
        return self.z[: self.n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def upwind(m, dtype):
    return synth.upwind_2d(m, dtype=dtype)


def true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, np.asarray(x, dtype=np.float64))
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))


# ---- 1. no preconditioner ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.LAYOUTS))
def test_without_a_preconditioner_it_is_gmres_bit_for_bit(layout, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = G.banded40000(dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS[layout])
    try:
        b = synth.x_rand(n).astype(dtype)
        x0 = KM.inputs(n, dtype)[1]
        for start, kw in ((None, dict(rtol=G.RTOL[dtype], max_iters=G.MAX_ITERS)), (x0, dict(rtol=0.0, max_iters=3, check_every=1)),
                          (x0, dict(rtol=G.RTOL[dtype], max_iters=G.MAX_ITERS, check_every=3))):
            ref, rres = GMRES[4].solve(A, None, b, start, **kw)
            got, res = solve(A, b, start, restart=4, **kw)
            G.same(got, ref, (layout, prec, kw))
            assert res.spmv_count == rres.spmv_count and ref.iterations > 0
        assert ref.status == capi.CG_CONVERGED and ref.iterations > 4
    finally:
        A.close()


# ---- 2. step by step against the model ----
def _banded(n):
    return lambda dtype: KM.banded("nonsym", n, dtype)[2:]


def _grid24(dtype):
    return upwind(24, dtype)[2:]


STEP_KINDS = {
    "block-jacobi-250-3": (_banded(250), lambda A, rp, ci, va: capi.Precond.block_jacobi(rp, ci, va, 3)),
    "block-jacobi-4099-32": (_banded(4099), lambda A, rp, ci, va: capi.Precond.block_jacobi(rp, ci, va, 32)),
    "ilu0": (_grid24, lambda A, rp, ci, va: capi.Precond.ilu0(rp, ci, va)),
    "ilu0-jacobi-2": (_grid24, lambda A, rp, ci, va: capi.Precond.ilu0_jacobi(rp, ci, va, 2)),
    "mcsgs": (_grid24, lambda A, rp, ci, va: capi.Precond.mcsgs(rp, ci, va)),
    "amg-mis2": (_grid24, lambda A, rp, ci, va: capi.Precond.amg_mis2(A, rp, ci, va)),
}


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("kind", sorted(STEP_KINDS))
def test_step_by_step_against_the_model(kind, prec):
    dtype = G.dtype_of(prec)
    rtol = RTOL[dtype]
    matrix, build = STEP_KINDS[kind]
    rp, ci, va = matrix(dtype)
    n = len(rp) - 1
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = build(A, rp, ci, va)
    try:
        if kind == "amg-mis2":
            assert P.amg_info().levels >= 2
        dev, dap = G.Dev(A), DevApply(n, dtype)
        b, x0, _ = KM.inputs(n, dtype)
        for restart in (3, 5):
            ctx = (kind, prec, restart)
            tr = FgmresModel(dev.product, dtype, lambda k, v: dap(P, v), restart=restart).run(b, x0, rtol=rtol, max_iters=MAX_ITERS)
            last = tr.last
            print(ctx, "the model's terminal step:", last.iterations)
            assert last.terminal and last.status == KM.CONVERGED and restart < last.iterations < MAX_ITERS, (ctx, last)
            for k in range(last.iterations + 1):
                got, res = solve(A, b, x0, restart, precond=P, rtol=rtol, max_iters=k, check_every=1)
                G.same(got, tr.at(k), (ctx, "max_iters", k))
                if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop: the handle's own products
                    assert res.spmv_count == GMRES[restart].spmvs(k), (ctx, k, res.spmv_count)
            for every in (1, 3, MAX_ITERS):
                for shift in (0, 1):
                    got, _ = solve(A, b, x0, restart, shift=shift, precond=P, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                    G.same(got, last, (ctx, "check_every", every, "shift", shift))
            k = last.iterations // 2          # and below the stop, where the batches end at different steps
            for every in (3, MAX_ITERS):
                got, _ = solve(A, b, x0, restart, precond=P, rtol=rtol, max_iters=k, check_every=every)
                G.same(got, tr.at(k), (ctx, "max_iters", k, "check_every", every))
        x, r = A.fgmres_host(b, 5, precond=P, x0=x0, rtol=rtol, max_iters=MAX_ITERS)          # the host twin
        G.same(KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), last, (kind, prec, "host"))
    finally:
        P.close()
        A.close()


# ---- 3. what it is for ----
SOLVE_KINDS = {
    "block-jacobi": lambda A, rp, ci, va: capi.Precond.block_jacobi(rp, ci, va, 4),
    "ilu0": lambda A, rp, ci, va: capi.Precond.ilu0(rp, ci, va),
    "ilu0-jacobi-2": lambda A, rp, ci, va: capi.Precond.ilu0_jacobi(rp, ci, va, 2),
    "mcsgs": lambda A, rp, ci, va: capi.Precond.mcsgs(rp, ci, va),
    "amg": lambda A, rp, ci, va: capi.Precond.amg(A, rp, ci, va),
    "amg-smoothed": lambda A, rp, ci, va: capi.Precond.amg_smoothed(A, rp, ci, va),
    "amg-mis2": lambda A, rp, ci, va: capi.Precond.amg_mis2(A, rp, ci, va),
}
FEWER_STEPS = ("ilu0", "amg", "amg-smoothed", "amg-mis2")


@pytest.mark.parametrize("kind", sorted(SOLVE_KINDS))
def test_every_kind_solves_the_upwind_system(kind):
    """40 x 40 upwind convection-diffusion (synth.upwind_2d: cx = -0.5, cy = -0.25), restart 20, rtol 1e-8: the true residual by the oracle's CSR loop in fp64"""
    rtol = 1e-8
    n, _, rp, ci, va = upwind(40, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = SOLVE_KINDS[kind](A, rp, ci, va)
    try:
        b = synth.x_rand(n)
        got, res = solve(A, b, None, 20, precond=P, rtol=rtol, max_iters=2000)
        plain, pres = GMRES[20].solve(A, None, b, rtol=rtol, max_iters=2000)
        true = true_residual(rp, ci, va, got.x, b)
        print(f"cvr_fgmres with {kind}: {res.iterations} steps, status {res.status}, true residual / rtol = {true / rtol:.3g}; cvr_gmres: {pres.iterations} steps, status {pres.status}")
        assert res.status == capi.CG_CONVERGED and pres.status == capi.CG_CONVERGED
        assert true <= 2 * rtol
        if kind in FEWER_STEPS:
            assert res.iterations < pres.iterations
    finally:
        P.close()
        A.close()


# ---- 4. the kinds built for symmetric positive definite matrices ----
@pytest.mark.parametrize("kind", ["chebyshev", "fsai", "amg-block"])
def test_the_spd_kinds_are_taken(kind):
    """the 24 x 24 Laplacian, restart 20, rtol 1e-8"""
    rtol = 1e-8
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8) if kind == "amg-block" else cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = None
    try:
        if kind == "chebyshev":
            P = capi.Precond.chebyshev(A, 4, *A.chebyshev_bounds())
        elif kind == "fsai":
            P = capi.Precond.fsai(rp, ci, va)
        else:
            P = capi.Precond.amg_block(A, rp, ci, va, 2)
        b = synth.x_rand(n)
        got, res = solve(A, b, None, 20, precond=P, rtol=rtol, max_iters=500)
        true = true_residual(rp, ci, va, got.x, b)
        print(f"cvr_fgmres with {kind} on the Laplacian: {res.iterations} steps, true residual / rtol = {true / rtol:.3g}")
        assert res.status == capi.CG_CONVERGED and res.iterations > 0
        assert true <= 2 * rtol
    finally:
        if P is not None:
            P.close()
        A.close()


# ---- 5. the callback ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_a_callback_alternating_two_objects_is_the_model(prec):
    dtype = G.dtype_of(prec)
    rtol = RTOL[dtype]
    n = 4099
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    Ps = [capi.Precond.block_jacobi(rp, ci, va, 1), capi.Precond.block_jacobi(rp, ci, va, 4)]
    try:
        dev, dap = G.Dev(A), DevApply(n, dtype)
        b, x0, _ = KM.inputs(n, dtype)
        tr = FgmresModel(dev.product, dtype, lambda k, v: dap(Ps[k % 2], v), restart=5).run(b, x0, rtol=rtol, max_iters=MAX_ITERS)
        last = tr.last
        assert last.terminal and last.status == KM.CONVERGED and 5 < last.iterations < MAX_ITERS, last
        for every in (1, 3, MAX_ITERS):
            calls = []

            def apply(v, z, nn, stream):
                assert nn == n and v % 16 == 0 and z % 16 == 0
                Ps[len(calls) % 2].apply(v, z, stream)
                calls.append((v, z))
                return 0

            got, res = solve(A, b, x0, 5, apply=apply, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            G.same(got, last, (prec, "check_every", every))
            assert len(calls) >= last.iterations
        k = last.iterations - 2
        calls = []
        got, _ = solve(A, b, x0, 5, apply=apply, rtol=rtol, max_iters=k, check_every=2)
        G.same(got, tr.at(k), (prec, "max_iters", k))
        assert len(calls) == k          # one call per step, none for a column that is never formed
        true = true_residual(rp, ci, va, last.x, b)
        assert true <= 2 * rtol, true
    finally:
        for P in Ps:
            P.close()
        A.close()


def test_a_callback_that_fails_ends_the_solve():
    n = 250
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, 3)
    try:
        b, x0, _ = KM.inputs(n, np.float64)
        want, _ = solve(A, b, x0, 5, precond=P, rtol=1e-10, max_iters=MAX_ITERS)
        calls = []

        def seven(v, z, nn, stream):
            calls.append(v)
            if len(calls) == 3:
                return 7
            P.apply(v, z, stream)
            return 0

        with pytest.raises(capi.CvrError) as e:
            solve(A, b, x0, 5, apply=seven, rtol=1e-10, max_iters=MAX_ITERS, check_every=MAX_ITERS)
        assert e.value.code == capi.ERR_STATE and "7" in str(e.value) and "step 2" in str(e.value), str(e.value)
        assert len(calls) == 3          # nothing further is enqueued

        def raises(v, z, nn, stream):
            raise KeyError("from the callback")

        with pytest.raises(KeyError):
            solve(A, b, x0, 5, apply=raises, rtol=1e-10, max_iters=MAX_ITERS)
        torch.cuda.synchronize()
        got, _ = solve(A, b, x0, 5, precond=P, rtol=1e-10, max_iters=MAX_ITERS)          # the handle solves afterwards
        G.same(got, want, "after a failed callback")
        assert got.status == capi.CG_CONVERGED
    finally:
        P.close()
        A.close()


# ---- 6. stop states and errors ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    """pkrylov_gpu.check_stop_states' cases: max_iters = 0, b = 0, a start within the tolerance, a NaN in b, the lucky breakdown; with an object,
    with a callback (never gated) and with neither"""
    dtype = G.dtype_of(prec)
    rtol = G.RTOL[dtype]
    n, bs = 1000, 8
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    S = capi.Precond.mcsgs(rp, ci, va)
    b, x0, _ = KM.inputs(n, dtype)
    try:
        for name, kw in (("block-Jacobi", dict(precond=P)), ("mcsgs", dict(precond=S)), ("callback", dict(apply=lambda v, z, nn, st: P.apply(v, z, st))), ("none", {})):
            got, res = solve(A, b, x0, 5, rtol=rtol, max_iters=0, **kw)
            assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1), name
            got, res = solve(A, np.zeros(n), x0, 5, rtol=rtol, max_iters=MAX_ITERS, **kw)
            assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0), name
            solved, res = solve(A, b, None, 5, rtol=rtol, max_iters=MAX_ITERS, **kw)
            assert res.status == capi.CG_CONVERGED and res.iterations > 0, name
            got, res = solve(A, b, solved.x, 5, rtol=1e-6 if dtype == np.float64 else 1e-3, max_iters=MAX_ITERS, **kw)
            assert got.x.tobytes() == solved.x.tobytes() and (res.iterations, res.status) == (0, capi.CG_CONVERGED), name
            bn = b.copy()
            bn[n // 2] = np.nan
            for every in (1, 0):
                got, res = solve(A, bn, x0, 5, rtol=rtol, max_iters=MAX_ITERS, check_every=every, **kw)
                assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN), (name, every)
    finally:
        S.close()
        P.close()
        A.close()
    # the lucky breakdown: an exactly block-diagonal system ends after one step, v_1 is never formed; the model's bits for every check_every
    _, _, rp, ci, va = synth.block_diag_nonsym(n, bs, cond=10.0, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        dev, dap = G.Dev(A), DevApply(n, dtype)
        tr = FgmresModel(dev.product, dtype, lambda k, v: dap(P, v), restart=5).run(b, x0, rtol=rtol, max_iters=MAX_ITERS)
        assert tr.last.terminal and tr.last.status == KM.CONVERGED and tr.last.iterations == 1, tr.last
        for every in (1, 3, 0):
            got, _ = solve(A, b, x0, 5, precond=P, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            G.same(got, tr.last, (prec, "the one-step stop", every))
            got, _ = solve(A, b, x0, 5, apply=lambda v, z, nn, st: P.apply(v, z, st), rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            G.same(got, tr.last, (prec, "the one-step stop, callback", every))
    finally:
        P.close()
        A.close()


def test_errors_and_the_other_solvers_afterwards():
    n, bs = 250, 3
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    b, x0, minv = KM.inputs(n, np.float64)
    L = capi.lib()
    try:
        before = [GMRES[5].solve(A, None, b, x0, minv=mv, rtol=1e-10, max_iters=MAX_ITERS)[0] for mv in (None, minv)]
        before.append(GMRES[5].solve(A, P, b, x0, rtol=1e-10, max_iters=MAX_ITERS)[0])
        ok = lambda v, z, nn, st: P.apply(v, z, st)
        # p and apply both set
        with pytest.raises(capi.CvrError) as e:
            solve(A, b, x0, 5, precond=P, apply=ok, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "both" in str(e.value)
        # minv_dev beside either
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        fn = capi.APPLY_FN(lambda ctx, v, z, nn, st: 0)
        for p, f in ((P._p, capi.APPLY_FN()), (None, fn)):
            assert L.cvr_fgmres_device(A._h, p, f, None, bt.data_ptr(), xt.data_ptr(), 5, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
            assert "minv_dev" in capi.last_error() and "cvr_fgmres" in capi.last_error()
        # restart
        for restart in (0, capi.GMRES_MAX_RESTART + 1):
            with pytest.raises(capi.CvrError) as e:
                solve(A, b, x0, restart, precond=P, rtol=1e-8, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "restart" in str(e.value)
        # type
        F = capi.Precond.block_jacobi(rp, ci, va.astype(np.float32), bs)
        with pytest.raises(capi.CvrError) as e:
            solve(A, b, x0, 5, precond=F, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value) and "cvr_fgmres" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            A.fgmres_host(b, 5, precond=F, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID
        F.close()
        # n
        _, _, rp2, ci2, va2 = KM.banded("nonsym", n + 1, np.float64)
        Q = capi.Precond.block_jacobi(rp2, ci2, va2, bs)
        with pytest.raises(capi.CvrError) as e:
            solve(A, b, x0, 5, precond=Q, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value) and "cvr_fgmres" in str(e.value)
        Q.close()
        # a rectangular handle, a handle before cvr_preprocess
        R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)
        with pytest.raises(capi.CvrError) as e:
            solve(R, b, x0, 5, apply=ok, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
        R.close()
        view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
        opt.minv_dev = None
        assert L.cvr_fgmres_device(h, P._p, capi.APPLY_FN(), None, bt.data_ptr(), xt.data_ptr(), 5, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
        assert "cvr_preprocess" in capi.last_error()
        assert L.cvr_destroy(h) == 0
        # the other solvers on the same handle: what they returned before
        got, _ = solve(A, b, x0, 5, precond=P, rtol=1e-10, max_iters=MAX_ITERS)
        assert got.status == capi.CG_CONVERGED
        after = [GMRES[5].solve(A, None, b, x0, minv=mv, rtol=1e-10, max_iters=MAX_ITERS)[0] for mv in (None, minv)]
        after.append(GMRES[5].solve(A, P, b, x0, rtol=1e-10, max_iters=MAX_ITERS)[0])
        for x, y in zip(after, before):
            G.same(x, y, "cvr_gmres_device / cvr_pgmres_device after cvr_fgmres_device")
            assert y.status == capi.CG_CONVERGED
    finally:
        P.close()
        A.close()
