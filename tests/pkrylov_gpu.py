"""What tests/test_gpu_pbicgstab.py and tests/test_gpu_pgmres.py share: the device arrays, the one solver call in the model's terms (the object's solver,
or the plain one with a diagonal or nothing), the model's product through the handle, and the tests that read the same for both solvers, written once
over a `Kind` (which entry points, which model, how many products a step enqueues)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import oraclelib as O
import pkrylov_model as PK
from cvr_amd import capi, synth

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 200


def dtype_of(prec):
    return np.float64 if prec == "fp64" else np.float32


def tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def put(a, dtype, shift=0):
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.empty(a.size + shift, dtype=tdt(dtype), device="cuda")[shift:]
    t.copy_(torch.from_numpy(a))
    return t


class Kind:
    """one of the two solvers: `restart` is None for BiCGSTAB"""

    def __init__(self, restart=None):
        self.restart = restart
        self.name = "bicgstab" if restart is None else "gmres"
        self.symbols = ("cvr_pbicgstab_device", "cvr_pbicgstab") if restart is None else ("cvr_pgmres_device", "cvr_pgmres")

    def solve(self, H, P, b, x0=None, shift=0, minv=None, **kw):
        """the object's solver (P a Precond) or the plain one (P None, minv an array or None) on arrays of exactly nrows values; (Got, result)"""
        n = H.nrows
        bt = put(b, H.dtype, shift)
        xt = put(np.zeros(n) if x0 is None else x0, H.dtype, shift)
        mt = None if minv is None else put(minv, H.dtype, shift)
        torch.cuda.synchronize()
        if self.restart is None:
            if P is not None:
                res = H.pbicgstab(P, bt.data_ptr(), xt.data_ptr(), **kw)
            else:
                res = H.bicgstab(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), **kw)
        elif P is not None:
            _, res = H.pgmres(P, bt, x0=xt, restart=self.restart, **kw)
        else:
            _, res = H.gmres(bt, x0=xt, restart=self.restart, minv=mt, **kw)
        torch.cuda.synchronize()
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res

    def solve_host(self, H, P, b, x0=None, **kw):
        if self.restart is None:
            x, r = H.pbicgstab_host(P, b, x0=x0, **kw)
        else:
            x, r = H.pgmres_host(P, b, x0=x0, restart=self.restart, **kw)
        return KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), r

    def model(self, product, dtype, W, bs):
        if self.restart is None:
            return PK.PBicgstab(product, dtype, W, bs)
        return PK.PGmres(product, dtype, W, bs, restart=self.restart)

    def spmvs(self, steps):
        """spmv_count behind `steps` enqueued steps, by the header: 1 + 2 per step; 1 + the steps + the restarts (one in front of the first step of every
        later cycle)"""
        if self.restart is None:
            return 1 + 2 * steps
        return 1 + steps + ((steps - 1) // self.restart if steps > 0 else 0)

    def raw_device_call(self, h, p, b_ptr, x_ptr, opt, res):
        L = capi.lib()
        if self.restart is None:
            return L.cvr_pbicgstab_device(h, p, b_ptr, x_ptr, C.byref(opt), C.byref(res), None)
        return L.cvr_pgmres_device(h, p, b_ptr, x_ptr, self.restart, C.byref(opt), C.byref(res), None)


def same(got, entry, ctx):
    msg = KM.compare(got, entry)
    assert msg == "", (ctx, msg)


class Dev:
    """a handle with the buffers of the model's product: the handle's own cvr_spmv_device"""

    def __init__(self, H):
        self.H, self.n = H, H.nrows
        self.xbuf = torch.zeros(max(H.info.x_elems, self.n + 1), dtype=tdt(H.dtype), device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, self.n, 1), dtype=tdt(H.dtype), device="cuda")

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()


# ---- block_size = 1 is the plain solver with the exported diagonal ----
@functools.lru_cache(maxsize=None)
def banded40000(dtype):
    """nonsym_from_pattern of banded_sym(40000), rows scaled by s in [0.5, 2): the diagonal is s, its Jacobi preconditioner 1 / s"""
    n, _, rp, ci, _ = synth.banded_sym(40000)
    s = 0.5 + 1.5 * np.random.default_rng(7).random(n)
    return synth.nonsym_from_pattern(n, rp, ci, rscale=s, dtype=dtype)


def check_block_size_one(kind, layout, prec):
    dtype = dtype_of(prec)
    n, _, rp, ci, va = banded40000(dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS[layout])          # (every layout builds for this matrix: a failure here is a failure)
    P = capi.Precond.block_jacobi(rp, ci, va, 1)
    try:
        W = P.export()
        assert W.shape == (n, 1, 1) and P.info.identity_blocks == 0
        assert (W.reshape(-1) != 1).any()
        b = synth.x_rand(n).astype(dtype)
        x0 = KM.inputs(n, dtype)[1]
        for start, kw in ((None, dict(rtol=RTOL[dtype], max_iters=MAX_ITERS)), (x0, dict(rtol=0.0, max_iters=3, check_every=1)),
                          (x0, dict(rtol=RTOL[dtype], max_iters=MAX_ITERS, check_every=3))):
            ref, _ = kind.solve(A, None, b, start, minv=W.reshape(-1), **kw)
            got, _ = kind.solve(A, P, b, start, **kw)
            same(got, ref, (kind.name, layout, prec, kw))
            assert ref.iterations > 0
        assert ref.status == capi.CG_CONVERGED
    finally:
        P.close()
        A.close()


# ---- step by step against the model ----
def check_step_by_step(kind, n, bs, prec):
    dtype = dtype_of(prec)
    rtol = RTOL[dtype]
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        dev = Dev(A)
        W = P.export()
        b, x0, _ = KM.inputs(n, dtype)
        ctx = (kind.name, kind.restart, n, bs, prec)
        tr = kind.model(dev.product, dtype, W, bs).run(b, x0, rtol=rtol, max_iters=MAX_ITERS)
        last = tr.last
        assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < MAX_ITERS, (ctx, last)
        for k in range(last.iterations + 1):
            got, res = kind.solve(A, P, b, x0, rtol=rtol, max_iters=k, check_every=1)
            same(got, tr.at(k), (ctx, "max_iters", k))
            if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop
                assert res.spmv_count == kind.spmvs(k), (ctx, k, res.spmv_count)
        for every in (1, 3, MAX_ITERS):
            for shift in (0, 1):
                got, res = kind.solve(A, P, b, x0, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                same(got, last, (ctx, "check_every", every, "shift", shift))
        got, res = kind.solve(A, P, b, x0, rtol=rtol, max_iters=MAX_ITERS, check_every=MAX_ITERS)
        assert res.spmv_count == kind.spmvs(MAX_ITERS), (ctx, res.spmv_count)          # (every step of the one batch is enqueued, a stop or none)
        k = last.iterations // 2          # and below the stop, where the batches end at different steps
        for every in (3, MAX_ITERS):
            got, _ = kind.solve(A, P, b, x0, rtol=rtol, max_iters=k, check_every=every)
            same(got, tr.at(k), (ctx, "max_iters", k, "check_every", every))
        got, _ = kind.solve_host(A, P, b, x0=x0, rtol=rtol, max_iters=MAX_ITERS)          # the host twin
        same(got, last, (ctx, "host"))
    finally:
        P.close()
        A.close()


# ---- what it is for ----
def check_block_diagonal(kind):
    n, bs, rtol = 4096, 8, 1e-10
    _, _, rp, ci, va = synth.block_diag_nonsym(n, bs, cond=1e3)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        assert P.info.identity_blocks == 0
        b = synth.x_rand(n)
        got, res = kind.solve(A, P, b, rtol=rtol, max_iters=MAX_ITERS)
        plain, pres = kind.solve(A, None, b, rtol=rtol, max_iters=8)
        y, _ = O.csr_spmv64(rp, ci, va, got.x)
        true = float(np.linalg.norm(b - y) / np.linalg.norm(b))
        print(f"{kind.name} with block-Jacobi: {res.iterations} steps, true residual / rtol = {true / rtol:.3g}; plain after 8 steps: status {pres.status}, "
              f"residual / (rtol |b|) = {pres.residual_norm / (rtol * pres.b_norm):.3g}")
        assert res.status == capi.CG_CONVERGED and res.iterations <= 2
        assert true <= 2 * rtol
        assert pres.status == capi.CG_MAX_ITERS
    finally:
        P.close()
        A.close()


# ---- stop states and errors ----
def check_stop_states(kind, prec):
    dtype = dtype_of(prec)
    rtol = RTOL[dtype]
    n, bs = 1000, 8
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        b, x0, _ = KM.inputs(n, dtype)
        # max_iters = 0: the initial residual alone
        got, res = kind.solve(A, P, b, x0, rtol=rtol, max_iters=0)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1)
        # b == 0: x = 0 whatever the start
        got, res = kind.solve(A, P, np.zeros(n), x0, rtol=rtol, max_iters=MAX_ITERS)
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        # a start within the tolerance
        solved, res = kind.solve(A, P, b, rtol=rtol, max_iters=MAX_ITERS)
        assert res.status == capi.CG_CONVERGED and res.iterations > 0
        got, res = kind.solve(A, P, b, solved.x, rtol=1e-6 if dtype == np.float64 else 1e-3, max_iters=MAX_ITERS)
        assert got.x.tobytes() == solved.x.tobytes() and (res.iterations, res.status) == (0, capi.CG_CONVERGED)
        # a NaN in b: breakdown with 0 iterations, x untouched
        bn = b.copy()
        bn[n // 2] = np.nan
        for every in (1, 0):
            got, res = kind.solve(A, P, bn, x0, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN)
    finally:
        P.close()
        A.close()
    # the stop an exactly block-diagonal system ends in after one step (BiCGSTAB: s = r - alpha v vanishes, the half step; GMRES: w is spanned by v_0,
    # the lucky breakdown, v_1 is never formed): the model's, bit for bit, for every check_every.  (Blocks of condition 10: W in fp32 inverts them to 1e-6.)
    _, _, rp, ci, va = synth.block_diag_nonsym(n, bs, cond=10.0, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        tr = kind.model(Dev(A).product, dtype, P.export(), bs).run(b, x0, rtol=rtol, max_iters=MAX_ITERS)
        assert tr.last.terminal and tr.last.status == KM.CONVERGED and tr.last.iterations == 1, tr.last
        if kind.restart is None:
            assert tr.last.scalars.get("half")
        for every in (1, 3, 0):
            got, _ = kind.solve(A, P, b, x0, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            same(got, tr.last, (kind.name, prec, "the one-step stop", every))
    finally:
        P.close()
        A.close()


def check_errors(kind):
    n, bs = 250, 3
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    b = synth.x_rand(n)
    try:
        # n
        _, _, rp2, ci2, va2 = KM.banded("nonsym", n + 1, np.float64)
        Q = capi.Precond.block_jacobi(rp2, ci2, va2, bs)
        with pytest.raises(capi.CvrError) as e:
            kind.solve(A, Q, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value) and kind.symbols[1] in str(e.value)
        Q.close()
        # type
        F = capi.Precond.block_jacobi(rp, ci, va.astype(np.float32), bs)
        with pytest.raises(capi.CvrError) as e:
            kind.solve(A, F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            kind.solve_host(A, F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID
        F.close()
        # minv_dev beside the object
        bt, xt = put(b, np.float64), put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        capi.lib().cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        assert kind.raw_device_call(A._h, P._p, bt.data_ptr(), xt.data_ptr(), opt, res) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()
        # a rectangular handle
        R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)
        with pytest.raises(capi.CvrError) as e:
            kind.solve(R, P, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
        R.close()
        # a handle before cvr_preprocess
        L = capi.lib()
        view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
        opt.minv_dev = None
        assert kind.raw_device_call(h, P._p, bt.data_ptr(), xt.data_ptr(), opt, res) == capi.ERR_STATE
        assert "cvr_preprocess" in capi.last_error()
        assert L.cvr_destroy(h) == 0
    finally:
        P.close()
        A.close()


def check_device_mismatch(kind):
    if cvr_amd.device_count() < 2:
        pytest.skip("one device")
    n, bs = 250, 3
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs, device=1)
    try:
        with pytest.raises(capi.CvrError) as e:
            kind.solve(A, P, synth.x_rand(n), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "device" in str(e.value)
    finally:
        P.close()
        A.close()
        torch.cuda.set_device(0)


def check_one_object_two_handles(kind):
    """the object belongs to no handle: two handles of the same matrix in different layouts use it, in turn, with the same bits; the plain solver on the
    same handle returns afterwards what it returned before"""
    n, bs = 4099, 16
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    B = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS["plain"])
    try:
        b, x0, minv = KM.inputs(n, np.float64)
        before = [kind.solve(A, None, b, x0, minv=mv, rtol=1e-10, max_iters=MAX_ITERS)[0] for mv in (None, minv)]
        tr = kind.model(Dev(A).product, np.float64, P.export(), bs).run(b, None, rtol=1e-10, max_iters=MAX_ITERS)
        for H in (A, B, A):
            got, _ = kind.solve(H, P, b, rtol=1e-10, max_iters=MAX_ITERS)
            assert got.status == capi.CG_CONVERGED
            if H is A:
                same(got, tr.last, "two handles")
        after = [kind.solve(A, None, b, x0, minv=mv, rtol=1e-10, max_iters=MAX_ITERS)[0] for mv in (None, minv)]
        for x, y in zip(after, before):
            same(x, y, "the plain solver after the object's")
            assert y.status == capi.CG_CONVERGED
    finally:
        A.close()
        B.close()
        P.close()
