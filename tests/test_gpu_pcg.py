"""GPU (MI355X): conjugate gradients with the block-Jacobi preconditioner object -- cvr_pcg_device / cvr_pcg, all through the ABI.

  * the block_size = 1 contract: bit for bit cvr_cg_device with minv_dev = the exported W, on every layout of cases.LAYOUTS in fp64 and fp32 (the 40 000-row
    banded SPD matrix of test_gpu_cg.py)
  * step by step against precond_model.Pcg on the exported W: every max_iters = k up to the model's terminal step, with the handle's own
    cvr_spmv_device as the model's product; the same bits for check_every = 1, 3 and max_iters, for arrays off the 16-byte grid and from the host twin
  * the benefit: an exactly block-diagonal matrix (blocks of condition 1e3) is solved within 2 steps, true residual (the oracle's CSR loop in fp64)
    within 2 * rtol
  * the stop states, the error returns with real objects, an object shared by two handles, and cvr_cg_device on the same handle afterwards"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import oraclelib as O
import precond_model as PM
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 60


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _put(a, dtype, shift=0):
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.empty(a.size + shift, dtype=_tdt(dtype), device="cuda")[shift:]
    t.copy_(torch.from_numpy(a))
    return t


def _solve(H, P, b, x0=None, shift=0, minv=None, **kw):
    """cvr_pcg_device (P a Precond) or cvr_cg_device (P None, minv an array or None) on arrays of exactly nrows values; (Got, result)"""
    n = H.nrows
    bt = _put(b, H.dtype, shift)
    xt = _put(np.zeros(n) if x0 is None else x0, H.dtype, shift)
    mt = None if minv is None else _put(minv, H.dtype, shift)
    torch.cuda.synchronize()
    if P is not None:
        res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw)
    else:
        res = H.cg(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _same(got, entry, ctx):
    msg = KM.compare(got, entry)
    assert msg == "", (ctx, msg)


# ---- block_size = 1 is cvr_cg_device with the exported diagonal ----
@functools.lru_cache(maxsize=None)
def _banded40000(dtype):
    n, _, rp, ci, _ = synth.banded_sym(40000)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.LAYOUTS))
def test_block_size_one_is_cg_with_the_exported_diagonal(layout, prec):
    dtype = _dtype(prec)
    n, _, rp, ci, va = _banded40000(dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS[layout])          # (every layout builds for this matrix: a failure here is a failure)
    P = capi.Precond.block_jacobi(rp, ci, va, 1)
    try:
        W = P.export()
        assert W.shape == (n, 1, 1) and P.info.identity_blocks == 0
        b = synth.x_rand(n).astype(dtype)
        x0 = KM.inputs(n, dtype)[1]
        for start, kw in ((None, dict(rtol=RTOL[dtype], max_iters=MAX_ITERS)), (x0, dict(rtol=0.0, max_iters=3, check_every=1)), (x0, dict(rtol=RTOL[dtype], max_iters=MAX_ITERS, check_every=3))):
            ref, rres = _solve(A, None, b, start, minv=W.reshape(-1), **kw)
            got, gres = _solve(A, P, b, start, **kw)
            _same(got, ref, (layout, prec, kw))
            assert ref.iterations > 0
        assert ref.status == capi.CG_CONVERGED
    finally:
        P.close()
        A.close()


# ---- step by step against the model ----
class Dev:
    """a handle with the buffers of the model's product: the handle's own cvr_spmv_device"""

    def __init__(self, H):
        self.H, self.n = H, H.nrows
        self.xbuf = torch.zeros(max(H.info.x_elems, self.n + 1), dtype=_tdt(H.dtype), device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, self.n, 1), dtype=_tdt(H.dtype), device="cuda")

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", [(250, 3), (1000, 8), (4099, 32)])
def test_step_by_step_against_the_model(n, bs, prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        dev = Dev(A)
        W = P.export()
        b, x0, _ = KM.inputs(n, dtype)
        for name, start in (("zero", None), ("random", x0)):
            ctx = (n, bs, prec, name)
            tr = PM.Pcg(dev.product, dtype, W, bs).run(b, start, rtol=rtol, max_iters=MAX_ITERS)
            last = tr.last
            assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < 30, (ctx, last)
            for k in range(len(tr.steps)):
                got, res = _solve(A, P, b, start, rtol=rtol, max_iters=k, check_every=1)
                _same(got, tr.at(k), (ctx, "max_iters", k))
                assert res.spmv_count == res.iterations + 1, (ctx, k, res.spmv_count)
            for every in (1, 3, MAX_ITERS):
                for shift in (0, 1):
                    got, res = _solve(A, P, b, start, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                    _same(got, last, (ctx, "check_every", every, "shift", shift))
            k = len(tr.steps) // 2          # and below the stop, where the batches end at different steps
            for every in (3, MAX_ITERS):
                got, _ = _solve(A, P, b, start, rtol=rtol, max_iters=k, check_every=every)
                _same(got, tr.at(k), (ctx, "max_iters", k, "check_every", every))
            xh, rh = A.pcg_host(P, b, x0=start, rtol=rtol, max_iters=MAX_ITERS)          # the host twin
            _same(KM.Got(xh, rh.iterations, rh.status, rh.residual_norm, rh.b_norm), last, (ctx, "host"))
    finally:
        P.close()
        A.close()


# ---- what it is for ----
def test_block_diagonal_system_is_solved_within_two_steps():
    n, bs, rtol = 4096, 8, 1e-10
    _, _, rp, ci, va = synth.block_diag_spd(n, bs, cond=1e3)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        assert P.info.identity_blocks == 0
        b = synth.x_rand(n)
        got, res = _solve(A, P, b, rtol=rtol, max_iters=MAX_ITERS)
        plain, pres = _solve(A, None, b, rtol=rtol, max_iters=8)
        y, _ = O.csr_spmv64(rp, ci, va, got.x)
        true = float(np.linalg.norm(b - y) / np.linalg.norm(b))
        print(f"block-Jacobi: {res.iterations} steps, true residual / rtol = {true / rtol:.3g}; plain CG after 8 steps: residual / (rtol |b|) = {pres.residual_norm / (rtol * pres.b_norm):.3g}")
        assert res.status == capi.CG_CONVERGED and res.iterations <= 2
        assert true <= 2 * rtol
        assert pres.status == capi.CG_MAX_ITERS
    finally:
        P.close()
        A.close()


# ---- stop states and errors ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    n, bs = 1000, 8
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        b, x0, _ = KM.inputs(n, dtype)
        # max_iters = 0: the initial residual alone
        got, res = _solve(A, P, b, x0, rtol=rtol, max_iters=0)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 1)
        # b == 0: x = 0 whatever the start
        got, res = _solve(A, P, np.zeros(n), x0, rtol=rtol, max_iters=MAX_ITERS)
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        # a start within the tolerance
        solved, res = _solve(A, P, b, rtol=rtol, max_iters=MAX_ITERS)
        assert res.status == capi.CG_CONVERGED and res.iterations > 0
        got, res = _solve(A, P, b, solved.x, rtol=1e-6 if dtype == np.float64 else 1e-3, max_iters=MAX_ITERS)
        assert got.x.tobytes() == solved.x.tobytes() and (res.iterations, res.status) == (0, capi.CG_CONVERGED)
        # a NaN in b: breakdown at step 0, x untouched
        bn = b.copy()
        bn[n // 2] = np.nan
        got, res = _solve(A, P, bn, x0, rtol=rtol, max_iters=MAX_ITERS)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN)
        # cvr_cg_device on the same handle afterwards: the bits it had before
        before, _ = _solve(A, None, b, x0, rtol=rtol, max_iters=MAX_ITERS)
        _solve(A, P, b, x0, rtol=rtol, max_iters=MAX_ITERS)
        after, _ = _solve(A, None, b, x0, rtol=rtol, max_iters=MAX_ITERS)
        _same(after, before, "cg after pcg")
    finally:
        A.close()
    # an indefinite A: p . A p < 0 at the first step (the object is still A's)
    N = cvr_amd.CvrMatrix(n, n, rp, ci, -va)
    try:
        got, res = _solve(N, P, b, x0, rtol=rtol, max_iters=MAX_ITERS)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN)
    finally:
        N.close()
        P.close()


def test_errors_with_real_objects():
    n, bs = 250, 3
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    b = synth.x_rand(n)
    try:
        # n
        _, _, rp2, ci2, va2 = KM.banded("spd", n + 1, np.float64)
        Q = capi.Precond.block_jacobi(rp2, ci2, va2, bs)
        with pytest.raises(capi.CvrError) as e:
            _solve(A, Q, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        Q.close()
        # type
        F = capi.Precond.block_jacobi(rp, ci, va.astype(np.float32), bs)
        with pytest.raises(capi.CvrError) as e:
            _solve(A, F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            A.pcg_host(F, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID
        F.close()
        # minv_dev beside the object
        bt, xt = _put(b, np.float64), _put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        capi.lib().cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        assert capi.lib().cvr_pcg_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()
        # a rectangular handle
        R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)
        with pytest.raises(capi.CvrError) as e:
            _solve(R, P, b, rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
        R.close()
    finally:
        P.close()
        A.close()


def test_device_mismatch():
    if cvr_amd.device_count() < 2:
        pytest.skip("one device")
    n, bs = 250, 3
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, bs, device=1)
    try:
        with pytest.raises(capi.CvrError) as e:
            _solve(A, P, synth.x_rand(n), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "device" in str(e.value)
    finally:
        P.close()
        A.close()
        torch.cuda.set_device(0)


def test_one_object_two_handles():
    """the object belongs to no handle: two handles of the same matrix in different layouts use it, in turn, with the same bits"""
    n, bs = 4099, 16
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    B = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS["plain"])
    try:
        b = synth.x_rand(n)
        tr = PM.Pcg(Dev(A).product, np.float64, P.export(), bs).run(b, None, rtol=1e-10, max_iters=MAX_ITERS)
        for H in (A, B, A):
            got, _ = _solve(H, P, b, rtol=1e-10, max_iters=MAX_ITERS)
            assert got.status == capi.CG_CONVERGED
            if H is A:
                _same(got, tr.last, "two handles")
    finally:
        A.close()
        B.close()
        P.close()
