"""GPU (MI355X): the Chebyshev polynomial preconditioner -- cvr_precond_chebyshev, cvr_precond_chebyshev_info, cvr_chebyshev_bounds, and
cvr_precond_apply_device / cvr_pcg_device / cvr_pcg with an object of this kind, all through the ABI, against tests/chebyshev_model.py.

  * the apply byte for byte against the model (the handle's own cvr_spmv_device as the model's product): degree 1, 2, 3, 16; fp64 and fp32;
    n = 1, 63, 64, 65, 1025, 4097; a banded SPD matrix and the power-law shape with empty rows; r and z off the 16-byte grid one by one; the plain
    layout and column phases.  The object's zi is not reachable through the ABI: that zi[ncols] stays 0 is checked through what it feeds -- every apply
    is repeated and gives the same bits (the products of a later apply read zi[ncols] at every pad slot)
  * PCG step by step against the model: x byte for byte, iterations, status, residual_norm and b_norm equal, max_iters 0 .. 4 at rtol 0 and a solve to
    rtol 1e-8 on the 24 x 24 Laplacian; check_every 1, 3 and the default give the same bits; spmv_count by the formula; the host twin
  * degree 1 on fp64 is cvr_cg_device with a constant minv, bit for bit
  * the stop states (NaN in b, b = 0), bounds that make the polynomial indefinite, cvr_chebyshev_bounds against the model, a mutable handle after
    cvr_update_values, every error return, CVR_ERR_STATE from the entry points that take block-Jacobi objects only"""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as K
import chebyshev_model as CM
import cvr_amd
import krylov_model as KM
import oraclelib as O
import power_model as PW
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1025, 4097]
DEGREES = [1, 2, 3, 16]
LAYOUTS = {"plain": K.LAYOUTS["plain"], "phases": K.LAYOUTS["phases"]}


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _put(a, dtype, shift=0):
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.empty(a.size + shift, dtype=_tdt(dtype), device="cuda")[shift:]
    t.copy_(torch.from_numpy(a))
    return t


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


def _apply(P, r, dtype, rshift=0, zshift=0):
    rt = _put(r, dtype, rshift)
    zt = _put(np.full(len(r), np.nan), dtype, zshift)
    torch.cuda.synchronize()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    return zt.cpu().numpy()


def _solve(H, P, b, x0=None, shift=0, minv=None, **kw):
    """cvr_pcg_device (P a Precond) or cvr_cg_device (P None) on arrays of exactly nrows values; (Got, result)"""
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


def _matrix(kind, n, dtype):
    """(row_ptr, col_idx, vals, lmin, lmax): the banded SPD matrix (spectrum in [0.5, 1.5]) with bounds around it, or the power-law shape with empty
    rows (power_model.power_law, not symmetric; values times 2^-10, so that its row sums stay below 3 and sixteen steps overflow nothing) with bounds
    that are only numbers"""
    if kind == "banded":
        _, _, rp, ci, va = KM.banded("spd", n, dtype)
        return rp, ci, va, 0.4, 1.6
    _, _, rp, ci, va = PW.power_law(n, dtype)
    return rp, ci, (va * dtype(2.0 ** -10)).astype(dtype), 0.1, 4.0


def _make(n, rp, ci, va, opts, **kw):
    try:
        return cvr_amd.CvrMatrix(n, n, rp, ci, va, **dict(opts, **kw))
    except capi.CvrError:          # (a layout the options cannot build for this matrix)
        return None


# ---- the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", ["banded", "power_law"])
def test_apply_against_the_model(kind, layout, prec):
    dtype = _dtype(prec)
    built = []
    for n in SIZES:
        rp, ci, va, lmin, lmax = _matrix(kind, n, dtype)
        A = _make(n, rp, ci, va, LAYOUTS[layout])
        if A is None:
            continue
        built.append(n)
        try:
            dev = Dev(A)
            r = KM.inputs(n, dtype)[0]
            for degree in DEGREES:
                want = CM.apply(dev.product, r, degree, lmin, lmax, dtype)
                assert np.isfinite(want).all(), (kind, n, degree)
                P = capi.Precond.chebyshev(A, degree, lmin, lmax)
                try:
                    for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind three applies)
                        got = _apply(P, r, dtype, rshift, zshift)
                        assert got.tobytes() == want.tobytes(), (kind, layout, prec, n, degree, rshift, zshift, int(np.flatnonzero(got != want)[0]) if (got != want).any() else -1)
                finally:
                    P.close()
        finally:
            A.close()
    assert layout != "plain" or built == SIZES, built          # the plain layout builds for every size
    assert {1025, 4097} <= set(built), built                   # ... and column phases for these at least (tests/test_gpu_power_model.py runs them)
    print(f"{kind} / {layout} / {prec}: built for n = {built}")


def test_info_of_both_calls():
    n = 1025
    _, _, rp, ci, va = KM.banded("spd", n, np.float32)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.chebyshev(A, 5, 0.25, 1.75)
    try:
        i = P.info
        assert (i.n, i.block_size, i.is_f32, i.nblocks, i.identity_blocks, i.device) == (n, 0, 1, 0, 0, 0)
        ci_ = P.chebyshev_info()
        model = CM.Cheb(5, 0.25, 1.75, np.float32)
        assert (ci_["degree"], ci_["is_f32"], ci_["lmin"], ci_["lmax"]) == (5, 1, 0.25, 1.75)
        assert ci_["a"].tobytes() == model.a.tobytes() and ci_["b"].tobytes() == model.b.tobytes()
        assert ci_["a"][0] == 0 and ci_["b"][0] == 1.0          # c0 = 1 / theta, theta = 1
        raw = capi.ChebyshevInfo()
        assert capi.lib().cvr_precond_chebyshev_info(P._p, C.byref(raw)) == 0
        assert not any(raw.a[5:]) and not any(raw.b[5:])
    finally:
        P.close()
        A.close()


# ---- the solver, step by step ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 2, 3, 8])
def test_pcg_step_by_step_against_the_model(degree, prec):
    dtype = _dtype(prec)
    n = 1025
    rp, ci, va, lmin, lmax = _matrix("banded", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.chebyshev(A, degree, lmin, lmax)
    try:
        dev = Dev(A)
        b, x0, _ = KM.inputs(n, dtype)
        cheb = CM.Cheb(degree, lmin, lmax, dtype)
        for name, start in (("zero", None), ("random", x0)):
            tr = CM.ChebPcg(dev.product, dtype, cheb).run(b, start, rtol=0.0, max_iters=4)
            assert len(tr.steps) == 5 and not tr.last.terminal, (degree, prec, name, tr.last)
            for k in range(5):
                for every in (1, 0):
                    for shift in (0, 1):
                        got, res = _solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        _same(got, tr.at(k), (degree, prec, name, "max_iters", k, "check_every", every, "shift", shift))
                        assert res.spmv_count == 1 + (degree - 1) + degree * k, (degree, k, every, res.spmv_count)
        xh, rh = A.pcg_host(P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        _same(KM.Got(xh, rh.iterations, rh.status, rh.residual_norm, rh.b_norm), tr.at(4), (degree, prec, "host"))
    finally:
        P.close()
        A.close()


def test_laplacian_to_1e_8_with_estimated_bounds():
    """the 24 x 24 Laplacian to rtol 1e-8, degree 4, bounds from cvr_chebyshev_bounds: the model's terminal entry whatever check_every is, fewer steps
    than plain CG on the same handle, and spmv_count by the formula with the steps enqueued (whole batches up to the stop)"""
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        lmin, lmax = A.chebyshev_bounds()
        assert 0 < lmin < lmax and 7.0 < lmax < 1.1 * 8.0, (lmin, lmax)
        P = capi.Precond.chebyshev(A, 4, lmin, lmax)
        b = synth.x_rand(n)
        tr = CM.ChebPcg(dev.product, np.float64, CM.Cheb(4, lmin, lmax, np.float64)).run(b, None, rtol=1e-8, max_iters=200)
        last = tr.last
        assert last.terminal and last.status == KM.CONVERGED, last
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = _solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            _same(got, last, ("check_every", every))
            assert res.spmv_count == 1 + 3 + 4 * enqueued, (every, res.spmv_count, enqueued)
        plain, _ = _solve(A, None, b, rtol=1e-8, max_iters=200)
        y, _ = O.csr_spmv64(rp, ci, va, got.x)
        true = float(np.linalg.norm(b - y) / np.linalg.norm(b))
        print(f"Chebyshev degree 4, bounds ({lmin:.4g}, {lmax:.4g}): {got.iterations} steps, plain CG {plain.iterations}; true residual {true:.3g}")
        assert plain.status == capi.CG_CONVERGED and got.iterations < plain.iterations
        assert true <= 2e-8
        P.close()
    finally:
        A.close()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_degree_one_on_fp64_is_cg_with_a_constant_minv(layout):
    n = 4097
    rp, ci, va, _, _ = _matrix("banded", n, np.float64)
    lmin, lmax = 0.45, 1.7          # (theta = 1.075: c0 is no power of two)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **LAYOUTS[layout])
    P = capi.Precond.chebyshev(A, 1, lmin, lmax)
    try:
        c0 = P.chebyshev_info()["b"][0]
        assert c0 == 1.0 / ((lmax + lmin) / 2)
        b, x0, _ = KM.inputs(n, np.float64)
        for start, kw in ((None, dict(rtol=1e-10, max_iters=60)), (x0, dict(rtol=0.0, max_iters=3, check_every=1)), (x0, dict(rtol=1e-10, max_iters=60, check_every=3))):
            ref, _ = _solve(A, None, b, start, minv=np.full(n, c0), **kw)
            got, _ = _solve(A, P, b, start, **kw)
            _same(got, ref, (layout, kw))
            assert ref.iterations > 0
        assert ref.status == capi.CG_CONVERGED
    finally:
        P.close()
        A.close()


# ---- stop states ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    dtype = _dtype(prec)
    n = 1025
    rp, ci, va, lmin, lmax = _matrix("banded", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.chebyshev(A, 3, lmin, lmax)
    try:
        b, x0, _ = KM.inputs(n, dtype)
        # a NaN in b: breakdown at step 0, x untouched
        bn = b.copy()
        bn[n // 2] = np.nan
        got, res = _solve(A, P, bn, x0, rtol=1e-6, max_iters=20)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status) == (0, capi.CG_BREAKDOWN)
        # b == 0: x = 0 whatever the start
        got, res = _solve(A, P, np.zeros(n), x0, rtol=1e-6, max_iters=20)
        assert not got.x.any() and (res.iterations, res.status, res.residual_norm, res.b_norm) == (0, capi.CG_CONVERGED, 0.0, 0.0)
        # max_iters = 0: the initial residual and the first apply
        got, res = _solve(A, P, b, x0, rtol=1e-6, max_iters=0)
        assert got.x.tobytes() == x0.tobytes() and (res.iterations, res.status, res.spmv_count) == (0, capi.CG_MAX_ITERS, 3)
        # ... and the object is as good as new behind the NaN (its buffers are rewritten by every apply)
        r = KM.inputs(n, dtype, seed=1)[0]
        assert _apply(P, r, dtype).tobytes() == CM.apply(Dev(A).product, r, 3, lmin, lmax, dtype).tobytes()
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("degree", [2, 4, 8])
def test_bounds_that_make_the_polynomial_indefinite(degree):
    """lmax = 0.2 * the true lambda_max of the 24 x 24 Laplacian: p_d(A) has negative eigenvalues, r.z changes sign and CG loses its footing.  The solve
    must end as CVR_CG_BREAKDOWN or CVR_CG_MAX_ITERS (the numpy model with the CPU product runs to max_iters at all three degrees), never fault and
    never report a wrong x as converged.  Where it does report convergence the true residual is held to 10 * rtol: the recurrence residual is within
    rtol, and the two drift apart by at most about iterations * 16 eps * ||A|| * max ||x_k|| = 200 * 16 * 2^-53 * 8 * max ||x_k|| = 2.8e-12 max ||x_k||,
    which reaches 9e-8 ||b|| only for iterates of 3e4 ||b||, a thousand times ||A^-1|| ||b||."""
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    lmax = 0.2 * 8 * np.cos(np.pi / 50) ** 2
    P = capi.Precond.chebyshev(A, degree, lmax / 30, lmax)
    try:
        b = synth.x_rand(n)
        got, res = _solve(A, P, b, rtol=1e-8, max_iters=200)
        y, _ = O.csr_spmv64(rp, ci, va, got.x.astype(np.float64))
        true = float(np.linalg.norm(b - y) / np.linalg.norm(b)) if np.isfinite(got.x).all() else np.inf
        print(f"degree {degree}: status {res.status} after {res.iterations} steps, recurrence residual {res.residual_norm / res.b_norm:.3g}, true {true:.3g}")
        assert res.status in (capi.CG_BREAKDOWN, capi.CG_MAX_ITERS, capi.CG_CONVERGED)
        if res.status == capi.CG_CONVERGED:
            assert true <= 1e-7
        # the handle and the object are unharmed: the next apply is the model's
        r = KM.inputs(n, np.float64)[0]
        assert _apply(P, r, np.float64).tobytes() == CM.apply(Dev(A).product, r, degree, lmax / 30, lmax, np.float64).tobytes()
    finally:
        P.close()
        A.close()


# ---- cvr_chebyshev_bounds ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", ["laplacian", "banded"])
def test_bounds_are_the_models(which, prec):
    """on the plain layout, where every sum of cvr_power_iteration is the dense tree's"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = synth.laplacian_2d(24, dtype) if which == "laplacian" else KM.banded("spd", 1025, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS["plain"])
    try:
        dev = Dev(A)
        for iters, ratio in ((20, 30.0), (3, 7.5)):
            lmin, lmax, lam = CM.bounds(dev.product, n, dtype, iters, ratio)
            got = A.chebyshev_bounds(iters, ratio)
            assert (np.float64(got[0]).tobytes(), np.float64(got[1]).tobytes()) == (lmin.tobytes(), lmax.tobytes()), (which, prec, iters, got, (lmin, lmax))
            assert lmax == np.float64(1.1) * lam and lam > 0
    finally:
        A.close()


# ---- a mutable handle ----
def test_a_mutable_handle_is_followed():
    n = 1025
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    v2 = (va * np.where(np.arange(len(va)) % 3 == 0, 0.5, 1.25)).astype(np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, mutable_values=1)
    P = capi.Precond.chebyshev(A, 4, 0.3, 2.0)
    try:
        assert A.update_values_supported()
        dev = Dev(A)
        r = KM.inputs(n, np.float64)[0]
        before = CM.apply(dev.product, r, 4, 0.3, 2.0, np.float64)
        assert _apply(P, r, np.float64).tobytes() == before.tobytes()
        A.update_values(v2)
        after = CM.apply(dev.product, r, 4, 0.3, 2.0, np.float64)          # (the product is the handle's: the new matrix)
        assert after.tobytes() != before.tobytes()
        assert _apply(P, r, np.float64).tobytes() == after.tobytes()
        assert P.chebyshev_info()["lmax"] == 2.0          # the bounds stay as given
    finally:
        P.close()
        A.close()


# ---- errors ----
def test_errors_of_the_constructor_and_of_the_bounds():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        p = C.c_void_p()
        assert L.cvr_precond_chebyshev(None, A._h, 2, 0.5, 1.5) == capi.ERR_INVALID
        assert L.cvr_precond_chebyshev(C.byref(p), None, 2, 0.5, 1.5) == capi.ERR_INVALID and not p.value
        for degree in (0, -1, capi.CHEBYSHEV_MAX_DEGREE + 1):
            assert L.cvr_precond_chebyshev(C.byref(p), A._h, degree, 0.5, 1.5) == capi.ERR_INVALID and "degree" in capi.last_error() and not p.value
        for lmin, lmax in ((0.0, 1.5), (-0.5, 1.5), (1.5, 1.5), (2.0, 1.5), (np.nan, 1.5), (0.5, np.nan), (0.5, np.inf), (-np.inf, 1.5)):
            assert L.cvr_precond_chebyshev(C.byref(p), A._h, 2, lmin, lmax) == capi.ERR_INVALID and "lmin" in capi.last_error() and not p.value
        # the largest degree is valid
        P = capi.Precond.chebyshev(A, capi.CHEBYSHEV_MAX_DEGREE, 0.5, 1.5)
        assert P.chebyshev_info()["degree"] == capi.CHEBYSHEV_MAX_DEGREE
        # r == z, null arguments of the apply
        rt = _put(np.ones(n), np.float64)
        assert L.cvr_precond_apply_device(P._p, rt.data_ptr(), rt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_apply_device(P._p, None, rt.data_ptr(), None) == capi.ERR_INVALID
        assert L.cvr_precond_chebyshev_info(P._p, None) == capi.ERR_INVALID and L.cvr_precond_chebyshev_info(None, C.byref(capi.ChebyshevInfo())) == capi.ERR_INVALID
        P.close()
        # the bounds
        lo, hi = C.c_double(-1.0), C.c_double(-1.0)
        assert L.cvr_chebyshev_bounds(None, 20, 30.0, C.byref(lo), C.byref(hi), None) == capi.ERR_INVALID
        assert L.cvr_chebyshev_bounds(A._h, 20, 30.0, None, C.byref(hi), None) == capi.ERR_INVALID
        assert L.cvr_chebyshev_bounds(A._h, -1, 30.0, C.byref(lo), C.byref(hi), None) == capi.ERR_INVALID
        for ratio in (1.0, 0.5, np.nan, np.inf):
            assert L.cvr_chebyshev_bounds(A._h, 20, ratio, C.byref(lo), C.byref(hi), None) == capi.ERR_INVALID and "eig_ratio" in capi.last_error()
        assert L.cvr_chebyshev_bounds(A._h, 0, 30.0, C.byref(lo), C.byref(hi), None) == capi.ERR_STATE          # lambda = 0 without a step
        assert (lo.value, hi.value) == (-1.0, -1.0)
    finally:
        A.close()
    # a negative definite matrix: lambda < 0
    N = cvr_amd.CvrMatrix(n, n, rp, ci, -va)
    try:
        with pytest.raises(capi.CvrError) as e:
            N.chebyshev_bounds()
        assert e.value.code == capi.ERR_STATE
    finally:
        N.close()
    # a rectangular handle
    R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, va)
    try:
        with pytest.raises(capi.CvrError) as e:
            capi.Precond.chebyshev(R, 2, 0.5, 1.5)
        assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            R.chebyshev_bounds()
        assert e.value.code == capi.ERR_INVALID
    finally:
        R.close()
    # before cvr_preprocess
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
    h, p = C.c_void_p(), C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    assert L.cvr_precond_chebyshev(C.byref(p), h, 2, 0.5, 1.5) == capi.ERR_STATE and "cvr_preprocess" in capi.last_error() and not p.value
    assert L.cvr_precond_chebyshev(C.byref(p), h, 0, 0.5, 1.5) == capi.ERR_INVALID          # (the argument checks come first)
    lo, hi = C.c_double(), C.c_double()
    assert L.cvr_chebyshev_bounds(h, 20, 30.0, C.byref(lo), C.byref(hi), None) == capi.ERR_STATE
    assert L.cvr_destroy(h) == 0


def test_mismatches_of_the_pair():
    """cvr_pcg_device's three checks hold for this kind; a second handle of the same n, type and device is taken"""
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.chebyshev(A, 3, 0.4, 1.6)
    b = synth.x_rand(n)
    try:
        _, _, rp2, ci2, va2 = KM.banded("spd", n + 1, np.float64)
        B = cvr_amd.CvrMatrix(n + 1, n + 1, rp2, ci2, va2)
        with pytest.raises(capi.CvrError) as e:
            _solve(B, P, synth.x_rand(n + 1), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        B.close()
        F = cvr_amd.CvrMatrix(n, n, rp, ci, va.astype(np.float32))
        with pytest.raises(capi.CvrError) as e:
            _solve(F, P, b, rtol=1e-4, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        F.close()
        bt, xt = _put(b, np.float64), _put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        capi.lib().cvr_cg_default_options(C.byref(opt))
        opt.minv_dev = bt.data_ptr()
        assert capi.lib().cvr_pcg_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()
        # another handle of the same matrix in another layout: the polynomial is in A, the solve on G -- the model with two products
        G = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS["plain"])
        tr = CM.ChebPcg(Dev(G).product, np.float64, CM.Cheb(3, 0.4, 1.6, np.float64), inner=Dev(A).product).run(b, None, rtol=0.0, max_iters=3)
        got, _ = _solve(G, P, b, rtol=0.0, max_iters=3)
        _same(got, tr.at(3), "two handles")
        G.close()
    finally:
        P.close()
        A.close()


def test_entry_points_that_take_block_jacobi_only():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.chebyshev(A, 3, 0.4, 1.6)
    J = capi.Precond.block_jacobi(rp, ci, va, 4)
    try:
        b = synth.x_rand(n)
        bt, xt = _put(b, np.float64), _put(np.zeros(n), np.float64)
        out = np.zeros(16)

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind" in capi.last_error() and "Chebyshev" in capi.last_error(), (name, capi.last_error())

        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), "apply_multi")
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), "pcg_multi_device")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), "pcg_multi")
        declined(L.cvr_pbicgstab_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None), "pbicgstab_device")
        declined(L.cvr_pbicgstab(A._h, P._p, hb.ctypes.data, hx.ctypes.data, C.byref(opt), C.byref(res)), "pbicgstab")
        declined(L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 10, C.byref(opt), C.byref(res), None), "pgmres_device")
        declined(L.cvr_pgmres(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 10, C.byref(opt), C.byref(res)), "pgmres")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any()          # nothing ran
        # behind their existing checks: a bad nvec is still CVR_ERR_INVALID
        assert L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 9, None) == capi.ERR_INVALID
        assert L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 0, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        # a block-Jacobi object is no Chebyshev object
        assert L.cvr_precond_chebyshev_info(J._p, C.byref(capi.ChebyshevInfo())) == capi.ERR_INVALID and "kind" in capi.last_error()
        with pytest.raises(capi.CvrError) as e:
            J.chebyshev_info()
        assert e.value.code == capi.ERR_INVALID
        # ... and still works where the Chebyshev object was declined
        got, res = _solve(A, J, b, rtol=1e-10, max_iters=60)
        assert res.status == capi.CG_CONVERGED
    finally:
        J.close()
        P.close()
        A.close()
