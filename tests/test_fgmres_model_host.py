"""The numpy model of cvr_fgmres_device (tests/fgmres_model.py) on the CPU: that it is GmresModel when nothing is applied, that it agrees with
right-preconditioned GMRES when M^-1 is one fixed matrix, that it still solves when M_j changes from step to step -- where forming x as M^-1 (V y)
does not -- and that the library exports the two entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import krylov_model as KM
import pkrylov_model as PK
import precond_model as PM
from cvr_amd import capi
from fgmres_model import FgmresModel, FixedFormModel
from gmres_model import GmresModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 60


def _banded60(dtype):
    n, _, rp, ci, va = KM.banded("nonsym", N, dtype)
    return rp, ci, va, PM.host_product(n, rp, ci, va, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identity_apply_gives_the_bits_of_gmres_model(dtype):
    rp, ci, va, prod = _banded60(dtype)
    b, x0, _ = KM.inputs(N, dtype)
    for start in (None, x0):
        for apply in (None, lambda k, v: v):
            for rtol, iters in ((0.0, 9), (1e-10 if dtype == np.float64 else 1e-4, 80)):
                got = FgmresModel(prod, dtype, apply, restart=4).run(b, start, rtol=rtol, max_iters=iters)
                ref = GmresModel(prod, dtype, restart=4).run(b, start, None, rtol=rtol, max_iters=iters)
                assert len(got.steps) == len(ref.steps)
                for k, (s, t) in enumerate(zip(got.steps, ref.steps)):
                    assert KM.compare(s, t) == "" and s.terminal == t.terminal, (k, KM.compare(s, t))
    assert ref.last.terminal and ref.last.status == KM.CONVERGED and ref.last.iterations > 4          # (across a restart)


def test_fixed_dense_m_agrees_with_right_preconditioned_gmres():
    """one dense M^-1 (the inverse of A's tridiagonal part, as a single block of pkrylov_model.PGmres): x = x0 + Z y and x = x0 + M^-1 (V y) are the same
    vector in exact arithmetic; the two models round differently (Z_i = T(M^-1 v_i) against M^-1 on the fp64 u), so they agree to rounding, not in bits"""
    dtype = np.float64
    rp, ci, va, prod = _banded60(dtype)
    A = PM.dense_of(N, rp, ci, va)
    W = np.linalg.inv(np.triu(np.tril(A, 1), -1)).reshape(1, N, N)
    b, x0, _ = KM.inputs(N, dtype)
    flex = FgmresModel(prod, dtype, lambda k, v: PM.apply(W, v, N, dtype), restart=5).run(b, x0, rtol=1e-10, max_iters=100)
    right = PK.PGmres(prod, dtype, W, N, restart=5).run(b, x0, rtol=1e-10, max_iters=100)
    plain = GmresModel(prod, dtype, restart=5).run(b, x0, None, rtol=1e-10, max_iters=100)
    assert flex.last.status == right.last.status == KM.CONVERGED and flex.last.iterations == right.last.iterations
    assert 5 < flex.last.iterations < plain.last.iterations          # (a restart is crossed; the preconditioner is one)
    for k, (s, t) in enumerate(zip(flex.steps, right.steps)):
        err = np.linalg.norm(s.x - t.x) / np.linalg.norm(t.x)
        assert err <= 1e-10, (k, err)
    print(f"fixed dense M: {flex.last.iterations} steps (plain {plain.last.iterations}), x of the two models {err:.3g} apart")


def _alternating():
    """M_j alternates between two diagonal matrices with entries in [0.5, 2) (seed 0), restart 8"""
    dtype = np.float64
    rp, ci, va, prod = _banded60(dtype)
    rng = np.random.default_rng(0)
    d = [0.5 + 1.5 * rng.random(N), 0.5 + 1.5 * rng.random(N)]
    b, x0, _ = KM.inputs(N, dtype)
    return prod, PM.dense_of(N, rp, ci, va), d, b, x0, (lambda k, v: (v.astype(np.float64) * d[k % 2]).astype(dtype))


def test_alternating_m_converges_on_the_true_residual_and_the_fixed_form_does_not():
    """Residuals below are relative to ||b||, the scale rtol is in.  The estimate and the true residual of the last iterate differ by the roundings of
    one cycle, a few 2^-53 ||b||: far inside 1e-8, but not inside 1e-8 of the residual itself (1e-10 ||b||), which no fp64 recurrence could promise.
    With x formed as D_0 (V y) or D_1 (V y) the estimate still falls below rtol -- the Arnoldi relation does not care how x is formed -- while the true
    residual of what is returned stays at 3.1e-7 ||b|| with D_0; with D_1 the restarts, which start from that x, diverge (200 steps, no stop)."""
    rtol = 1e-10
    prod, A, d, b, x0, apply = _alternating()
    bn = np.linalg.norm(b)
    flex = FgmresModel(prod, np.float64, apply, restart=8).run(b, x0, rtol=rtol, max_iters=200).last
    true = np.linalg.norm(b - A @ flex.x) / bn
    print(f"alternating M: {flex.iterations} steps, estimate {flex.residual_norm / bn:.6e}, true {true:.6e}")
    assert flex.status == KM.CONVERGED and flex.iterations > 8
    assert true < rtol
    assert abs(flex.residual_norm / bn - true) <= 1e-8
    for i in (0, 1):
        fixed = FixedFormModel(prod, np.float64, apply, lambda u: d[i] * u, restart=8).run(b, x0, rtol=rtol, max_iters=200).last
        ftrue = np.linalg.norm(b - A @ fixed.x) / bn
        print(f"x = D_{i} (V y): {fixed.iterations} steps, status {fixed.status}, estimate {fixed.residual_norm / bn:.3e}, true {ftrue:.3e}")
        assert ftrue > 100 * rtol, (i, ftrue)
        assert abs(fixed.residual_norm / bn - ftrue) > 1e-8, i


def test_library_exports_the_two_entry_points():
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library is not built")
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = C.CDLL(capi.lib_path())
    for s in ("cvr_fgmres_device", "cvr_fgmres"):
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert re.search(r"typedef int \(\*cvr_apply_fn\)\(void \*ctx, const void \*v_dev, void \*z_dev, int64_t n, void \*stream\);", hdr)
    assert C.sizeof(capi.APPLY_FN) == C.sizeof(C.c_void_p)
    for name in ("fgmres", "fgmres_host"):
        assert hasattr(capi.CvrMatrix, name), name


def test_arguments_declined_before_the_handle_is_looked_at():
    """the checks in front of any device work: a null handle, p and fn both set, minv_dev beside either or alone, restart out of range"""
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library is not built")
    L = capi.lib()
    opt, res = capi.CgOptions(), capi.CgResult()
    L.cvr_cg_default_options(C.byref(opt))
    buf = (C.c_double * 4)()
    fake = C.cast(buf, C.c_void_p)          # stands for a handle / an object: never dereferenced by the checks that fail here
    fn = capi.APPLY_FN(lambda ctx, v, z, n, st: 0)
    none = capi.APPLY_FN()

    def call(h, p, f, restart=4):
        return L.cvr_fgmres_device(h, p, f, None, fake, fake, restart, C.byref(opt), C.byref(res), None)

    assert call(None, None, none) == capi.ERR_INVALID and "null" in capi.last_error()
    assert call(fake, fake, fn) == capi.ERR_INVALID and "both" in capi.last_error() and "cvr_fgmres" in capi.last_error()
    opt.minv_dev = C.addressof(buf)
    for p, f in ((fake, none), (None, fn), (None, none)):
        assert call(fake, p, f) == capi.ERR_INVALID and "minv_dev" in capi.last_error(), (p, f)
    opt.minv_dev = None
    for restart in (0, capi.GMRES_MAX_RESTART + 1):
        assert call(fake, None, fn, restart) == capi.ERR_INVALID and "restart" in capi.last_error(), restart
    assert L.cvr_fgmres(fake, None, none, None, fake, fake, 0, C.byref(opt), C.byref(res)) == capi.ERR_INVALID and "restart" in capi.last_error()
