"""GPU (MI355X): smoothed-aggregation AMG -- cvr_precond_amg_smoothed, cvr_precond_amg_smoothed_info, cvr_precond_amg_export_prolongator, and
cvr_precond_apply_device / cvr_pcg with such an object, through the ABI, against tests/sa_amg_model.py and the host twin.

  * every level and every prolongator byte for byte against the model and against cvr_amg_smoothed_setup_host, fp64 and fp32, from host and from
    device arrays, on the Laplacians 24 x 24 and 23 x 23 and on singletons among coupled rows; the same bytes under CVR_DEBUG=spgemm_limits=8:64 and
    =1:1 (fresh child processes): all three row classes of the SpGEMM build the hierarchy
  * the apply bit for bit against the model's cycle carried out by the test: the products through handles the test makes of the exported A_l, P_l
    and P_l's numpy transpose; sweeps 1 and 2, coarse_scale 1.0 and 1.5, a smoothed coarsest level (max_levels = 2 on 40 x 40); r and z off the
    16-byte grid; the apply repeated
  * PCG step by step against the model, the pinned step counts to 1e-8 on 24 x 24 and 40 x 40, spmv_count = 1 + P + (1 + P) * (steps enqueued)
    with P = (2 * sweeps + 2) * (levels - 1), the result independent of check_every
  * the declines (naming "kind 4 (AMG)"), the new calls on a plain AMG object and on a block-Jacobi object, the handle mismatches"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cvr_amd
import krylov_model as KM
import pkrylov_gpu as G
import sa_amg_model as SA
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETUP_CASES = ["laplacian-24", "laplacian-23", "singletons"]
STEPS = {24: 14, 40: 16}          # the model's own counts, pinned in test_sa_amg_model_host.py


class RectDev:
    """a handle of any shape with the buffers of a product: x (ncols values and the pad), y (the handle's yext_elems)"""

    def __init__(self, H, nrows, ncols):
        self.H, self.nrows, self.ncols = H, nrows, ncols
        self.xbuf = torch.zeros(max(H.info.x_elems, ncols + 1), dtype=G.tdt(H.dtype), device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, nrows, 1), dtype=G.tdt(H.dtype), device="cuda")

    def product(self, x):
        self.xbuf[: self.ncols].copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.nrows].cpu().numpy()


def _export(P):
    info, sinfo = P.amg_info(), P.amg_smoothed_info()
    return info, sinfo, [P.amg_export_level(l) for l in range(info.levels)], [P.amg_export_prolongator(l) for l in range(info.levels - 1)]


class Levels:
    """what a caller makes of an object's exports: the model's Hierarchy and handles of A_l (l >= 1), P_l and R_l = P_l^T (numpy's transpose),
    made as the object makes its own (device arrays, the default options); level 0's product is the borrowed handle's"""

    def __init__(self, A, P):
        info, sinfo, exp, pro = _export(P)
        self.H = SA.from_export(info, sinfo, exp, pro, P.dtype)
        self.handles, self.keep = [], []
        self.A = [G.Dev(A).product]
        for l, e in enumerate(exp[1:], 1):
            self.A.append(None if l == info.levels - 1 and info.coarse_direct else self._handle(e.n, e.n, e.rp, e.ci, e.va))
        self.P = [self._handle(p.nrows, p.ncols, p.rp, p.ci, p.va) for p in self.H.P]
        self.R = [self._handle(r.nrows, r.ncols, r.rp, r.ci, r.va) for r in self.H.R]

    def _handle(self, nrows, ncols, rp, ci, va):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, va)]
        torch.cuda.synchronize()
        self.keep.append(t)
        h = cvr_amd.CvrMatrix.from_device(nrows, ncols, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=va.dtype == np.float32)
        self.handles.append(h)
        return RectDev(h, nrows, ncols).product

    def apply(self, r):
        return SA.apply(self.H, self.A, self.P, self.R, r)

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


def _same_exports(a, b):
    """two exports (info, sinfo, levels, prolongators) byte for byte"""
    if a[0].levels != b[0].levels or bytes(a[1]) != bytes(b[1]):
        return "the infos differ"
    for l, (x, y) in enumerate(zip(a[2], b[2])):
        for f in ("rp", "ci", "va", "dinv", "agg", "winv"):
            u, v = getattr(x, f), getattr(y, f)
            if (u is None) != (v is None) or (u is not None and u.tobytes() != v.tobytes()):
                return f"level {l}: {f}"
    for l, (x, y) in enumerate(zip(a[3], b[3])):
        for f in ("rp", "ci", "va"):
            if getattr(x, f).tobytes() != getattr(y, f).tobytes():
                return f"P_{l}: {f}"
    return ""


# ---- the set-up ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SETUP_CASES)
def test_levels_and_prolongators_are_the_models_and_the_host_twins(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = SA.matrix(name, dtype)
    model = SA.cached_setup(name, dtype)
    assert model.bad is None and len(model.levels) >= 2
    twin = capi.amg_smoothed_setup_host(rp, ci, va)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.amg_smoothed(A, rp, ci, va)
    Q = capi.Precond.amg_smoothed_from_device(A, n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), is_f32=dtype == np.float32)
    del rt, ct, vt          # the object keeps nothing of the caller's arrays
    try:
        for obj, how in ((P, "host arrays"), (Q, "device arrays")):
            got = _export(obj)
            assert SA.same_hierarchy(model, *got) == "", (name, prec, how)
            assert _same_exports(got, twin) == "", (name, prec, how)
            pi = obj.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks) == (n, 0, int(dtype == np.float32), 0, 0)
    finally:
        P.close()
        Q.close()
        A.close()


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import cvr_amd
import sa_amg_model as SA
from cvr_amd import capi
out = {}
for name in sys.argv[4].split(","):
    for prec, dtype in (("fp64", np.float64), ("fp32", np.float32)):
        n, _, rp, ci, va = SA.matrix(name, dtype)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        P = capi.Precond.amg_smoothed(A, rp, ci, va)
        info = P.amg_info()
        out[f"{name}/{prec}/levels"] = np.array([info.levels])
        for l in range(info.levels):
            e = P.amg_export_level(l)
            out[f"{name}/{prec}/A{l}/rp"], out[f"{name}/{prec}/A{l}/ci"], out[f"{name}/{prec}/A{l}/va"], out[f"{name}/{prec}/A{l}/dinv"] = e.rp, e.ci, e.va, e.dinv
            if l + 1 < info.levels:
                p = P.amg_export_prolongator(l)
                out[f"{name}/{prec}/P{l}/rp"], out[f"{name}/{prec}/P{l}/ci"], out[f"{name}/{prec}/P{l}/va"] = p.rp, p.ci, p.va
        P.close()
        A.close()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("limits", [(8, 64), (1, 1)], ids=["8:64", "1:1"])
def test_a_lowered_spgemm_plan_builds_the_same_hierarchy(limits, tmp_path):
    path = str(tmp_path / "levels.npz")
    env = dict(os.environ, CVR_DEBUG=f"spgemm_limits={limits[0]}:{limits[1]}")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), path, ",".join(SETUP_CASES)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    for name in SETUP_CASES:
        for prec in ("fp64", "fp32"):
            H = SA.cached_setup(name, G.dtype_of(prec))
            key = f"{name}/{prec}/"
            assert got[key + "levels"][0] == len(H.levels)
            for l, lv in enumerate(H.levels):
                for f in ("rp", "ci", "va", "dinv"):
                    assert got[f"{key}A{l}/{f}"].tobytes() == getattr(lv, f).tobytes(), (name, prec, limits, "A", l, f)
            for l, p in enumerate(H.P):
                for f in ("rp", "ci", "va"):
                    assert got[f"{key}P{l}/{f}"].tobytes() == getattr(p, f).tobytes(), (name, prec, limits, "P", l, f)


# ---- the apply ----
APPLY_CASES = [("laplacian-24", {}), ("laplacian-23", {}), ("singletons", {}), ("laplacian-24", dict(sweeps=2)), ("laplacian-24", dict(coarse_scale=1.5)),
               ("laplacian-23", dict(sweeps=2, coarse_scale=1.5)), ("laplacian-40", dict(max_levels=2))]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", APPLY_CASES, ids=lambda c: c[0] + "".join(f",{k}={v}" for k, v in c[1].items()))
def test_the_apply_is_the_models_cycle_bit_for_bit(case, prec):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = SA.matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_smoothed(A, rp, ci, va, **options)
    lv = Levels(A, P)
    try:
        info, sinfo = P.amg_info(), P.amg_smoothed_info()
        s = info.sweeps
        assert sinfo.products_per_apply == (2 * s + 2) * (info.levels - 1) + (0 if info.coarse_direct else 2 * s - 1) == lv.H.products_per_apply()
        if options.get("max_levels") == 2:
            assert (info.levels, info.coarse_direct, info.n[1]) == (2, 0, 280)          # the coarsest level is smoothed, not inverted
        r = KM.inputs(n, dtype)[0]
        want = lv.apply(r)
        assert np.isfinite(want).all() and want.any()
        for rshift, zshift in ((0, 0), (0, 0), (1, 0), (0, 1), (1, 1)):          # (twice in a row on the aligned arrays first)
            got = _apply(P, r, dtype, rshift, zshift)
            assert got.tobytes() == want.tobytes(), (name, prec, rshift, zshift, _first_difference(got, want))
    finally:
        lv.close()
        P.close()
        A.close()


# ---- the solver ----
def _solve(H, P, b, x0=None, shift=0, **kw):
    bt = G.put(b, H.dtype, shift)
    xt = G.put(np.zeros(H.nrows) if x0 is None else x0, H.dtype, shift)
    torch.cuda.synchronize()
    res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _spmvs(per_apply, steps):
    return 1 + per_apply + (1 + per_apply) * steps


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["laplacian-24", "singletons"])
def test_pcg_step_by_step_against_the_model(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = SA.matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_smoothed(A, rp, ci, va)
    lv = Levels(A, P)
    try:
        per_apply = P.amg_smoothed_info().products_per_apply
        b, x0, _ = KM.inputs(n, dtype)
        for start_name, start in (("zero", None), ("random", x0)):
            tr = SA.SaAmgPcg(lv.A[0], dtype, lv.H, lv.A, lv.P, lv.R).run(b, start, rtol=0.0, max_iters=4)
            for k in range(5):
                if k >= len(tr.steps) and not tr.last.terminal:
                    break
                for every in (1, 3, 0):
                    for shift in (0, 1):
                        got, res = _solve(A, P, b, start, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                        G.same(got, tr.at(k), (name, prec, start_name, "max_iters", k, "check_every", every, "shift", shift))
                        if got.status == capi.CG_MAX_ITERS:
                            assert res.spmv_count == _spmvs(per_apply, k), (k, every, res.spmv_count)
        x, r = A.pcg_host(P, b, x0=x0, rtol=0.0, max_iters=4)          # the host twin
        G.same(KM.Got(x, r.iterations, r.status, r.residual_norm, r.b_norm), tr.at(4), (name, prec, "host"))
    finally:
        lv.close()
        P.close()
        A.close()


@pytest.mark.parametrize("m", [24, 40])
def test_laplacian_to_1e_8_takes_the_pinned_steps(m):
    n, _, rp, ci, va = synth.laplacian_2d(m)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_smoothed(A, rp, ci, va)
    lv = Levels(A, P)
    try:
        per_apply = P.amg_smoothed_info().products_per_apply
        assert per_apply == 8 and P.amg_info().levels == 3
        b = KM.inputs(n, np.float64)[0]
        last = SA.SaAmgPcg(lv.A[0], np.float64, lv.H, lv.A, lv.P, lv.R).run(b, None, rtol=1e-8, max_iters=200).last
        print(f"laplacian_2d({m}): smoothed AMG-PCG {last.iterations} steps")
        assert last.terminal and last.status == KM.CONVERGED and last.iterations == STEPS[m]
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8)):
            got, res = _solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, ("check_every", every))
            assert res.spmv_count == _spmvs(per_apply, enqueued), (every, res.spmv_count, enqueued)
    finally:
        lv.close()
        P.close()
        A.close()


# ---- declines, cross-kind calls, mismatches ----
def test_declines_cross_kind_calls_and_mismatches():
    L = capi.lib()
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_smoothed(A, rp, ci, va, omega=1.2)
    plain = capi.Precond.amg(A, rp, ci, va)
    J = capi.Precond.block_jacobi(rp, ci, va, 4)
    try:
        assert P.amg_smoothed_info().omega == 1.2 and P.info.n == n
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind 4 (AMG)" in capi.last_error(), (name, capi.last_error())

        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), "apply_multi")
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), "pcg_multi_device")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), "pcg_multi")
        declined(L.cvr_pbicgstab_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(res), None), "pbicgstab_device")
        declined(L.cvr_pbicgstab(A._h, P._p, hb.ctypes.data, hx.ctypes.data, C.byref(opt), C.byref(res)), "pbicgstab")
        declined(L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 30, C.byref(opt), C.byref(res), None), "pgmres_device")
        declined(L.cvr_pgmres(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 30, C.byref(opt), C.byref(res)), "pgmres")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran
        # the new calls on a plain AMG object: the info all zero, no prolongator; on a block-Jacobi object: CVR_ERR_INVALID
        si = plain.amg_smoothed_info()
        assert bytes(si) == bytes(C.sizeof(capi.AmgSmoothedInfo))
        p0 = P.amg_export_prolongator(0)
        args = (p0.rp.ctypes.data, p0.ci.ctypes.data, p0.va.ctypes.data)
        assert L.cvr_precond_amg_export_prolongator(plain._p, 0, *args) == capi.ERR_INVALID and "plain" in capi.last_error()
        assert L.cvr_precond_amg_smoothed_info(J._p, C.byref(capi.AmgSmoothedInfo())) == capi.ERR_INVALID and "kind" in capi.last_error()
        assert L.cvr_precond_amg_export_prolongator(J._p, 0, *args) == capi.ERR_INVALID and "kind" in capi.last_error()
        levels = P.amg_info().levels
        assert L.cvr_precond_amg_export_prolongator(P._p, levels - 1, *args) == capi.ERR_INVALID and "level" in capi.last_error()          # the coarsest
        assert L.cvr_precond_amg_export_prolongator(P._p, -1, *args) == capi.ERR_INVALID
        assert L.cvr_precond_amg_export_prolongator(P._p, 0, None, args[1], args[2]) == capi.ERR_INVALID
        assert L.cvr_precond_amg_smoothed_info(P._p, None) == capi.ERR_INVALID and L.cvr_precond_amg_smoothed_info(None, C.byref(si)) == capi.ERR_INVALID
        # the constructor's checks in cvr_precond_amg's order: options, omega, the view against the handle
        view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
        p = C.c_void_p()
        for omega in (np.nan, -0.5, 2.0, np.inf):
            assert L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(view), None, omega, None) == capi.ERR_INVALID and "omega" in capi.last_error() and not p.value
        o = capi.amg_options(sweeps=5)
        assert L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(view), C.byref(o), np.nan, None) == capi.ERR_INVALID and "sweeps" in capi.last_error()
        n2, _, rp2, ci2, va2 = synth.laplacian_2d(25)
        v2 = capi.CsrView(n2, n2, rp2.ctypes.data, ci2.ctypes.data, va2.ctypes.data, 0, 0)
        assert L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(v2), None, 0.0, None) == capi.ERR_INVALID and "nrows" in capi.last_error()
        va32 = va.astype(np.float32)
        v3 = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va32.ctypes.data, 1, 0)
        assert L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(v3), None, 0.0, None) == capi.ERR_INVALID and "type" in capi.last_error()
        # ... and of the solver: n and type of the pair
        A2 = cvr_amd.CvrMatrix(n2, n2, rp2, ci2, va2)
        F = cvr_amd.CvrMatrix(n, n, rp, ci, va32)
        with pytest.raises(capi.CvrError) as e:
            _solve(A2, P, np.ones(n2), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            _solve(F, P, np.ones(n), rtol=1e-8, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        A2.close()
        F.close()
        # a bad diagonal: CVR_ERR_STATE naming level and row, no object
        broken = va.copy()
        broken[int(rp[7] + np.flatnonzero(ci[rp[7]: rp[8]] == 7)[0])] = -4.0
        vb = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, broken.ctypes.data, 0, 0)
        assert L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(vb), None, 0.0, None) == capi.ERR_STATE and "level 0" in capi.last_error() and "row 7 " in capi.last_error()
        assert not p.value
    finally:
        J.close()
        plain.close()
        P.close()
        A.close()
