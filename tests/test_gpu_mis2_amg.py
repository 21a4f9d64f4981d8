"""GPU (MI355X): smoothed-aggregation AMG set up on the device with the MIS(2) aggregation -- cvr_amg_mis2_aggregate_device, cvr_precond_amg_mis2,
cvr_precond_amg_mis2_info and the smoothed kind's exports, apply and PCG on such an object, through the ABI, against tests/mis2_amg_model.py and
the host twin (cvr_amg_mis2_setup_host).

  * the aggregation alone on every named case (an unsymmetric pattern and a long chain among them), n = 0 and n = 1, fp64 and fp32: agg, nc and
    rounds are the model's; a non-zero first row pointer
  * the object from host arrays and from device arrays: levels, prolongators and the three infos byte for byte the model's and the host twin's;
    the same under CVR_DEBUG=mis2_check=1, =1000 and spgemm_limits=8:64 (fresh child processes)
  * the apply bit for bit the model's cycle through handles of the exported levels, twice in a row; the PCG step counts of the model
  * a bad diagonal on level 0 and a non-positive pivot on the coarsest level: CVR_ERR_STATE naming level and row, and a build after them works
  * the declines that name "kind 4 (AMG)", the info on objects built another way
The shapes: n = 0, n = 1, a level within one wavefront (singletons: 90 rows), levels that do not divide the workgroup (576, 1600 rows), a coarse
level with rows of a few dozen entries (level 1 of 40 x 40)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cvr_amd
import amg_model as AM
import krylov_model as KM
import mis2_amg_model as M
import pkrylov_gpu as G
import sa_amg_model as SA
import test_gpu_sa_amg as SAG          # its helpers: Levels (handles of exported levels), _apply, _same_exports, _solve
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {24: 19, 40: 19}          # the model's own counts, pinned in test_mis2_amg_model_host.py


def _export(P):
    return SAG._export(P) + (P.amg_mis2_info(),)


def _device(rp, ci, va):
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, va)]
    torch.cuda.synchronize()
    return t


def _aggregate_device(n, rp, ci, va, strength=0.08):
    t = _device(rp, ci, va)
    agg = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nc, rounds = capi.amg_mis2_aggregate_device(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), agg.data_ptr(), is_f32=va.dtype == np.float32, strength=strength)
    return agg.cpu().numpy()[:n], nc, rounds


# ---- the aggregation alone ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.AGGREGATION_CASES)
def test_the_device_aggregation_is_the_models(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    want, nc, rounds = M.cached_aggregate(name, dtype)
    got = _aggregate_device(n, rp, ci, va)
    assert (got[1], got[2]) == (nc, rounds), (name, prec, got[1:], nc, rounds)
    assert np.array_equal(got[0], want), (name, prec, np.flatnonzero(got[0] != want)[:5])


def test_the_device_aggregation_of_no_rows_one_row_and_a_shifted_row_pointer():
    agg, nc, rounds = _aggregate_device(0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert (len(agg), nc, rounds) == (0, 0, 0)
    agg, nc, rounds = _aggregate_device(1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([2.0]))
    assert (agg.tolist(), nc, rounds) == ([0], 1, 1)
    n, _, rp, ci, va = M.matrix("lopsided", np.float64)
    want = M.cached_aggregate("lopsided", np.float64)
    got = _aggregate_device(n, rp + 3, np.r_[np.zeros(3, dtype=np.int32), ci], np.r_[np.full(3, 9.0), va])
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    # another strength: everything is strong at 0
    lv = M.level_of("laplacian-24", np.float64)
    want = M.aggregate(lv, 0.0)
    got = _aggregate_device(lv.n, lv.rp, lv.ci, lv.va, strength=0.0)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    # the checks of device arrays: a row without its diagonal entry, columns out of order
    L = capi.lib()
    for cols, what in (([0, 0, 2, 2], "diagonal"), ([0, 2, 1, 2], "increasing")):
        t = _device(np.array([0, 1, 3, 4], dtype=np.int64), np.array(cols, dtype=np.int32), np.ones(4))
        out = torch.zeros(3, dtype=torch.int32, device="cuda")
        view = capi.CsrView(3, 3, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, 1)
        nc, rounds = C.c_int64(), C.c_int32()
        rc = L.cvr_amg_mis2_aggregate_device(C.byref(view), 0.08, out.data_ptr(), C.byref(nc), C.byref(rounds), 0, None)
        assert rc == capi.ERR_INVALID and "row 1" in capi.last_error() and what in capi.last_error() and "cvr_amg_mis2_aggregate_device" in capi.last_error(), capi.last_error()


# ---- the set-up ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", M.SETUP_CASES, ids=AM.case_id)
def test_levels_prolongators_and_infos_are_the_models_and_the_host_twins(case, prec):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    model = M.cached_setup(name, dtype, **options)
    assert model.bad is None
    twin = capi.amg_mis2_setup_host(rp, ci, va, **options)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    t = _device(rp + 2, np.r_[np.zeros(2, dtype=np.int32), ci], np.r_[np.ones(2, dtype=dtype), va])          # (the device arrays begin at row_ptr[0] = 2)
    P = capi.Precond.amg_mis2(A, rp, ci, va, **options)
    Q = capi.Precond.amg_mis2_from_device(A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=dtype == np.float32, **options)
    del t          # the object keeps nothing of the caller's arrays
    try:
        for obj, how in ((P, "host arrays"), (Q, "device arrays")):
            got = _export(obj)
            assert SA.same_hierarchy(model, *got[:4]) == "", (name, prec, how)
            assert M.same_rounds(model, got[4]) == "", (name, prec, how)
            assert SAG._same_exports(got[:4], twin[:4]) == "" and bytes(got[4]) == bytes(twin[4]), (name, prec, how)
            assert got[1].smoothed == 1 and obj.info.n == n
            again = _export(obj)          # (the second export reads the host copy the first one left)
            assert SAG._same_exports(got[:4], again[:4]) == ""
    finally:
        P.close()
        Q.close()
        A.close()


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
import cvr_amd
import mis2_amg_model as M
from cvr_amd import capi
out = {}
for name in sys.argv[4].split(","):
    for prec, dtype in (("fp64", np.float64), ("fp32", np.float32)):
        n, _, rp, ci, va = M.matrix(name, dtype)
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        P = capi.Precond.amg_mis2(A, rp, ci, va)
        info = P.amg_info()
        out[f"{name}/{prec}/levels"] = np.array([info.levels])
        out[f"{name}/{prec}/rounds"] = np.array(list(P.amg_mis2_info().rounds))
        for l in range(info.levels):
            e = P.amg_export_level(l)
            out[f"{name}/{prec}/A{l}/rp"], out[f"{name}/{prec}/A{l}/ci"], out[f"{name}/{prec}/A{l}/va"], out[f"{name}/{prec}/A{l}/dinv"] = e.rp, e.ci, e.va, e.dinv
            if l + 1 < info.levels:
                out[f"{name}/{prec}/A{l}/agg"] = e.agg
                p = P.amg_export_prolongator(l)
                out[f"{name}/{prec}/P{l}/rp"], out[f"{name}/{prec}/P{l}/ci"], out[f"{name}/{prec}/P{l}/va"] = p.rp, p.ci, p.va
        P.close()
        A.close()
np.savez(sys.argv[3], **out)
"""
CHILD_CASES = ["laplacian-24", "laplacian-40", "singletons"]


@pytest.mark.parametrize("setting", ["mis2_check=1", "mis2_check=1000", "spgemm_limits=8:64"])
def test_a_debug_setting_changes_no_bit_and_no_count(setting, tmp_path):
    path = str(tmp_path / "levels.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), path, ",".join(CHILD_CASES)], env=dict(os.environ, CVR_DEBUG=setting), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    for name in CHILD_CASES:
        for prec in ("fp64", "fp32"):
            H = M.cached_setup(name, G.dtype_of(prec))
            key = f"{name}/{prec}/"
            assert got[key + "levels"][0] == len(H.levels)
            assert got[key + "rounds"].tolist() == H.rounds + [0] * (AM.MAX_LEVELS - len(H.rounds)), (name, prec, setting)
            for l, lv in enumerate(H.levels):
                for f in ("rp", "ci", "va", "dinv") + (("agg",) if l + 1 < len(H.levels) else ()):
                    assert got[f"{key}A{l}/{f}"].tobytes() == getattr(lv, f).tobytes(), (name, prec, setting, "A", l, f)
            for l, p in enumerate(H.P):
                for f in ("rp", "ci", "va"):
                    assert got[f"{key}P{l}/{f}"].tobytes() == getattr(p, f).tobytes(), (name, prec, setting, "P", l, f)


# ---- the apply and the solver ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", [("laplacian-24", {}), ("singletons", {}), ("laplacian-40", dict(max_levels=2)), ("laplacian-24", dict(sweeps=2, coarse_scale=1.5))], ids=AM.case_id)
def test_the_apply_is_the_models_cycle_bit_for_bit(case, prec):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_mis2(A, rp, ci, va, **options)
    lv = SAG.Levels(A, P)
    try:
        info, sinfo = P.amg_info(), P.amg_smoothed_info()
        s = info.sweeps
        assert sinfo.products_per_apply == (2 * s + 2) * (info.levels - 1) + (0 if info.coarse_direct else 2 * s - 1) == lv.H.products_per_apply()
        r = KM.inputs(n, dtype)[0]
        want = lv.apply(r)
        assert np.isfinite(want).all() and want.any()
        for rshift, zshift in ((0, 0), (0, 0), (1, 1)):          # (twice in a row on the aligned arrays first)
            got = SAG._apply(P, r, dtype, rshift, zshift)
            assert got.tobytes() == want.tobytes(), (name, prec, rshift, zshift, SAG._first_difference(got, want))
    finally:
        lv.close()
        P.close()
        A.close()


@pytest.mark.parametrize("m", [24, 40])
def test_laplacian_to_1e_8_takes_the_models_steps(m):
    n, _, rp, ci, va = synth.laplacian_2d(m)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    t = _device(rp, ci, va)
    P = capi.Precond.amg_mis2_from_device(A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    lv = SAG.Levels(A, P)
    try:
        per_apply = P.amg_smoothed_info().products_per_apply
        assert per_apply == 8 and P.amg_info().levels == 3
        b = KM.inputs(n, np.float64)[0]
        last = SA.SaAmgPcg(lv.A[0], np.float64, lv.H, lv.A, lv.P, lv.R).run(b, None, rtol=1e-8, max_iters=200).last
        print(f"laplacian_2d({m}): MIS(2) smoothed AMG-PCG {last.iterations} steps")
        assert last.terminal and last.status == KM.CONVERGED and last.iterations == STEPS[m]
        for every, enqueued in ((1, last.iterations), (0, -(-last.iterations // 8) * 8)):
            got, res = SAG._solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, ("check_every", every))
            assert res.spmv_count == SAG._spmvs(per_apply, enqueued), (every, res.spmv_count, enqueued)
    finally:
        lv.close()
        P.close()
        A.close()


# ---- failures, declines, the smallest shapes ----
def test_failures_name_level_and_row_and_a_build_after_them_works():
    L = capi.lib()
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    p = C.c_void_p()
    try:
        # a bad diagonal on level 0, rows 7 and 300: the lowest is named; from host and from device arrays
        broken = va.copy()
        for row in (300, 7):
            broken[int(rp[row] + np.flatnonzero(ci[rp[row]: rp[row + 1]] == row)[0])] = -4.0
        t = _device(rp, ci, broken)
        for view in (capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, broken.ctypes.data, 0, 0), capi.CsrView(n, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, 1)):
            rc = L.cvr_precond_amg_mis2(C.byref(p), A._h, C.byref(view), None, 0.0, None)
            msg = capi.last_error()
            assert rc == capi.ERR_STATE and not p.value and "cvr_precond_amg_mis2" in msg and "level 0" in msg and "row 7 " in msg and "diagonal" in msg, msg
        # device arrays that break the structure rules: row 5 holds column 4 twice and no diagonal entry
        cols = ci.copy()
        cols[int(rp[5] + np.flatnonzero(ci[rp[5]: rp[6]] == 5)[0])] = 4          # (4, 4, 6, 29)
        t = _device(rp, cols, va)
        view = capi.CsrView(n, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, 1)
        assert L.cvr_precond_amg_mis2(C.byref(p), A._h, C.byref(view), None, 0.0, None) == capi.ERR_INVALID and "row 5" in capi.last_error() and not p.value, capi.last_error()
        # the options and omega first, as in the smoothed entry point
        ok = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
        o = capi.amg_options(sweeps=5)
        assert L.cvr_precond_amg_mis2(C.byref(p), A._h, C.byref(ok), C.byref(o), np.nan, None) == capi.ERR_INVALID and "sweeps" in capi.last_error()
        assert L.cvr_precond_amg_mis2(C.byref(p), A._h, C.byref(ok), None, 2.0, None) == capi.ERR_INVALID and "omega" in capi.last_error() and "cvr_precond_amg_mis2" in capi.last_error()
        # ... and a build after the failures works
        P = capi.Precond.amg_mis2(A, rp, ci, va)
        assert M.same_rounds(M.cached_setup("laplacian-24", np.float64), P.amg_mis2_info()) == ""
        P.close()
    finally:
        A.close()
    # a non-positive pivot on the coarsest level: an indefinite 3 x 3 matrix (level 0 is the coarsest), and the singular Neumann chain in fp32, whose
    # Galerkin matrix on level 1 loses its last pivot -- wherever the model finds it
    small = (np.array([0, 2, 4, 5], dtype=np.int64), np.array([0, 1, 0, 1, 2], dtype=np.int32), np.array([1.0, 2.0, 2.0, 1.0, 1.0]))
    m = 100
    D = np.zeros((m, m))
    for i in range(m - 1):
        D[i, i] += 1
        D[i + 1, i + 1] += 1
        D[i, i + 1] = D[i + 1, i] = -1
    chain = AM._csr_of_dense(D, np.float32)[2:]
    for rp, ci, va in (small, chain):
        n = len(rp) - 1
        H = M.setup(rp, ci, va, va.dtype)
        assert H.bad is not None and H.bad[2] == "pivot", H.bad
        A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
        try:
            with pytest.raises(capi.CvrError) as e:
                capi.Precond.amg_mis2(A, rp, ci, va)
            msg = str(e.value)
            assert e.value.code == capi.ERR_STATE and f"level {H.bad[0]}" in msg and f"row {H.bad[1]} " in msg and "pivot" in msg, (H.bad, msg)
            with pytest.raises(capi.CvrError) as e:
                capi.amg_mis2_setup_host(rp, ci, va)
            assert e.value.bad == H.bad[:2]
        finally:
            A.close()


def test_no_rows_one_row_the_declines_and_the_info_of_other_objects():
    L = capi.lib()
    # n = 1
    A = cvr_amd.CvrMatrix(1, 1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([4.0]))
    P = capi.Precond.amg_mis2(A, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([4.0]))
    info, sinfo, levels, pro, minfo = _export(P)
    assert (info.levels, info.coarse_direct, sinfo.smoothed, minfo.mis2, any(minfo.rounds), pro) == (1, 1, 1, 1, False, []) and levels[0].winv.ravel().tolist() == [0.25]
    assert SAG._apply(P, np.array([2.0]), np.float64).tolist() == [0.5]
    P.close()
    A.close()
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_mis2(A, rp, ci, va, omega=1.2)
    S = capi.Precond.amg_smoothed(A, rp, ci, va)
    plain = capi.Precond.amg(A, rp, ci, va)
    J = capi.Precond.block_jacobi(rp, ci, va, 4)
    try:
        assert P.amg_smoothed_info().omega == 1.2 and P.amg_smoothed_info().smoothed == 1 and P.amg_mis2_info().mis2 == 1
        for other in (S, plain):          # a kind-4 object built another way: all zero
            assert bytes(other.amg_mis2_info()) == bytes(C.sizeof(capi.AmgMis2Info))
        mi = capi.AmgMis2Info()
        assert L.cvr_precond_amg_mis2_info(J._p, C.byref(mi)) == capi.ERR_INVALID and "kind" in capi.last_error()
        assert L.cvr_precond_amg_mis2_info(P._p, None) == capi.ERR_INVALID and L.cvr_precond_amg_mis2_info(None, C.byref(mi)) == capi.ERR_INVALID
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx, out = b.copy(), np.zeros(n), np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE and "kind 4 (AMG)" in capi.last_error(), (name, rc, capi.last_error())

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
        levels = P.amg_info().levels
        p0 = P.amg_export_prolongator(0)
        args = (p0.rp.ctypes.data, p0.ci.ctypes.data, p0.va.ctypes.data)
        assert L.cvr_precond_amg_export_prolongator(P._p, levels - 1, *args) == capi.ERR_INVALID and "level" in capi.last_error()
        assert L.cvr_precond_amg_export_prolongator(P._p, -1, *args) == capi.ERR_INVALID
    finally:
        for o in (J, plain, S, P):
            o.close()
        A.close()
    # n = 0: one empty level
    Z = cvr_amd.CvrMatrix(0, 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    P0 = capi.Precond.amg_mis2(Z, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    info, sinfo, minfo = P0.amg_info(), P0.amg_smoothed_info(), P0.amg_mis2_info()
    assert (info.levels, info.coarse_direct, info.n[0], sinfo.smoothed, sinfo.products_per_apply, minfo.mis2, any(minfo.rounds)) == (1, 1, 0, 1, 0, 1, False)
    P0.close()
    Z.close()
