"""GPU (MI355X): the MIS(2) aggregation and the smoothed-aggregation set-up on the device where tests/test_gpu_mis2_amg.py leaves them unrun, on the
cases of mis2_amg_model.IRREGULAR (held to their conditions, and shown to tell ten mutants apart, by tests/test_mis2_amg_model_host.py):

  * levels of more rows than one grid of 1024 x 256 threads (262 143, 262 144, 262 145 and 513^2 = 263 169 rows): the second trip of the row
    kernels, lanes of one wavefront with different trip counts in front of the m2 reduction, a scan of the root flags over many blocks, a device
    transpose of 263 169 entries, the SpGEMM's group kernel beyond 131 072 rows;
  * rows whose 31 hash bits agree (ties-62290, ties-grid-513): the key's index bits decide;
  * magnitudes that differ inside a row, equal ones beside them, a strong graph that is not symmetric, at 3000 rows and inside a set-up;
  * a row of 2000 entries under the one-thread-a-row kernels and, in star-2000's Galerkin products, block and spill rows under the default limits.
Everything is compared byte for byte: with the numpy model where it is quick enough, with the host twin (pinned to the model on the CPU) at 513^2."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cvr_amd
import amg_model as AM
import krylov_model as KM
import mis2_amg_model as M
import pkrylov_gpu as G
import sa_amg_model as SA
import test_gpu_mis2_amg as MG          # its helpers: _export, _device, _aggregate_device, CHILD
import test_gpu_sa_amg as SAG           # Levels, _apply, _same_exports, _solve
from cvr_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = "ties-grid-513"
STEPS = {"irr-spd-3000": 21, "star-2000": 17}          # the model's own counts with the CPU products, as the CPU run of this file's model printed them


@functools.lru_cache(maxsize=None)
def _twin(name, prec):
    """the host twin's hierarchy, computed once, shared, never changed"""
    n, _, rp, ci, va = M.matrix(name, G.dtype_of(prec))
    return capi.amg_mis2_setup_host(rp, ci, va)


# ---- 1. the aggregation alone ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.IRREGULAR_CASES)
def test_the_device_aggregation_is_the_models(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    want, nc, rounds = M.cached_aggregate(name, dtype)
    got = MG._aggregate_device(n, rp, ci, va)          # (agg is prefilled with -7: a row that no trip reached shows)
    assert (got[1], got[2]) == (nc, rounds), (name, prec, got[1:], nc, rounds)
    assert np.array_equal(got[0], want), (name, prec, np.flatnonzero(got[0] != want)[:5])
    if name == BIG:          # a first row pointer of 3
        got = MG._aggregate_device(n, rp + 3, np.r_[np.zeros(3, dtype=np.int32), ci], np.r_[np.full(3, 9.0).astype(dtype), va])
        assert (got[1], got[2]) == (nc, rounds) and np.array_equal(got[0], want), (name, prec, "row_ptr[0] = 3")


# ---- 2. the set-up where the model computes the whole hierarchy ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES)
def test_levels_prolongators_and_infos_are_the_models_and_the_host_twins(name, prec):
    """(the object's SpGEMM classes are not visible through the ABI: that star-2000's products hold block and spill rows under the default limits is
    asserted on the CPU, test_the_stars_products_reach_the_block_and_the_spill_class; the bytes are what is compared here)"""
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    model = M.cached_setup(name, dtype)
    assert model.bad is None
    twin = _twin(name, prec)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    t = MG._device(rp + 2, np.r_[np.zeros(2, dtype=np.int32), ci], np.r_[np.ones(2, dtype=dtype), va])
    P = capi.Precond.amg_mis2(A, rp, ci, va)
    Q = capi.Precond.amg_mis2_from_device(A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=dtype == np.float32)
    del t
    try:
        for obj, how in ((P, "host arrays"), (Q, "device arrays")):
            got = MG._export(obj)
            assert SA.same_hierarchy(model, *got[:4]) == "", (name, prec, how)
            assert M.same_rounds(model, got[4]) == "", (name, prec, how)
            assert SAG._same_exports(got[:4], twin[:4]) == "" and bytes(got[4]) == bytes(twin[4]), (name, prec, how)
    finally:
        P.close()
        Q.close()
        A.close()


@pytest.mark.parametrize("setting", ["spgemm_limits=8:64", "mis2_check=1"])
def test_a_debug_setting_changes_no_bit_and_no_count(setting, tmp_path):
    path = str(tmp_path / "levels.npz")
    r = subprocess.run([sys.executable, "-c", MG.CHILD, ROOT, os.path.join(ROOT, "tests"), path, ",".join(M.IRREGULAR_SETUP_CASES)], env=dict(os.environ, CVR_DEBUG=setting),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(path)
    for name in M.IRREGULAR_SETUP_CASES:
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


# ---- 3. the set-up of 513^2 rows ----
@pytest.mark.parametrize("prec,how", [("fp64", "host arrays"), ("fp32", "device arrays")])
def test_the_setup_of_the_grid_beyond_one_trip_is_the_host_twins(prec, how):
    """Against cvr_amg_mis2_setup_host, not against the Python model: the model's SpGEMM is a Python loop over every product and far too slow at
    263 169 rows.  The model still pins level 0's agg, nc, rounds and dinv here, and the twin is pinned to the model on the 3000- and 2000-row cases
    and on every older one by tests/test_mis2_amg_host.py."""
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(BIG, dtype)
    twin = _twin(BIG, prec)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    if how == "host arrays":
        P = capi.Precond.amg_mis2(A, rp, ci, va)
    else:
        t = MG._device(rp, ci, va)
        P = capi.Precond.amg_mis2_from_device(A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=dtype == np.float32)
        del t
    try:
        got = MG._export(P)
        assert SAG._same_exports(got[:4], twin[:4]) == "" and bytes(got[4]) == bytes(twin[4]), (prec, how)
        assert bytes(got[0]) == bytes(twin[0])
        assert got[0].levels >= 3 and got[0].n[0] == n > M.GRID_THREADS
        agg, nc, rounds = M.cached_aggregate(BIG, dtype)
        lv = AM.Level(n, rp, ci, va)
        assert np.array_equal(got[2][0].agg, agg) and got[0].n[1] == nc and got[4].rounds[0] == rounds
        assert got[2][0].dinv.tobytes() == AM.smoother_diagonal(lv, dtype)[0].tobytes()
    finally:
        P.close()
        A.close()


# ---- 4. the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES + [BIG])
def test_the_apply_is_the_models_cycle_bit_for_bit(name, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = M.matrix(name, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_mis2(A, rp, ci, va)
    lv = SAG.Levels(A, P)
    try:
        info, sinfo = P.amg_info(), P.amg_smoothed_info()
        assert sinfo.products_per_apply == 4 * (info.levels - 1) + (0 if info.coarse_direct else 1) == lv.H.products_per_apply()
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


# ---- 5. the solver ----
@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES)
def test_pcg_step_by_step_and_to_1e_8(name):
    n, _, rp, ci, va = M.matrix(name, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.amg_mis2(A, rp, ci, va)
    lv = SAG.Levels(A, P)
    try:
        per_apply = P.amg_smoothed_info().products_per_apply
        b = KM.inputs(n, np.float64)[0]
        model = SA.SaAmgPcg(lv.A[0], np.float64, lv.H, lv.A, lv.P, lv.R)
        tr = model.run(b, None, rtol=0.0, max_iters=4)
        for k in range(5):
            got, res = SAG._solve(A, P, b, rtol=0.0, max_iters=k, check_every=1)
            G.same(got, tr.at(k), (name, "max_iters", k))
            if got.status == capi.CG_MAX_ITERS:
                assert res.spmv_count == SAG._spmvs(per_apply, k), (k, res.spmv_count)
        last = model.run(b, None, rtol=1e-8, max_iters=200).last
        print(f"{name}: MIS(2) smoothed AMG-PCG {last.iterations} steps to 1e-8")
        assert last.terminal and last.status == KM.CONVERGED and last.iterations == STEPS[name]
        for every in (1, 0):
            got, res = SAG._solve(A, P, b, rtol=1e-8, max_iters=200, check_every=every)
            G.same(got, last, (name, "check_every", every))
    finally:
        lv.close()
        P.close()
        A.close()


# ---- 6. a failure ----
def test_the_lowest_of_two_bad_diagonals_is_named_and_a_build_after_it_works():
    L = capi.lib()
    name = "irr-spd-3000"
    n, _, rp, ci, va = M.matrix(name, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    p = C.c_void_p()
    try:
        broken = va.copy()
        for row in (2900, 41):
            broken[int(rp[row] + np.flatnonzero(ci[rp[row]: rp[row + 1]] == row)[0])] = -4.0
        assert M.setup(rp, ci, broken, np.float64, max_levels=1).bad == (0, 41, "diagonal")
        t = MG._device(rp, ci, broken)
        for view in (capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, broken.ctypes.data, 0, 0), capi.CsrView(n, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, 1)):
            rc = L.cvr_precond_amg_mis2(C.byref(p), A._h, C.byref(view), None, 0.0, None)
            msg = capi.last_error()
            assert rc == capi.ERR_STATE and not p.value and "cvr_precond_amg_mis2" in msg and "level 0" in msg and "row 41 " in msg and "diagonal" in msg, msg
        P = capi.Precond.amg_mis2(A, rp, ci, va)
        try:
            assert M.same_rounds(M.cached_setup(name, np.float64), P.amg_mis2_info()) == ""
            assert SAG._same_exports(MG._export(P)[:4], _twin(name, "fp64")[:4]) == ""
        finally:
            P.close()
    finally:
        A.close()
