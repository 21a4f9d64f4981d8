"""GPU (MI355X): ILU(0) with Jacobi-swept triangular solves -- cvr_precond_ilu0_jacobi, cvr_precond_ilu0_jacobi_info, and cvr_precond_apply_device /
cvr_pcg / cvr_pbicgstab / cvr_pgmres with such an object, all through the ABI, against tests/ilu_jacobi_model.py (the device is compared with the
model, and with the exact object where the two must agree; the model is never compared with itself).

  * the apply byte for byte against the model, fp32 and fp64, s = 1 .. 4 (both parities of the y and of the z buffers): the 8 x 8 Laplacian, the
    irregular cases with G = 2, 4, 32 and 64, the wide matrix (n = 4097, G = 1: 17 workgroups, the last one of a single row), r and z off the 16-byte grid
    one at a time, every apply repeated; CVR_DEBUG=ilu_lanes = 1 and 64 on irr-spd-700
  * with s = max(levels) the swept object and an exact Precond.ilu0 object give the same bits, device against device; the exported factors are
    the exact object's; r1, r2, r1 again gives the first result again
  * n = 0, n = 1, a diagonal matrix (z = T(r / d)), a chain with a row of 200 lower entries (G = 2 by default, 1 and 64)
  * the two info calls, on swept and on exact objects
  * six steps of PCG, PBiCGSTAB and PGMRES (restart 5: a restart and x through the fp64 combination, R = double on an fp32 object) against the
    model's IluPcg / IluBicgstab / IluGmres on the swept object; PCG to 1e-8 on the 24 x 24 Laplacian at s = 3: the model's step count, below plain
    CG's, and with max_iters far above it x and the result are those at the stop
  * the entry points that decline kind 2 decline it"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cvr_amd
import ilu_jacobi_model as JM
import ilu_model as IM
import krylov_model as KM
import pkrylov_gpu as G
import test_gpu_ilu0 as B
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

SWEEPS = [1, 2, 3, 4]


def _build(rp, ci, va, sweeps, lanes=None):
    """Precond.ilu0_jacobi, or Precond.ilu0 for sweeps None, with CVR_DEBUG=ilu_lanes=<lanes> in the environment while the object is built"""
    old = os.environ.get("CVR_DEBUG")
    try:
        if lanes is not None:
            os.environ["CVR_DEBUG"] = f"ilu_lanes={lanes}"
        else:
            os.environ.pop("CVR_DEBUG", None)
        return capi.Precond.ilu0(rp, ci, va) if sweeps is None else capi.Precond.ilu0_jacobi(rp, ci, va, sweeps)
    finally:
        if old is None:
            os.environ.pop("CVR_DEBUG", None)
        else:
            os.environ["CVR_DEBUG"] = old


def _case(name, prec):
    """(n, rp, ci, va, the model's factors, levels_lower, levels_upper)"""
    dtype = G.dtype_of(prec)
    if name.startswith("irr-"):
        c = IM.irregular_case(name, prec)
        return c[:5] + c[7:9]
    n, _, rp, ci, va = IM.wide_matrix(dtype) if name == "wide" else synth.laplacian_2d(int(name.partition("-")[2]), dtype)
    f, bad = IM.factor(rp, ci, va, dtype)
    assert bad is None
    return (n, rp, ci, va, f) + IM.levels(rp, ci)[2:]


def _same_bits(got, want, ctx):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (ctx, B._first_difference(got, want))


# ---- the apply ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name, lanes", [("laplacian-8", 2), ("irr-nonsym-2500", 2), ("irr-spd-700", 4), ("irr-dense-nonsym-320", 32), ("irr-dense-spd-320", 64), ("wide", 1)])
def test_apply_against_the_model(name, lanes, prec):
    dtype = G.dtype_of(prec)
    n, rp, ci, va, f, nlo, nup = _case(name, prec)
    nnz = int(rp[-1])
    assert IM.default_lanes(n, nnz) == lanes
    r = KM.inputs(n, dtype)[0]
    for s in SWEEPS:
        want = JM.IluJacobi(rp, ci, f, lanes, dtype, s).apply(r)
        assert np.isfinite(want).all() and want.any()
        P = _build(rp, ci, va, s)
        try:
            i = P.ilu0_jacobi_info()
            assert (i.n, i.nnz, i.sweeps, i.launches_per_apply, i.lanes_per_row, i.levels_lower, i.levels_upper, i.is_f32) == (n, nnz, s, 2 * s, lanes, nlo, nup, int(dtype == np.float32))
            assert not any(i.reserved)
            _same_bits(P.ilu0_export(), f, (name, prec, s, "factors"))
            for rshift, zshift in ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0)):          # (the last: once more on the aligned arrays, behind four applies)
                _same_bits(B._apply(P, r, dtype, rshift, zshift), want, (name, prec, "s", s, "shifts", rshift, zshift))
        finally:
            P.close()


@pytest.mark.parametrize("lanes", [1, 64])
def test_ilu_lanes_is_honoured(lanes):
    n, rp, ci, va, f, _, _ = _case("irr-spd-700", "fp64")
    r = KM.inputs(n, np.float64)[0]
    P = _build(rp, ci, va, 3, lanes)
    try:
        assert P.ilu0_jacobi_info().lanes_per_row == lanes == P.ilu0_info().lanes_per_row
        want = JM.IluJacobi(rp, ci, f, lanes, np.float64, 3).apply(r)
        assert want.tobytes() != JM.IluJacobi(rp, ci, f, 4, np.float64, 3).apply(r).tobytes()          # (the lane count shows in the bits)
        _same_bits(B._apply(P, r, np.float64), want, ("ilu_lanes", lanes))
    finally:
        P.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["laplacian-8", "irr-nonsym-2500", "wide"])
def test_exact_once_s_reaches_the_level_count_and_the_same_factors(name, prec):
    """device against device: s = max(levels_lower, levels_upper) gives the exact object's apply, and the swept object exports its factors"""
    dtype = G.dtype_of(prec)
    n, rp, ci, va, _, nlo, nup = _case(name, prec)
    r = KM.inputs(n, dtype)[0]
    E = _build(rp, ci, va, None)
    P = _build(rp, ci, va, max(nlo, nup))
    try:
        i = P.ilu0_jacobi_info()
        assert (i.levels_lower, i.levels_upper, i.sweeps) == (nlo, nup, max(nlo, nup)) and i.sweeps <= capi.ILU0_MAX_SWEEPS
        _same_bits(P.ilu0_export(), E.ilu0_export(), (name, prec, "factors"))
        want = B._apply(E, r, dtype)
        assert np.isfinite(want).all() and want.any()
        _same_bits(B._apply(P, r, dtype), want, (name, prec, "s", i.sweeps))
    finally:
        P.close()
        E.close()


@pytest.mark.parametrize("s", [2, 3])
def test_no_state_leaks_between_applies(s):
    n, rp, ci, va, f, _, _ = _case("irr-spd-700", "fp64")
    r1, r2 = KM.inputs(n, np.float64)[0], KM.inputs(n, np.float64, seed=5)[0]
    P = _build(rp, ci, va, s)
    try:
        z1, z2, z3 = B._apply(P, r1, np.float64), B._apply(P, r2, np.float64), B._apply(P, r1, np.float64)
        assert z1.tobytes() == z3.tobytes() and z1.tobytes() != z2.tobytes()
        _same_bits(z2, JM.IluJacobi(rp, ci, f, 4, np.float64, s).apply(r2), ("r2", s))
    finally:
        P.close()


# ---- edge cases ----
def _long_row(dtype, n=256, long_row=250, width=200):
    """a chain (row i reads row i - 1) with one row of `width` lower entries; strictly row dominant; the upper triangle mirrors the lower one"""
    rng = np.random.default_rng(20261021)
    lower = [[i - 1] if i else [] for i in range(n)]
    lower[long_row] = list(range(width - 1)) + [long_row - 1]
    upper = [[] for _ in range(n)]
    for i in range(n):
        for c in lower[i]:
            upper[c].append(i)
    rp, ci, va = [0], [], []
    for i in range(n):
        cols = lower[i] + [i] + upper[i]
        off = rng.uniform(-1.0, 1.0, size=len(cols))
        off[len(lower[i])] = 1.0 + np.abs(off).sum()
        ci += cols
        va += off.tolist()
        rp.append(len(ci))
    return n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_edge_cases(prec):
    dtype = G.dtype_of(prec)
    # n = 0: valid, an apply enqueues nothing
    E = capi.Precond.ilu0_jacobi(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype), 3)
    i = E.ilu0_jacobi_info()
    assert (i.n, i.nnz, i.sweeps, i.launches_per_apply, len(E.ilu0_export())) == (0, 0, 3, 0, 0) and E.ilu0_info().launches_lower == 0
    t = torch.full((2,), 7.0, dtype=G.tdt(dtype), device="cuda")
    E.apply(t[:1].data_ptr(), t[1:].data_ptr())
    torch.cuda.synchronize()
    assert t.cpu().tolist() == [7.0, 7.0]
    E.close()
    # n = 1
    for s in (1, 2):
        P = capi.Precond.ilu0_jacobi(np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.array([4.0], dtype=dtype), s)
        _same_bits(B._apply(P, np.array([3.0], dtype=dtype), dtype), np.array([0.75], dtype=dtype), ("n = 1", s))
        P.close()
    # a diagonal matrix: z = T(r / d)
    n = 1000
    rp, ci = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)
    d = (1.5 + np.random.default_rng(3).random(n)).astype(dtype)
    r = KM.inputs(n, dtype)[0]
    for s in (1, 2, 3):
        P = capi.Precond.ilu0_jacobi(rp, ci, d, s)
        _same_bits(B._apply(P, r, dtype), (r.astype(np.float64) / d.astype(np.float64)).astype(dtype), ("diagonal", s))
        P.close()
    # a row of 200 lower entries: two lanes by default, one lane that takes them all, 64 lanes in four rounds
    n, rp, ci, va = _long_row(dtype)
    f, bad = IM.factor(rp, ci, va, dtype)
    assert bad is None and IM.default_lanes(n, int(rp[-1])) == 2
    r = KM.inputs(n, dtype)[0]
    for s, lanes in ((2, None), (3, 1), (3, 64)):
        P = _build(rp, ci, va, s, lanes)
        assert P.ilu0_jacobi_info().lanes_per_row == (lanes or 2)
        _same_bits(B._apply(P, r, dtype), JM.IluJacobi(rp, ci, f, lanes or 2, dtype, s).apply(r), ("long row", s, lanes))
        P.close()


# ---- the info calls ----
def test_info_of_swept_and_exact_objects():
    L = capi.lib()
    n, _, rp, ci, va = synth.laplacian_2d(24)
    nnz = int(rp[-1])
    E = capi.Precond.ilu0(rp, ci, va)
    before = bytes(E.ilu0_info())
    try:
        for s in (1, 3, capi.ILU0_MAX_SWEEPS):
            P = capi.Precond.ilu0_jacobi(rp, ci, va, s)
            j, i, e = P.ilu0_jacobi_info(), P.ilu0_info(), E.ilu0_info()
            assert (j.sweeps, j.launches_per_apply) == (s, 2 * s) and (i.launches_lower, i.launches_upper) == (s, s)
            assert (j.n, j.nnz, j.lanes_per_row, j.levels_lower, j.levels_upper, j.is_f32) == (n, nnz, 2, 47, 47, 0)
            assert (i.n, i.nnz, i.levels_lower, i.levels_upper, i.max_level_width, i.lanes_per_row, i.wide_threshold, i.is_f32) == \
                   (e.n, e.nnz, e.levels_lower, e.levels_upper, e.max_level_width, e.lanes_per_row, e.wide_threshold, e.is_f32)
            pi = P.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks, pi.device) == (n, 0, 0, 0, 0, 0)
            assert L.cvr_precond_ilu0_jacobi_info(P._p, None) == capi.ERR_INVALID
            P.close()
        # an exact object is no swept one, and its own info is what it was
        assert L.cvr_precond_ilu0_jacobi_info(E._p, C.byref(capi.Ilu0JacobiInfo())) == capi.ERR_INVALID and "cvr_precond_ilu0_jacobi" in capi.last_error()
        e = E.ilu0_info()
        assert bytes(e) == before and (e.launches_lower, e.launches_upper) == (1, 1) and (e.levels_lower, e.levels_upper) == (47, 47)
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        assert L.cvr_precond_ilu0_jacobi_info(J._p, C.byref(capi.Ilu0JacobiInfo())) == capi.ERR_INVALID and "kind" in capi.last_error()
        J.close()
        for sweeps in (0, -1, capi.ILU0_MAX_SWEEPS + 1):
            with pytest.raises(capi.CvrError) as err:
                capi.Precond.ilu0_jacobi(rp, ci, va, sweeps)
            assert err.value.code == capi.ERR_INVALID and "sweeps" in str(err.value)
    finally:
        E.close()


def test_arrays_on_the_device():
    n, _, rp, ci, va = synth.laplacian_2d(24)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    P = capi.Precond.ilu0_jacobi_from_device(n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), 3)
    Q = capi.Precond.ilu0_jacobi(rp, ci, va, 3)
    try:
        f = IM.factor(rp, ci, va, np.float64)[0]
        assert P.ilu0_export().tobytes() == Q.ilu0_export().tobytes() == f.tobytes()
        r = KM.inputs(n, np.float64)[0]
        del rt, ct, vt          # the object keeps nothing of the caller's
        want = JM.IluJacobi(rp, ci, f, 2, np.float64, 3).apply(r)
        _same_bits(B._apply(P, r, np.float64), want, "device arrays")
        _same_bits(B._apply(Q, r, np.float64), want, "host arrays")
    finally:
        P.close()
        Q.close()


# ---- the solvers ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", ["pcg", "bicgstab", "gmres5"])
@pytest.mark.parametrize("name, s", [("laplacian-24", 3), ("irr", 2)])
def test_six_steps_against_the_model(name, s, which, prec):
    """irr: irr-spd-700 for PCG, irr-nonsym-700 (an unsymmetric pattern and factor) for the other two; gmres5 restarts after step 5 and forms x from
    the fp64 combination through the sweeps with R = double, on the fp32 object too"""
    dtype = G.dtype_of(prec)
    if name == "irr":
        name = "irr-spd-700" if which == "pcg" else "irr-nonsym-700"
    n, rp, ci, va, f, _, _ = _case(name, prec)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = _build(rp, ci, va, s)
    try:
        dev = G.Dev(A)
        kind = B._solver(which)
        lanes = P.ilu0_jacobi_info().lanes_per_row
        _same_bits(P.ilu0_export(), f, (name, prec, "factors"))
        model = JM.IluJacobi(rp, ci, f, lanes, dtype, s)
        b, x0, _ = KM.inputs(n, dtype)
        tr = B._model(which, dev.product, dtype, model).run(b, x0, rtol=0.0, max_iters=6)
        for k in range(7):
            if k >= len(tr.steps) and not tr.last.terminal:
                break
            for every, shift in ((1, 0), (0, 1)):
                got, res = kind.solve(A, P, b, x0, shift=shift, rtol=0.0, max_iters=k, check_every=every)
                G.same(got, tr.at(k), (name, which, prec, "s", s, "max_iters", k, "check_every", every, "shift", shift))
                if got.status == capi.CG_MAX_ITERS:          # k steps enqueued, none behind a stop: kind 2's spmv_count
                    assert res.spmv_count == kind.spmvs(k), (which, k, every, res.spmv_count)
        got, _ = kind.solve_host(A, P, b, x0=x0, rtol=0.0, max_iters=6)          # the host twin
        G.same(got, tr.at(6), (name, which, prec, "host"))
    finally:
        P.close()
        A.close()


def test_pcg_to_1e_8_on_the_24_by_24_laplacian():
    """the model's step count, below plain CG's; with max_iters far above it the steps enqueued behind the stop change nothing: every sweep launch
    returns at its top under the gate, so x and the result are those at the stop, whatever check_every is"""
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0_jacobi(rp, ci, va, 3)
    try:
        kind = B._solver("pcg")
        model = JM.IluJacobi(rp, ci, P.ilu0_export(), 2, np.float64, 3)
        b = KM.inputs(n, np.float64)[0]
        last = B._model("pcg", G.Dev(A).product, np.float64, model).run(b, None, rtol=1e-8, max_iters=400).last
        assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < 60, last
        plain, pres = kind.solve(A, None, b, rtol=1e-8, max_iters=400)
        assert pres.status == capi.CG_CONVERGED
        for every, enqueued in ((1, last.iterations), (3, -(-last.iterations // 3) * 3), (0, -(-last.iterations // 8) * 8), (400, 400)):
            got, res = kind.solve(A, P, b, rtol=1e-8, max_iters=400, check_every=every)
            G.same(got, last, ("pcg", "check_every", every))
            assert res.spmv_count == kind.spmvs(enqueued), (every, res.spmv_count, enqueued)
        print(f"laplacian_2d(24): swept ILU(0)-PCG at s = 3 {last.iterations} steps, cvr_cg {pres.iterations}")
        assert got.iterations < pres.iterations
    finally:
        P.close()
        A.close()


@pytest.mark.parametrize("which", ["bicgstab", "gmres5"])
def test_the_gate_holds_behind_a_stop(which):
    """BiCGSTAB's two stop words and GMRES's stop and owed-x guard: a solve to 1e-8 with every step of one batch enqueued ends in the model's state"""
    n, rp, ci, va, f, _, _ = _case("irr-nonsym-700", "fp64")
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0_jacobi(rp, ci, va, 2)
    try:
        kind = B._solver(which)
        b = KM.inputs(n, np.float64)[0]
        last = B._model(which, G.Dev(A).product, np.float64, JM.IluJacobi(rp, ci, f, 4, np.float64, 2)).run(b, None, rtol=1e-8, max_iters=100).last
        assert last.terminal and last.status == KM.CONVERGED and 0 < last.iterations < 50, last
        for every in (1, 100):
            got, _ = kind.solve(A, P, b, rtol=1e-8, max_iters=100, check_every=every)
            G.same(got, last, (which, "check_every", every))
    finally:
        P.close()
        A.close()


def test_entry_points_that_decline_kind_2():
    L = capi.lib()
    n = 250
    _, _, rp, ci, va = KM.banded("spd", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.ilu0_jacobi(rp, ci, va, 3)
    try:
        b = synth.x_rand(n)
        bt, xt = G.put(b, np.float64), G.put(np.zeros(n), np.float64)
        out = np.zeros(len(va))

        def declined(rc, name):
            assert rc == capi.ERR_STATE, (name, rc, capi.last_error())
            assert "kind 2" in capi.last_error() and "ILU(0)" in capi.last_error(), (name, capi.last_error())

        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_precond_apply_multi_device(P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None), "apply_multi")
        opt, res = capi.CgOptions(), capi.CgResult()
        L.cvr_cg_default_options(C.byref(opt))
        hb, hx = b.copy(), np.zeros(n)
        declined(L.cvr_pcg_multi_device(A._h, P._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None), "pcg_multi_device")
        declined(L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)), "pcg_multi")
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran
        assert L.cvr_precond_apply_device(P._p, bt.data_ptr(), bt.data_ptr(), None) == capi.ERR_INVALID          # r == z, as for every kind
    finally:
        P.close()
        A.close()
