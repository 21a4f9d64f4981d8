"""Restarted GMRES on the device (cvr_gmres_device, cvr_gmres) -- what can be checked without a GPU: the ABI (exports, the argument checks that come
before any device work and before the handle is looked at, `restart` among them), the code of the solver's kernels for gfx950 (no scratch, no spills),
and the numpy model of the header's text (tests/gmres_model.py) on cases worked by hand, against numpy.linalg.solve, against the true residual, and
against its own mutants.  The model's product here is the oracle's CSR loop rounded to T."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gmres_model as GM
import krylov_model as KM
import oraclelib as O
from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_gmres_device", "cvr_gmres")


def test_library_exports_the_solver_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    assert re.search(r"#define\s+CVR_GMRES_MAX_RESTART\s+64\b", hdr)


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    ok, res = _options(), capi.CgResult()
    for call in (lambda h, b, x, m, o, r: L.cvr_gmres_device(h, b, x, m, o, r, None), L.cvr_gmres):
        assert call(None, p, p, 30, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, None, p, 30, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, None, 30, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, 30, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, 30, C.byref(ok), None) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, p, p, 30, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, p, p, 30, C.byref(o), C.byref(res)) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()
        for restart in (0, -1, 65):
            assert call(fake, p, p, restart, C.byref(ok), C.byref(res)) == capi.ERR_INVALID, restart
            assert "restart" in capi.last_error()
        # the other checks come first: a null b with a bad restart is the null
        assert call(fake, None, p, 0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()


def test_python_wrappers_exist():
    for name in ("gmres", "gmres_host"):
        assert callable(getattr(capi.CvrMatrix, name))


@pytest.fixture(scope="module")
def gmres_md():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_gmres.hip"))
    try:
        yield isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def test_solver_kernels_without_scratch_or_spills(gmres_md):
    names = list(gmres_md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in gmres_md.items():
        d = dem[name]
        m = re.search(r"(?<!\w)(p?gmres_\w+_kernel)<(float|double)", d)          # (anchored: the pgmres_* kernels are no gmres_* kernels)
        assert m, d
        seen.setdefault(m.group(1), set()).add(m.group(2))
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    assert {k for k in seen if k.startswith("gmres_")} == {"gmres_dots_kernel", "gmres_update_kernel", "gmres_finish_kernel", "gmres_rr_kernel",
                                                        "gmres_begin_kernel", "gmres_x_kernel"}, seen
    # ... and the block-Jacobi object's kernels, which live in this file too (test_pkrylov_host.py)
    assert {k for k in seen if not k.startswith("gmres_")} == {"pgmres_apply_kernel", "pgmres_u_kernel", "pgmres_x_kernel"}, seen
    assert all(v == {"float", "double"} for v in seen.values()), seen


# ---- the model ----
def _csr(A, dtype):
    A = np.asarray(A, dtype=np.float64)
    n = len(A)
    rp = np.zeros(n + 1, dtype=np.int64)
    ci, va = [], []
    for i in range(n):
        for j in range(n):
            if A[i, j] != 0:
                ci.append(j)
                va.append(A[i, j])
        rp[i + 1] = len(ci)
    return rp, np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def _product(rp, ci, va):
    return lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)


def _shift(n, dtype):
    """the cyclic shift of tests/test_gpu_bicgstab.py: row i holds a one in column i + 1 mod n"""
    return np.arange(n + 1, dtype=np.int64), ((np.arange(n) + 1) % n).astype(np.int32), np.ones(n, dtype=dtype)


def _true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, x)
    return float(np.linalg.norm(np.asarray(b, dtype=np.float64) - y))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_lucky_breakdown_worked_by_hand(dtype):
    """A = [[0, 1], [-1, 0]], b = (1, 0), m = 2.  v_0 = (1, 0), w = A v_0 = (0, -1): h_0 = 0, H_1 = 1, so cs_0 = 0, sn_0 = 1, g = (0, -1), e = 1.
    v_1 = (0, -1), w = A v_1 = (-1, 0): h_0 = -1, h_1 = 0, w becomes 0, H_2 = 0; rotation 0 turns (H_0, H_1) = (-1, 0) into (0, 1); rho = 1, cs_1 = 1,
    sn_1 = 0, e = 0.  R = I, y = (0, -1), x = -v_1 = (0, 1)."""
    rp, ci, va = _csr([[0, 1], [-1, 0]], dtype)
    tr = GM.GmresModel(_product(rp, ci, va), dtype, restart=2).run(np.array([1, 0], dtype=dtype), rtol=1e-8, max_iters=10)
    assert len(tr.steps) == 3 and tr.last.terminal
    s1, s2 = tr.steps[1], tr.steps[2]
    assert (s1.scalars["cs"], s1.scalars["sn"]) == (0.0, 1.0) and s1.residual_norm == 1.0 and (s1.status, s1.iterations) == (KM.MAX_ITERS, 1)
    assert (s2.status, s2.iterations, s2.residual_norm) == (KM.CONVERGED, 2, 0.0)
    assert s2.x.dtype == dtype and s2.x.tolist() == [0.0, 1.0]
    assert tr.at(7) is s2


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_cyclic_shift(dtype):
    """b = e_0: the Krylov vectors are e_0, e_7, e_6, ... -- orthogonal to b until the eighth, so the estimate stays ||b|| through step 7 and m = 8
    converges at step 8, while m = 4 restarts from the same residual for ever"""
    n = 8
    rp, ci, va = _shift(n, dtype)
    b = np.zeros(n, dtype=dtype)
    b[0] = 1
    tr = GM.GmresModel(_product(rp, ci, va), dtype, restart=8).run(b, rtol=1e-8, max_iters=20)
    assert len(tr.steps) == 9 and tr.last.terminal
    for k in range(8):
        assert (tr.steps[k].status, tr.steps[k].iterations, tr.steps[k].residual_norm) == (KM.MAX_ITERS, k, 1.0), k
    assert (tr.last.status, tr.last.iterations, tr.last.residual_norm) == (KM.CONVERGED, 8, 0.0)
    assert _true_residual(rp, ci, va, tr.last.x, b) == 0.0
    tr = GM.GmresModel(_product(rp, ci, va), dtype, restart=4).run(b, rtol=1e-8, max_iters=12)
    assert len(tr.steps) == 13 and not tr.last.terminal
    for k in range(13):
        s = tr.steps[k]
        assert (s.status, s.iterations, s.residual_norm, s.b_norm) == (KM.MAX_ITERS, k, 1.0, 1.0), k
        assert not s.x.any()


def test_breakdown_on_a_zero_matrix():
    """no entry at all: w = 0, every h is 0 and rho = 0 at j = 0 -- found before the step is counted, x untouched"""
    n = 5
    rp, ci, va = np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)
    b, x0, _ = KM.inputs(n, np.float64)
    tr = GM.GmresModel(_product(rp, ci, va), np.float64, restart=3).run(b, x0, rtol=1e-8, max_iters=10)
    assert len(tr.steps) == 2 and tr.last.terminal
    assert (tr.last.status, tr.last.iterations) == (KM.BREAKDOWN, 0)
    assert tr.last.x.tobytes() == x0.tobytes()
    assert tr.last.residual_norm == tr.steps[0].residual_norm == np.sqrt(KM.tree_sum(b.astype(np.float64) ** 2, 2))


def test_stop_states_of_the_start():
    n = 40
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    prod = _product(rp, ci, va)
    b, x0, _ = KM.inputs(n, np.float64)
    tr = GM.GmresModel(prod, np.float64, restart=3).run(np.zeros(n), x0, rtol=1e-8)
    assert len(tr.steps) == 1 and (tr.last.status, tr.last.iterations, tr.last.residual_norm, tr.last.b_norm) == (KM.CONVERGED, 0, 0.0, 0.0) and not tr.last.x.any()
    for bad in (np.nan, np.inf):
        bn = b.copy()
        bn[n // 2] = bad
        tr = GM.GmresModel(prod, np.float64, restart=3).run(bn, x0, rtol=1e-8)
        assert len(tr.steps) == 1 and (tr.last.status, tr.last.iterations) == (KM.BREAKDOWN, 0) and tr.last.x.tobytes() == x0.tobytes()
    xs = np.linalg.solve(_dense(n, rp, ci, va), b)
    tr = GM.GmresModel(prod, np.float64, restart=3).run(b, xs, rtol=1e-8)
    assert len(tr.steps) == 1 and (tr.last.status, tr.last.iterations) == (KM.CONVERGED, 0) and tr.last.x.tobytes() == xs.tobytes()
    tr = GM.GmresModel(prod, np.float64, restart=3).run(b, x0, rtol=0.0, max_iters=0)
    assert len(tr.steps) == 1 and not tr.last.terminal and tr.last.x.tobytes() == x0.tobytes()


def _dense(n, rp, ci, va):
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    return A


def test_full_gmres_solves_a_small_system():
    """m = n = 12 in fp64: the Krylov space is everything after at most 12 steps"""
    n = 12
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    b, _, _ = KM.inputs(n, np.float64)
    tr = GM.GmresModel(_product(rp, ci, va), np.float64, restart=n).run(b, rtol=1e-14, max_iters=n)
    ref = np.linalg.solve(_dense(n, rp, ci, va), b)
    err = np.linalg.norm(tr.last.x - ref) / np.linalg.norm(ref)
    print(f"{tr.last.iterations} steps, status {tr.last.status}, |x - solve| / |solve| = {err:.3g}")
    assert tr.last.iterations <= n
    assert err <= 1e-12


@pytest.mark.parametrize("pre", [False, True])
def test_the_estimate_is_the_true_residual(pre):
    """banded("nonsym", 300), m = 5, fp64: at every entry the estimate e = |g_(j+1)| agrees with ||b - A x|| of that entry's x to 1e-10 relative.  The two
    differ by the rounding of the basis and of x, O(eps * steps * ||b||) absolute (the twice-applied Gram-Schmidt keeps the basis orthogonal to eps), so
    the relative bound holds while e >= 1e-4 ||b||: the run stops at rtol = 1e-4, which lies behind a restart (the spectrum lies in |z - 1| <= 0.5)."""
    n, m = 300, 5
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    b, x0, minv = KM.inputs(n, np.float64)
    tr = GM.GmresModel(_product(rp, ci, va), np.float64, restart=m).run(b, x0, minv if pre else None, rtol=1e-4, max_iters=60)
    assert tr.last.terminal and tr.last.status == KM.CONVERGED and tr.last.iterations > m, tr.last          # (behind a restart)
    worst = 0.0
    for k, s in enumerate(tr.steps):
        true = _true_residual(rp, ci, va, s.x, b)
        worst = max(worst, abs(s.residual_norm - true) / true)
        assert abs(s.residual_norm - true) <= 1e-10 * true, (k, s.residual_norm, true)
    print(f"{tr.last.iterations} steps, worst |e - true| / true = {worst:.3g}")
    # and the estimate never grows within the run
    norms = [s.residual_norm for s in tr.steps]
    assert all(a >= c * (1 - 1e-10) for a, c in zip(norms, norms[1:]))


# ---- the mutants: each is the model with one method replaced; its trajectory must differ from the model's on the stated case ----
def _descending_rows(self, R, g, q):
    y = np.zeros(q)
    for i in range(q - 1, -1, -1):
        t = g[i]
        for l in range(q - 1, i, -1):
            t = t - R[i, l] * y[l]
        y[i] = t / R[i, i]
    return y


def _descending_u(self, y, V):
    u = np.zeros(len(V[0]))
    for yi, v in zip(y[::-1], V[::-1]):
        u = u + yi * KM._f64(v)
    return u


# name -> (the defect, restart, max_iters, why it shows there)
MUTANTS = {
    "one pass instead of two": (dict(passes=lambda self: 1), 4, 9, "w and H keep the first pass's rounding: v_1 differs in its last bits from step 1 on"),
    "H_i = h_i only": (dict(combine=lambda self, h, d: h), 4, 9, "the second pass's d_i, a few eps of h_i, is missing from R"),
    "rotation sign": (dict(rotate=lambda self, cs, sn, a, b: (cs * a - sn * b, cs * b + sn * a)), 4, 9, "step 2 is the first with an earlier rotation"),
    "back substitution order": (dict(back_substitute=_descending_rows), 8, 9, "from three columns on a row has two terms to subtract in either order"),
    "u accumulated descending": (dict(combination=_descending_u), 8, 9, "from three columns on the order of the additions shows"),
    "v_(j+1) divided by the rotated value": (dict(divisor=lambda self, hn, rho: rho), 4, 9, "v_1 has another length from step 1 on: step 2 differs"),
    "restart on the estimate": (dict(cycle_norm=lambda self, rr, est: np.sqrt(rr) if est is None else est), 4, 9,
                                "the first restart, in front of step 5: g_0 and v_0 differ in their last bits"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_compare_rejects_the_mutant(name):
    methods, m, steps, why = MUTANTS[name]
    n, dtype = 300, np.float64
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    prod = _product(rp, ci, va)
    b, x0, minv = KM.inputs(n, dtype)
    good = GM.GmresModel(prod, dtype, restart=m).run(b, x0, minv, rtol=0.0, max_iters=steps)
    bad = type("Mutant", (GM.GmresModel,), methods)(prod, dtype, restart=m).run(b, x0, minv, rtol=0.0, max_iters=steps)
    assert len(good.steps) == steps + 1
    found = [(k, msg) for k in range(len(good.steps)) for msg in [KM.compare(bad.at(k) if bad.last.terminal else bad.steps[min(k, len(bad.steps) - 1)], good.steps[k])] if msg]
    assert found, f"{name}: not rejected within {steps} steps"
    k, msg = found[0]
    print(f"mutant '{name}' rejected at step {k} ({why}): {msg}")
    again = GM.GmresModel(prod, dtype, restart=m).run(b, x0, minv, rtol=0.0, max_iters=steps)
    assert all(KM.compare(again.at(k), good.at(k)) == "" for k in range(len(good.steps)))
