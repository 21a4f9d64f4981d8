"""BiCGSTAB on the device (cvr_bicgstab_device, cvr_bicgstab) -- what can be checked without a GPU: the ABI (exports, the argument checks that
come before any device work and before the handle is looked at), the code of the solver's vector kernels for gfx950 (every fp32 / fp64
instantiation is there and runs without scratch or spills) and the generator of its test matrices."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_bicgstab_device", "cvr_bicgstab")


def test_library_exports_the_solver_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


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
    for call in (lambda h, b, x, o, r: L.cvr_bicgstab_device(h, b, x, o, r, None), L.cvr_bicgstab):
        assert call(None, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, None, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, None, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, p, p, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, p, p, C.byref(o), C.byref(res)) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()


def test_python_wrappers_exist():
    for name in ("bicgstab", "bicgstab_host"):
        assert callable(getattr(capi.CvrMatrix, name))


def test_nonsym_from_pattern():
    """A = I - W: unit diagonal, every row's off-diagonal absolute sum c (at most c, to the rounding of a row of k entries: c (1 + (k + 4) eps) of
    the type), sorted columns without duplicates, not symmetric; rscale scales rows"""
    n, _, rp, ci, _ = synth.rmat(9, dedupe=True)
    c = 0.5
    for dtype in (np.float64, np.float32):
        n2, nc, rp2, ci2, va = synth.nonsym_from_pattern(n, rp, ci, c=c, dtype=dtype)
        assert (n2, nc) == (n, n) and va.dtype == dtype and rp2[-1] == len(ci2) == len(va)
        rows = np.repeat(np.arange(n), np.diff(rp2))
        assert len(set(zip(rows.tolist(), ci2.tolist()))) == len(ci2), "duplicates"
        for r in range(n):
            assert np.all(np.diff(ci2[rp2[r]:rp2[r + 1]]) > 0), "columns of a row sorted"
        A = np.zeros((n, n))
        A[rows, ci2] = va
        assert not np.array_equal(A, A.T)
        assert not np.array_equal(A != 0, (A != 0).T), "the pattern is not symmetrised"
        assert np.array_equal(np.diag(A), np.ones(n))
        offsum = np.abs(A - np.eye(n)).sum(axis=1)
        tol = c * (np.diff(rp2) + 4) * np.finfo(dtype).eps          # the row's sum in the generator, the entries' rounding, the sum here
        assert np.all(offsum <= c + tol), (offsum - c).max()
        has_off = np.diff(rp2) > 1
        assert has_off.any() and np.all(offsum[has_off] >= c - tol[has_off])
        assert np.all(A[~np.eye(n, dtype=bool)] <= 0)
        ev = np.linalg.eigvals(A)
        assert np.abs(ev - 1).max() <= c + 1e-6          # Gershgorin
    # the weights are seeded: the same call gives the same values, another seed other ones
    assert np.array_equal(synth.nonsym_from_pattern(n, rp, ci)[4], synth.nonsym_from_pattern(n, rp, ci)[4])
    assert not np.array_equal(synth.nonsym_from_pattern(n, rp, ci, seed=4)[4], synth.nonsym_from_pattern(n, rp, ci)[4])
    s = 10.0 ** (2 * np.random.default_rng(1).random(n))
    _, _, rp2, ci2, va = synth.nonsym_from_pattern(n, rp, ci)
    _, _, rp3, ci3, vs = synth.nonsym_from_pattern(n, rp, ci, rscale=s)
    assert np.array_equal(rp3, rp2) and np.array_equal(ci3, ci2)
    rows = np.repeat(np.arange(n), np.diff(rp2))
    assert np.array_equal(vs, s[rows] * va)
    B = np.zeros((n, n))
    B[rows, ci3] = vs
    assert np.array_equal(np.diag(B), s)


@pytest.fixture(scope="module")
def bicg_md():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_bicgstab.hip"))
    try:
        yield isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def _demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def test_solver_kernels_without_scratch_or_spills(bicg_md):
    dem = _demangled(list(bicg_md))
    seen = {}
    for name, item in bicg_md.items():
        d = dem[name]
        m = re.search(r"(?<!\w)(p?bicg_\w+_kernel)(?:<(float|double)[^>]*>)?", d)          # (anchored: pbicg_apply_kernel is no bicg_* kernel)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x preconditioner x alignment of the caller's arrays where a pass touches them: b, x and minv at the start, x (and s^ apart from s) in the
    # update, x alone in the half step; minv alone in the s and direction passes (no alignment variant without a preconditioner); T for r^ . v
    # The block-Jacobi object's apply, which lives in this file too (test_pkrylov_host.py), by T.
    assert {k: len(v) for k, v in seen.items()} == dict(bicg_init_kernel=8, bicg_check_kernel=1, bicg_rv_kernel=2, bicg_s_kernel=6, bicg_half_kernel=4,
                                                        bicg_update_kernel=8, bicg_direction_kernel=6, pbicg_apply_kernel=2), seen
    for k, v in seen.items():
        if k != "bicg_check_kernel":
            assert any("<float" in d for d in v) and any("<double" in d for d in v), k
    # at most five vector launches per step without a preconditioner and with the diagonal: the bicg_* kernels
    assert len({k for k in seen if k.startswith("bicg_")} - {"bicg_init_kernel", "bicg_check_kernel"}) <= 5
