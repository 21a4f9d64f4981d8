"""The thick-restart Golub-Kahan-Lanczos solver (cvr_svds_device, cvr_svds, cvr_svd_host) -- what can be checked without a GPU: the ABI (exports,
struct sizes and field order, the defaults, the Python methods), the argument checks that come before any device work and before a handle is looked
at, in their order, the code of the solver's kernels for gfx950, and cvr_svd_host against numpy.linalg.svd (LAPACK).

cvr_svd_host: random p x q matrices with p <= q at sizes 1 .. 65, bidiagonal-plus-spike matrices of the restart's shape (square, and the p x (p + 1)
shape of a closed left half), repeated and zero singular values, a graded matrix, one of rank 1 with equal rows and a zero one; ldb, lduq and ldvp
beyond the matrix.  Four figures per matrix, each relative to sigma_max: max |s - s_ref|, ||B - Q diag(s) P^T||_F, ||Q^T Q - I||_F and
||P^T P - I||_F (the last two absolute: the factors have unit columns).  The bound is measured, not guessed: the largest figure over exactly these
matrices (fixed seeds, x86-64) is 1.47e-14 = 66 * 2^-52, the reconstruction of the 64 x 65 graded matrix; the orthogonality of Q reaches 1.46e-14
(65 x 65 repeated: Q is the product of every rotation of every sweep), the largest value error is 1.72e-15 (64 x 65 bidiagonal) and the largest
figure for P 5.17e-15 (65 x 65 equal rows).  The test allows MULTIPLE = 8 times the measured maximum, 8 * MEASURED = 1.18e-13, for all four."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_svds_device", "cvr_svds", "cvr_svd_host")
MEASURED, MULTIPLE = 1.47e-14, 8          # the module docstring: the largest figure observed, and what the test allows of it


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert hasattr(L, "cvr_svd_default_options") and "cvr_svd_default_options" in capi.SYMBOLS and re.search(r"\bvoid cvr_svd_default_options\(", hdr)
    assert re.search(r"}\s*cvr_svd_options;\s*/\* 40 bytes \*/", hdr) and re.search(r"}\s*cvr_svd_result;\s*/\* 32 bytes \*/", hdr)
    assert C.sizeof(capi.SvdOptions) == 40 and [f[0] for f in capi.SvdOptions._fields_] == ["nev", "ncv", "max_restarts", "reserved0", "tol", "reserved"]
    assert [getattr(capi.SvdOptions, f).offset for f in ("nev", "ncv", "max_restarts", "reserved0", "tol", "reserved")] == [0, 4, 8, 12, 16, 24]
    assert C.sizeof(capi.SvdResult) == 32 and [f[0] for f in capi.SvdResult._fields_] == ["nconv", "status", "restarts", "spmv_count", "seconds", "max_estimate"]
    assert [getattr(capi.SvdResult, f).offset for f in ("nconv", "status", "restarts", "spmv_count", "seconds", "max_estimate")] == [0, 4, 8, 12, 16, 24]
    assert re.search(r"#define CVR_SVD_MAX_NCV\s+64\b", hdr) and capi.SVD_MAX_NCV == 64
    # one set of status codes: the eigensolver's
    assert not re.search(r"#define CVR_SVD_(CONVERGED|MAX_RESTARTS|BREAKDOWN|INVARIANT)", hdr)
    section = hdr[hdr.index("thick-restart Golub-Kahan-Lanczos"):hdr.index("int cvr_svd_host(")]
    for word in ("HIP graph", "harmonic-Ritz", "shift-and-invert", "more\n * than one GPU", "block variant", "implicit A^T", "CVR_EIG_INVARIANT", "spmv_count"):
        assert word in section, word


def test_default_options():
    o = capi.SvdOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    capi.lib().cvr_svd_default_options(C.byref(o))
    assert (o.nev, o.ncv, o.max_restarts, o.reserved0, o.tol, list(o.reserved)) == (1, 0, 100, 0, 1e-8, [0, 0, 0, 0])
    capi.lib().cvr_svd_default_options(None)          # a null pointer is ignored


def test_python_methods_exist():
    for name in ("svds", "svds_host"):
        assert callable(getattr(capi.CvrMatrix, name))
    s, Q, P = capi.svd_host(np.array([[3.0, 0.0, 0.0], [0.0, 0.0, -4.0]]))
    assert s.tolist() == [4.0, 3.0] and Q.tolist() == [[0.0, 1.0], [1.0, 0.0]] and P.tolist() == [[0.0, 1.0], [0.0, 0.0], [-1.0, 0.0]]
    assert capi.svd_host(np.array([[-5.0]]), vectors=False).tolist() == [5.0]
    with pytest.raises(capi.CvrError):
        capi.svd_host(np.zeros((3, 2)))          # p > q


def _options(**kw):
    o = capi.SvdOptions()
    capi.lib().cvr_svd_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_svds_device", lambda a, at, v, s, U, ldu, V, ldv, o, r: L.cvr_svds_device(a, at, v, s, U, ldu, V, ldv, o, r, None)),
            ("cvr_svds", lambda a, at, v, s, U, ldu, V, ldv, o, r: L.cvr_svds(a, at, v, s, U, ldu, V, ldv, o, r)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at a handle)
    ok, res = _options(), capi.SvdResult()
    for name, call in _calls():
        def bad(what, *a):
            assert call(*a) == capi.ERR_INVALID, (name, what)
            assert what in capi.last_error(), (name, what, capi.last_error())
        bad("null a", None, fake, p, p, p, 64, p, 64, C.byref(ok), C.byref(res))
        bad("null handle of the transpose", fake, None, p, p, p, 64, p, 64, C.byref(ok), C.byref(res))
        bad("null v0", fake, fake, None, p, p, 64, p, 64, C.byref(ok), C.byref(res))
        bad("null svals", fake, fake, p, None, p, 64, p, 64, C.byref(ok), C.byref(res))
        bad("null opt", fake, fake, p, p, p, 64, p, 64, None, C.byref(res))
        bad("null res", fake, fake, p, p, p, 64, p, 64, C.byref(ok), None)
        for nev in (0, -3):
            bad("nev", fake, fake, p, p, p, 64, p, 64, C.byref(_options(nev=nev)), C.byref(res))
        for nev, ncv in ((1, 1), (1, 2), (3, 4), (1, 65), (1, -1), (63, 64)):
            bad("ncv", fake, fake, p, p, p, 64, p, 64, C.byref(_options(nev=nev, ncv=ncv)), C.byref(res))
        bad("max_restarts", fake, fake, p, p, p, 64, p, 64, C.byref(_options(max_restarts=-1)), C.byref(res))
        bad("reserved0", fake, fake, p, p, p, 64, p, 64, C.byref(_options(reserved0=1)), C.byref(res))
        for tol in (-1.0, float("nan"), float("inf")):
            bad("tol", fake, fake, p, p, p, 64, p, 64, C.byref(_options(tol=tol)), C.byref(res))
        o = _options()
        o.reserved[2] = 1
        bad("reserved[2]", fake, fake, p, p, p, 64, p, 64, C.byref(o), C.byref(res))
        for ld in (0, -5):
            bad("ldu", fake, fake, p, p, p, ld, p, 64, C.byref(ok), C.byref(res))
            bad("ldv", fake, fake, p, p, p, 64, p, ld, C.byref(ok), C.byref(res))
            bad("ldv", fake, fake, p, p, None, ld, p, ld, C.byref(ok), C.byref(res))          # a null block's leading dimension is not looked at
        # the order: every check fails at once -> the first one named; then one by one
        o = _options(nev=0, ncv=1, max_restarts=-1, reserved0=9, tol=-1.0)
        o.reserved[0] = 1
        bad("null handle of the transpose", fake, None, None, None, p, 0, p, 0, C.byref(o), None)
        bad("null v0", fake, fake, None, None, p, 0, p, 0, C.byref(o), None)
        bad("null svals", fake, fake, p, None, p, 0, p, 0, C.byref(o), None)
        bad("null res", fake, fake, p, p, p, 0, p, 0, C.byref(o), None)
        bad("nev", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.nev = 1
        bad("ncv", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.ncv = 0
        bad("max_restarts", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.max_restarts = 0
        bad("reserved0", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.reserved0 = 0
        bad("tol", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.tol = 0.0
        bad("reserved[0]", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        o.reserved[0] = 0
        bad("ldu", fake, fake, p, p, p, 0, p, 0, C.byref(o), C.byref(res))
        bad("ldv", fake, fake, p, p, p, 1, p, 0, C.byref(o), C.byref(res))


def test_svd_host_argument_checks():
    L = capi.lib()
    b, s, uq, vp = np.eye(3, 4, order="F"), np.zeros(3), np.zeros((3, 3), order="F"), np.zeros((4, 3), order="F")
    ptr = lambda a: a.ctypes.data          # noqa: E731
    assert L.cvr_svd_host(3, 4, ptr(b), 3, ptr(s), ptr(uq), 3, ptr(vp), 4) == 0 and s.tolist() == [1.0, 1.0, 1.0]
    big = np.zeros((66, 67), order="F")
    for p, q, bp, ldb, sp, lduq, ldvp in ((0, 4, ptr(b), 3, ptr(s), 3, 4), (4, 3, ptr(b), 4, ptr(s), 4, 4), (66, 66, ptr(big), 66, ptr(big), 66, 66),
                                          (3, 66, ptr(big), 3, ptr(s), 3, 66), (3, 4, None, 3, ptr(s), 3, 4), (3, 4, ptr(b), 3, None, 3, 4),
                                          (3, 4, ptr(b), 2, ptr(s), 3, 4), (3, 4, ptr(b), 3, ptr(s), 2, 4), (3, 4, ptr(b), 3, ptr(s), 3, 3)):
        assert L.cvr_svd_host(p, q, bp, ldb, sp, ptr(uq), lduq, ptr(vp), ldvp) == capi.ERR_INVALID, (p, q, ldb, lduq, ldvp)
    assert L.cvr_svd_host(3, 4, ptr(b), 3, ptr(s), None, 0, None, 0) == 0          # values only: the leading dimensions are not looked at
    for v in (np.nan, np.inf, -np.inf):
        b[2, 3] = v
        assert L.cvr_svd_host(3, 4, ptr(b), 3, ptr(s), ptr(uq), 3, ptr(vp), 4) == capi.ERR_INVALID and "finite" in capi.last_error()


# ---- cvr_svd_host against LAPACK
def _with_values(p, q, sv, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    P, _ = np.linalg.qr(rng.standard_normal((q, p)))
    return (Q * sv) @ P.T


def _restart_shape(p, q, k, rng):
    """diag(sigma) of k entries with the spike in column k, upper bidiagonal beyond: the solver's projected matrix (q = p, or p + 1: a closed left half)"""
    B = np.zeros((p, q))
    B[np.arange(p), np.arange(p)] = np.abs(rng.standard_normal(p)) + 0.1
    B[:k, :k] = np.diag(np.sort(np.abs(rng.standard_normal(k)) + 1.0)[::-1])
    if k < q:
        B[:k, k] = 1e-3 * rng.standard_normal(k)
    for j in range(k, p):
        if j + 1 < q:
            B[j, j + 1] = abs(rng.standard_normal())
    return B


def _matrices(p, q):
    rng = np.random.default_rng(20261021 + 100 * p + q)
    yield "random", rng.standard_normal((p, q))
    yield "restart", _restart_shape(p, q, p // 3, rng)
    yield "bidiagonal", _restart_shape(p, q, 0, rng)
    yield "repeated", _with_values(p, q, np.repeat(np.arange(-(-p // 5), 0, -1.0), 5)[:p], rng)
    yield "zeros", _with_values(p, q, np.where(np.arange(p) < (p + 1) // 2, np.arange(p, 0, -1.0), 0.0), rng)
    yield "graded", _with_values(p, q, 10.0 ** -np.arange(p, dtype=np.float64).clip(max=30), rng) * 1e40
    yield "equal rows", np.outer(np.where(np.arange(p) % 3 == 0, 1.0, 0.0), np.arange(q) % 5 + 1.0)          # rank 1: rotations leave rows of rounding noise
    yield "zero matrix", np.zeros((p, q))


SHAPES = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 65), (7, 8), (20, 20), (20, 21), (33, 40), (63, 64), (64, 64), (64, 65), (65, 65)]


@pytest.mark.parametrize("p,q", SHAPES, ids=[f"{p}x{q}" for p, q in SHAPES])
def test_svd_host_against_lapack(p, q):
    """the four figures of the module docstring, each at most MULTIPLE * MEASURED; order, sign rule, the same bytes on two calls, values only"""
    L = capi.lib()
    worst = np.zeros(4)
    for name, B in _matrices(p, q):
        s_ref = np.linalg.svd(B, compute_uv=False)
        top = s_ref[0] if s_ref[0] > 0 else 1.0
        for pad in (0, 3):
            ldb, lduq, ldvp = p + pad, p + 2 * pad, q + pad
            b = np.full((q, ldb), 1e300)          # b[j, i] in C order is element (i, j) at i + j * ldb; garbage beyond p
            b[:, :p] = B.T
            s, uq, vp = np.zeros(p), np.full((p, lduq), 7.0), np.full((p, ldvp), 7.0)
            assert L.cvr_svd_host(p, q, b.ctypes.data, ldb, s.ctypes.data, uq.ctypes.data, lduq, vp.ctypes.data, ldvp) == 0, (name, capi.last_error())
            assert (uq[:, p:] == 7.0).all() and (vp[:, q:] == 7.0).all(), "written beyond a column"
            Q, P = uq[:, :p].T.copy(), vp[:, :q].T.copy()
            fig = np.array([np.abs(s - s_ref).max() / top, np.linalg.norm(B - (Q * s) @ P.T) / top, np.linalg.norm(Q.T @ Q - np.eye(p)),
                            np.linalg.norm(P.T @ P - np.eye(p))])
            worst = np.maximum(worst, fig)
            print(f"{p} x {q} {name} pad {pad}: values {fig[0]:.3g}, reconstruction {fig[1]:.3g}, Q {fig[2]:.3g}, P {fig[3]:.3g}")
            assert (fig <= MULTIPLE * MEASURED).all(), (name, p, q, pad, fig)
            assert (np.diff(s) <= 0).all() and (s >= 0).all(), (name, s)
            for c in range(p):          # the sign rule: the first component of largest magnitude of the left vector is positive
                assert Q[int(np.argmax(np.abs(Q[:, c]))), c] > 0, (name, c)
            s2, uq2, vp2 = np.zeros(p), np.full((p, lduq), 7.0), np.full((p, ldvp), 7.0)
            assert L.cvr_svd_host(p, q, b.ctypes.data, ldb, s2.ctypes.data, uq2.ctypes.data, lduq, vp2.ctypes.data, ldvp) == 0
            assert s2.tobytes() == s.tobytes() and uq2.tobytes() == uq.tobytes() and vp2.tobytes() == vp.tobytes(), "two calls differ"
            assert capi.svd_host(B, vectors=False).tobytes() == s.tobytes()
    print(f"{p} x {q}: worst figures: values {worst[0]:.3g}, reconstruction {worst[1]:.3g}, Q {worst[2]:.3g}, P {worst[3]:.3g}; measured maximum {MEASURED:.3g}")


def test_svd_host_ties_keep_their_order():
    s, Q, P = capi.svd_host(np.diag([3.0, 1.0, 3.0, 1.0]))
    assert s.tolist() == [3.0, 3.0, 1.0, 1.0]
    assert [int(np.argmax(Q[:, c])) for c in range(4)] == [0, 2, 1, 3] and (Q == P).all()


def test_solver_kernels_without_scratch_or_spills():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_svds.hip"))
    try:
        md = isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(r"((?:svds|lanczos)_\w+_kernel)<(float|double)", d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        # streaming passes live on occupancy: 128 VGPRs keep 4 wavefronts per SIMD, the limit tests/test_lanczos_host.py sets for the same group size.
        # Measured (hipcc for gfx950, this commit): svds_dots 72 (fp64) / 80 (fp32), svds_update 76 / 68, svds_begin and svds_finish 22 .. 30; the
        # restart product, Lanczos's kernel as it is, 96 / 128.
        assert item.get("vgpr_count", 999) <= 128, (d, item)
    # T x what a pass touches: the alignment of v0 at the start, the pass in the update, the half in the finish, the alignment of the output in the
    # restart product (Lanczos's kernel, as it is)
    assert {k: len(v) for k, v in seen.items()} == dict(lanczos_vv_kernel=4, svds_begin_kernel=4, svds_dots_kernel=2, svds_update_kernel=4,
                                                        svds_finish_kernel=4, lanczos_restart_kernel=4), seen
