"""The thick-restart Lanczos eigensolver (cvr_eigsh_device, cvr_eigsh, cvr_sym_eig_host) -- what can be checked without a GPU: the ABI (exports, struct
sizes and field order, the Python methods, the argument checks that come before any device work and before the handle is looked at, in their order)
and the code of the solver's vector kernels for gfx950 (every fp32 / fp64 instantiation is there and runs without scratch or spills)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_eigsh_device", "cvr_eigsh", "cvr_sym_eig_host")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert hasattr(L, "cvr_eig_default_options") and "cvr_eig_default_options" in capi.SYMBOLS and re.search(r"\bvoid cvr_eig_default_options\(", hdr)
    assert re.search(r"}\s*cvr_eig_options;", hdr) and re.search(r"}\s*cvr_eig_result;", hdr)
    assert C.sizeof(capi.EigOptions) == 40 and [f[0] for f in capi.EigOptions._fields_] == ["nev", "ncv", "which", "max_restarts", "tol", "reserved"]
    assert C.sizeof(capi.EigResult) == 32 and [f[0] for f in capi.EigResult._fields_] == ["nconv", "status", "restarts", "spmv_count", "seconds", "max_estimate"]
    for name, value in (("CVR_EIG_MAX_NCV", 64), ("CVR_EIG_LARGEST", 0), ("CVR_EIG_SMALLEST", 1), ("CVR_EIG_CONVERGED", 0), ("CVR_EIG_MAX_RESTARTS", 1),
                        ("CVR_EIG_BREAKDOWN", 2), ("CVR_EIG_INVARIANT", 3)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), hdr), name
    assert (capi.EIG_MAX_NCV, capi.EIG_LARGEST, capi.EIG_SMALLEST, capi.EIG_CONVERGED, capi.EIG_MAX_RESTARTS, capi.EIG_BREAKDOWN, capi.EIG_INVARIANT) == (64, 0, 1, 0, 1, 2, 3)
    # eps23 is a decimal literal of the header: ARPACK's eps^(2/3), not a pow call
    m = re.search(r"#define CVR_EIG_EPS23\s+([0-9.e+-]+)", hdr)
    assert m and float(m.group(1)) == capi.EIG_EPS23 and abs(capi.EIG_EPS23 / (2.0 ** -52) ** (2.0 / 3.0) - 1) < 1e-14
    assert "HIP graph" in hdr[hdr.index("CVR_EIG_MAX_NCV"):]


def test_default_options():
    o = capi.EigOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    capi.lib().cvr_eig_default_options(C.byref(o))
    assert (o.nev, o.ncv, o.which, o.max_restarts, o.tol, list(o.reserved)) == (1, 0, capi.EIG_LARGEST, 100, 1e-8, [0, 0, 0, 0])


def test_python_methods_exist():
    for name in ("eigsh", "eigsh_host"):
        assert callable(getattr(capi.CvrMatrix, name))
    assert callable(capi.sym_eig_host)
    w, Z = capi.sym_eig_host(np.array([[2.0, 99.0], [1.0, 2.0]]))          # the upper triangle is never read
    assert np.allclose(w, [1.0, 3.0]) and np.allclose(np.abs(Z), np.sqrt(0.5)) and Z[0, 0] > 0 and Z[0, 1] > 0
    assert capi.sym_eig_host(np.array([[5.0]]), vectors=False).tolist() == [5.0]


def _options(**kw):
    o = capi.EigOptions()
    capi.lib().cvr_eig_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_eigsh_device", lambda h, v, e, z, ldv, o, r: L.cvr_eigsh_device(h, v, e, z, ldv, o, r, None)),
            ("cvr_eigsh", lambda h, v, e, z, ldv, o, r: L.cvr_eigsh(h, v, e, z, ldv, o, r)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    ok, res = _options(), capi.EigResult()
    for name, call in _calls():
        def bad(what, *a):
            assert call(*a) == capi.ERR_INVALID, (name, what)
            assert what in capi.last_error(), (name, what, capi.last_error())
        bad("null h", None, p, p, p, 64, C.byref(ok), C.byref(res))
        bad("null v0", fake, None, p, p, 64, C.byref(ok), C.byref(res))
        bad("null evals", fake, p, None, p, 64, C.byref(ok), C.byref(res))
        bad("null opt", fake, p, p, p, 64, None, C.byref(res))
        bad("null res", fake, p, p, p, 64, C.byref(ok), None)
        for nev in (0, -3):
            bad("nev", fake, p, p, p, 64, C.byref(_options(nev=nev)), C.byref(res))
        for nev, ncv in ((1, 1), (1, 2), (3, 4), (1, 65), (1, -1), (63, 64)):
            bad("ncv", fake, p, p, p, 64, C.byref(_options(nev=nev, ncv=ncv)), C.byref(res))
        for which in (-1, 2):
            bad("which", fake, p, p, p, 64, C.byref(_options(which=which)), C.byref(res))
        bad("max_restarts", fake, p, p, p, 64, C.byref(_options(max_restarts=-1)), C.byref(res))
        for tol in (-1.0, float("nan"), float("inf")):
            bad("tol", fake, p, p, p, 64, C.byref(_options(tol=tol)), C.byref(res))
        o = _options()
        o.reserved[2] = 1
        bad("reserved", fake, p, p, p, 64, C.byref(o), C.byref(res))
        for ldv in (0, -5):
            bad("ldv", fake, p, p, p, ldv, C.byref(ok), C.byref(res))
        # the order: every check fails at once -> the first one named; then one by one
        o = _options(nev=0, ncv=1, which=7, max_restarts=-1, tol=-1.0)
        o.reserved[0] = 1
        bad("null v0", fake, None, None, p, 0, C.byref(o), None)
        bad("null evals", fake, p, None, p, 0, C.byref(o), None)
        bad("null res", fake, p, p, p, 0, C.byref(o), None)
        bad("nev", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.nev = 1
        bad("ncv", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.ncv = 0
        bad("which", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.which = capi.EIG_SMALLEST
        bad("max_restarts", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.max_restarts = 0
        bad("tol", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.tol = 0.0
        bad("reserved", fake, p, p, p, 0, C.byref(o), C.byref(res))
        o.reserved[0] = 0
        bad("ldv", fake, p, p, p, 0, C.byref(o), C.byref(res))


def test_sym_eig_host_argument_checks():
    L = capi.lib()
    a, w, z = np.eye(3, order="F"), np.zeros(3), np.zeros((3, 3), order="F")
    assert L.cvr_sym_eig_host(3, a.ctypes.data, 3, w.ctypes.data, z.ctypes.data, 3) == 0 and w.tolist() == [1.0, 1.0, 1.0]
    for m, lda, ldz, ap, wp in ((0, 3, 3, a.ctypes.data, w.ctypes.data), (65, 65, 65, a.ctypes.data, w.ctypes.data), (3, 2, 3, a.ctypes.data, w.ctypes.data),
                                (3, 3, 2, a.ctypes.data, w.ctypes.data), (3, 3, 3, None, w.ctypes.data), (3, 3, 3, a.ctypes.data, None)):
        assert L.cvr_sym_eig_host(m, ap, lda, wp, z.ctypes.data, ldz) == capi.ERR_INVALID, (m, lda, ldz)
    a[2, 0] = np.nan
    assert L.cvr_sym_eig_host(3, a.ctypes.data, 3, w.ctypes.data, z.ctypes.data, 3) == capi.ERR_INVALID and "finite" in capi.last_error()
    a[2, 0], a[0, 2] = 0.0, np.nan          # the other triangle is not looked at
    assert L.cvr_sym_eig_host(3, a.ctypes.data, 3, w.ctypes.data, None, 0) == 0


def test_solver_kernels_without_scratch_or_spills():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_lanczos.hip"))
    try:
        md = isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(r"(lanczos_\w+_kernel)<(float|double)", d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x what a pass touches: the alignment of v0 at the start, the pass in the update, the alignment of the output in the restart product
    assert {k: len(v) for k, v in seen.items()} == dict(lanczos_vv_kernel=4, lanczos_begin_kernel=4, lanczos_dots_kernel=2, lanczos_update_kernel=4,
                                                        lanczos_finish_kernel=2, lanczos_restart_kernel=4), seen
    for k, v in seen.items():
        assert {t for d in v for t in re.findall(r"_kernel<(float|double)", d)} == {"float", "double"}, (k, v)
    # five vector launches of three kernels per step; the restart product is the one new pass over the basis
    assert len(set(seen) - {"lanczos_vv_kernel", "lanczos_begin_kernel", "lanczos_restart_kernel"}) == 3
