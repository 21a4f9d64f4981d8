"""The block eigensolver (cvr_lobpcg_device, cvr_lobpcg) -- what can be checked without a GPU: the ABI (exports, struct sizes and field order, the
Python methods, the default options, the argument checks that come before any device work and before the handle is looked at, in their order)."""
import ctypes as C
import os
import re

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvr_lobpcg_device", "cvr_lobpcg")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert hasattr(L, "cvr_lobpcg_default_options") and "cvr_lobpcg_default_options" in capi.SYMBOLS and re.search(r"\bvoid cvr_lobpcg_default_options\(", hdr)
    assert re.search(r"}\s*cvr_lobpcg_options;", hdr) and re.search(r"}\s*cvr_lobpcg_result;", hdr)
    assert C.sizeof(capi.LobpcgOptions) == 40 and [f[0] for f in capi.LobpcgOptions._fields_] == ["nev", "which", "max_iters", "reserved0", "tol", "reserved"]
    assert C.sizeof(capi.LobpcgResult) == 40
    assert [f[0] for f in capi.LobpcgResult._fields_] == ["nconv", "status", "iterations", "spmv_count", "precond_applies", "restarts_without_p", "seconds",
                                                          "max_rel_residual"]
    # CVR_EIG_MAX_ITERS is a value no other CVR_EIG_* status has
    status = {name: int(v) for name, v in re.findall(r"#define (CVR_EIG_(?:CONVERGED|MAX_RESTARTS|BREAKDOWN|INVARIANT|MAX_ITERS))\s+(\d+)", hdr)}
    assert len(status) == 5 and len(set(status.values())) == 5 and status["CVR_EIG_MAX_ITERS"] == capi.EIG_MAX_ITERS, status
    assert re.search(r"#define CVR_LOBPCG_MAX_BLOCK\s+8\b", hdr) and capi.LOBPCG_MAX_BLOCK == 8
    doc = hdr[hdr.index("LOBPCG"):]
    for word in ("locking", "generalised", "constraints", "cvr_spmm_device", "more than\n * 8 columns", "cvr_eigsh is unchanged", "HIP graph"):
        assert word in doc, word


def test_default_options():
    o = capi.LobpcgOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    capi.lib().cvr_lobpcg_default_options(C.byref(o))
    assert (o.nev, o.which, o.max_iters, o.reserved0, o.tol, list(o.reserved)) == (1, capi.EIG_SMALLEST, 200, 0, 1e-8, [0, 0, 0, 0])


def test_python_methods_exist():
    for name in ("lobpcg", "lobpcg_host"):
        assert callable(getattr(capi.CvrMatrix, name))


def _options(**kw):
    o = capi.LobpcgOptions()
    capi.lib().cvr_lobpcg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_lobpcg_device", lambda h, p, x, ldx, e, r, o, res: L.cvr_lobpcg_device(h, p, x, ldx, e, r, o, res, None)),
            ("cvr_lobpcg", lambda h, p, x, ldx, e, r, o, res: L.cvr_lobpcg(h, p, x, ldx, e, r, o, res)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first look at neither the handle nor the object)
    ok, res = _options(), capi.LobpcgResult()
    for name, call in _calls():
        def bad(what, *a):
            assert call(*a) == capi.ERR_INVALID, (name, what)
            assert what in capi.last_error(), (name, what, capi.last_error())
        bad("null h", None, None, p, 64, p, p, C.byref(ok), C.byref(res))
        bad("null X", fake, None, None, 64, p, p, C.byref(ok), C.byref(res))
        bad("null evals", fake, None, p, 64, None, p, C.byref(ok), C.byref(res))
        bad("null resnorms", fake, None, p, 64, p, None, C.byref(ok), C.byref(res))
        bad("null opt", fake, None, p, 64, p, p, None, C.byref(res))
        bad("null res", fake, None, p, 64, p, p, C.byref(ok), None)
        for nev in (0, -3, 9):
            bad("nev", fake, None, p, 64, p, p, C.byref(_options(nev=nev)), C.byref(res))
        for which in (-1, 2):
            bad("which", fake, None, p, 64, p, p, C.byref(_options(which=which)), C.byref(res))
        bad("max_iters", fake, None, p, 64, p, p, C.byref(_options(max_iters=-1)), C.byref(res))
        for tol in (-1.0, float("nan"), float("inf")):
            bad("tol", fake, None, p, 64, p, p, C.byref(_options(tol=tol)), C.byref(res))
        bad("reserved0", fake, None, p, 64, p, p, C.byref(_options(reserved0=1)), C.byref(res))
        o = _options()
        o.reserved[2] = 1
        bad("reserved[2]", fake, None, p, 64, p, p, C.byref(o), C.byref(res))
        for ldx in (0, -5):
            bad("ldx", fake, None, p, ldx, p, p, C.byref(ok), C.byref(res))
        bad("CVR_EIG_LARGEST", fake, fake, p, 64, p, p, C.byref(_options(which=capi.EIG_LARGEST)), C.byref(res))
        # the order: every check fails at once -> the first one named; then one by one
        o = _options(nev=0, which=7, max_iters=-1, tol=-1.0, reserved0=3)
        o.reserved[0] = 1
        bad("null X", fake, fake, None, 0, None, None, C.byref(o), None)
        bad("null evals", fake, fake, p, 0, None, None, C.byref(o), None)
        bad("null resnorms", fake, fake, p, 0, p, None, C.byref(o), None)
        bad("null res", fake, fake, p, 0, p, p, C.byref(o), None)
        bad("nev", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.nev = 8
        bad("which", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.which = capi.EIG_LARGEST
        bad("max_iters", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.max_iters = 0
        bad("tol", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.tol = 0.0
        bad("reserved0", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.reserved0 = 0
        bad("reserved[0]", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        o.reserved[0] = 0
        bad("ldx", fake, fake, p, 0, p, p, C.byref(o), C.byref(res))
        bad("CVR_EIG_LARGEST", fake, fake, p, 1, p, p, C.byref(o), C.byref(res))
