"""LSQR on the device (cvr_lsqr_device, cvr_lsqr) -- what can be checked without a GPU: the ABI (exports, the Python methods, the argument checks
that come before any device work and before a handle is looked at, in their order) and the code of the solver's vector kernels for gfx950 (every
fp32 / fp64 instantiation is there and runs without scratch or spills)."""
import ctypes as C
import os
import re
import subprocess
import sys

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_lsqr_device", "cvr_lsqr")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert re.search(r"}\s*cvr_lsqr_info;", hdr)
    assert C.sizeof(capi.LsqrInfo) == 24 and [f[0] for f in capi.LsqrInfo._fields_] == ["arnorm", "anorm", "stop_test", "reserved"]


def test_python_methods_exist():
    for name in ("lsqr", "lsqr_host"):
        assert callable(getattr(capi.CvrMatrix, name))


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_lsqr_device", lambda a, at, b, x, damp, o, r, i=None: L.cvr_lsqr_device(a, at, b, x, damp, o, r, i, None)),
            ("cvr_lsqr", lambda a, at, b, x, damp, o, r, i=None: L.cvr_lsqr(a, at, b, x, damp, o, r, i)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first look at neither handle)
    ok, res = _options(), capi.CgResult()
    for name, call in _calls():
        # cvr_cg_device's checks, on a, b, x, opt and res
        assert call(None, fake, p, p, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID, name
        assert call(fake, fake, None, p, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, None, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, 0.0, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, 0.0, C.byref(ok), None) == capi.ERR_INVALID
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, fake, p, p, 0.0, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, (name, bad)
        # a null handle of the transpose
        assert call(fake, None, p, p, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error() and "transpose" in capi.last_error()
        # a preconditioner
        assert call(fake, fake, p, p, 0.0, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error() and "cvr_lsqr" in capi.last_error()
        # damp
        for damp in (-1.0, -0.0 - 1e-300, float("nan"), float("inf"), -float("inf")):
            assert call(fake, fake, p, p, damp, C.byref(ok), C.byref(res)) == capi.ERR_INVALID, (name, damp)
            assert "damp" in capi.last_error()
        # the order: the solvers' own checks, then the null transpose, then minv_dev, then damp
        o = _options()
        o.reserved[0] = 1
        assert call(fake, None, p, p, -1.0, C.byref(o), C.byref(res)) == capi.ERR_INVALID
        assert "reserved" in capi.last_error()
        assert call(fake, None, p, p, -1.0, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        assert call(fake, fake, p, p, -1.0, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()


def test_solver_kernels_without_scratch_or_spills():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_lsqr.hip"))
    try:
        md = isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(r"(lsqr_\w+_kernel)<(float|double)", d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x alignment of the caller's array where a pass touches one: b at the start, x in the x kernel; T alone elsewhere
    assert {k: len(v) for k, v in seen.items()} == dict(lsqr_init_kernel=4, lsqr_v0_kernel=2, lsqr_start_kernel=2, lsqr_u_kernel=2, lsqr_v_kernel=2,
                                                        lsqr_x_kernel=4), seen
    for k, v in seen.items():
        assert {t for d in v for t in re.findall(r"_kernel<(float|double)", d)} == {"float", "double"}, (k, v)
    # three vector launches per step
    assert len(set(seen) - {"lsqr_init_kernel", "lsqr_v0_kernel", "lsqr_start_kernel"}) == 3
