"""MINRES on the device (cvr_minres_device, cvr_minres) -- what can be checked without a GPU: the ABI (exports, the Python methods, the argument checks
that come before any device work and before the handle is looked at, in their order) and the code of the solver's vector kernels for gfx950 (every
fp32 / fp64 instantiation is there and runs without scratch or spills)."""
import ctypes as C
import os
import re
import subprocess
import sys

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_minres_device", "cvr_minres")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert re.search(r"}\s*cvr_minres_info;", hdr)
    assert C.sizeof(capi.MinresInfo) == 24 and [f[0] for f in capi.MinresInfo._fields_] == ["anorm", "acond", "reserved"]
    assert "cvr_pminres" not in capi.SYMBOLS and not hasattr(L, "cvr_pminres_device")
    assert re.search(r"CVR_CG_BREAKDOWN 2[^#]*MINRES:", hdr), "the status comment has no MINRES line"


def test_python_methods_exist():
    for name in ("minres", "minres_host"):
        assert callable(getattr(capi.CvrMatrix, name))


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_minres_device", lambda h, b, x, shift, o, r, i=None: L.cvr_minres_device(h, b, x, shift, o, r, i, None)),
            ("cvr_minres", lambda h, b, x, shift, o, r, i=None: L.cvr_minres(h, b, x, shift, o, r, i)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    ok, res = _options(), capi.CgResult()
    for name, call in _calls():
        # cvr_cg_device's checks
        assert call(None, p, p, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID, name
        assert call(fake, None, p, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, None, 0.0, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, 0.0, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, 0.0, C.byref(ok), None) == capi.ERR_INVALID
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, p, p, 0.0, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, (name, bad)
        # shift, with a preconditioner too (minv_dev is allowed: it is not what fails)
        for shift in (float("nan"), float("inf"), -float("inf")):
            for o in (ok, _options(minv_dev=p.value)):
                assert call(fake, p, p, shift, C.byref(o), C.byref(res)) == capi.ERR_INVALID, (name, shift)
                assert "shift" in capi.last_error() and "cvr_minres" in capi.last_error()
        # the order: the solvers' own checks, then shift
        o = _options()
        o.reserved[0] = 1
        assert call(fake, p, p, float("nan"), C.byref(o), C.byref(res)) == capi.ERR_INVALID
        assert "reserved" in capi.last_error()
        assert call(None, p, p, float("nan"), C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()


def test_solver_kernels_without_scratch_or_spills():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_minres.hip"))
    try:
        md = isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(r"(minres_\w+_kernel)<(float|double)", d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x what a pass touches: minv and the alignment of b and minv at the start; the shift and r1 terms in the y' kernel; minv and its alignment in the
    # r kernel (no alignment without minv); the alignment of x in the x kernel; T alone in the kernel that builds the cell
    assert {k: len(v) for k, v in seen.items()} == dict(minres_init_kernel=8, minres_start_kernel=2, minres_yp_kernel=8, minres_r_kernel=6, minres_x_kernel=4), seen
    for k, v in seen.items():
        assert {t for d in v for t in re.findall(r"_kernel<(float|double)", d)} == {"float", "double"}, (k, v)
    # three vector launches per step
    assert len(set(seen) - {"minres_init_kernel", "minres_start_kernel"}) == 3
