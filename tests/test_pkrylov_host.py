"""cvr_pbicgstab_device / cvr_pbicgstab and cvr_pgmres_device / cvr_pgmres -- what can be checked without a GPU: the ABI (exports, the Python methods,
the argument checks that come before any device work, in their order), the code of the new kernels for gfx950 (every fp32 / fp64 instantiation is
there and runs without scratch or spills; they live in cvr_bicgstab.hip and cvr_gmres.hip, whose own kernels are pinned by their own host tests),
and the generator of the nonsymmetric block-diagonal test family."""
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

NAMES = ("cvr_pbicgstab_device", "cvr_pbicgstab", "cvr_pgmres_device", "cvr_pgmres")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert re.search(r"#define\s+CVR_GMRES_MAX_RESTART\s+%d\b" % capi.GMRES_MAX_RESTART, hdr)


def test_python_methods_exist():
    for name in ("pbicgstab", "pbicgstab_host", "pgmres", "pgmres_host"):
        assert callable(getattr(capi.CvrMatrix, name))


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls():
    L = capi.lib()
    return (("cvr_pbicgstab_device", None, lambda h, pc, b, x, o, r, m=None: L.cvr_pbicgstab_device(h, pc, b, x, o, r, None)),
            ("cvr_pbicgstab", None, lambda h, pc, b, x, o, r, m=None: L.cvr_pbicgstab(h, pc, b, x, o, r)),
            ("cvr_pgmres_device", 30, lambda h, pc, b, x, o, r, m=30: L.cvr_pgmres_device(h, pc, b, x, m, o, r, None)),
            ("cvr_pgmres", 30, lambda h, pc, b, x, o, r, m=30: L.cvr_pgmres(h, pc, b, x, m, o, r)))


def test_argument_checks_come_before_any_device_work_in_their_order():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first look neither at the handle nor at the object)
    ok, res = _options(), capi.CgResult()
    for name, restart, call in _calls():
        assert call(None, fake, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID, name
        assert call(fake, fake, None, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, None, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, fake, p, p, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, (name, bad)
        # a null object
        assert call(fake, None, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        # minv_dev beside the object
        assert call(fake, fake, p, p, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error() and name.replace("_device", "") in capi.last_error()
        # the solver's own checks come first: a bad option beside a null object is the option's error
        o = _options()
        o.reserved[0] = 1
        assert call(fake, None, p, p, C.byref(o), C.byref(res)) == capi.ERR_INVALID
        assert "reserved" in capi.last_error()
        # the null object comes before minv_dev
        assert call(fake, None, p, p, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        if restart is None:
            continue
        for m in (0, -1, capi.GMRES_MAX_RESTART + 1):
            assert call(fake, fake, p, p, C.byref(ok), C.byref(res), m) == capi.ERR_INVALID, (name, m)
            assert "restart" in capi.last_error()
        # ... and both before the restart
        assert call(fake, None, p, p, C.byref(ok), C.byref(res), 0) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        assert call(fake, fake, p, p, C.byref(_options(minv_dev=p.value)), C.byref(res), 0) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()


def _metadata(src):
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", src))
    try:
        md = isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    return md, dem


def _counts(src, pattern):
    md, dem = _metadata(src)
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(pattern, d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)
    return seen


def _types(ds):
    return {t for d in ds for t in re.findall(r"_kernel<(float|double)", d)}


def _forms(ds, *flags):
    """the instantiations among ds whose template arguments behind T begin with `flags`"""
    want = ", ".join(("true" if f else "false") for f in flags)
    return [d for d in ds if re.search(r"_kernel<(?:float|double), %s[,>]" % want, d)]


def test_pbicgstab_kernels_without_scratch_or_spills():
    # (the alternation tries pbicg first, so pbicg_apply_kernel is not taken for a bicg_* kernel)
    seen = _counts("cvr_bicgstab.hip", r"((?:pbicg|bicg)_\w+_kernel)(?:<(float|double)[^>]*>)?")
    # T for the apply; beside it, among the bicg_* kernels of the merged file (test_bicgstab_host.py pins all of them), the forms the solver launches
    # with an object: no diagonal (PRE = false) in the start, s and the direction, s^ from its own buffer (PRE = true) in the update, T x alignment of
    # the caller's b and x where a kernel touches them
    assert len(seen["pbicg_apply_kernel"]) == 2, seen
    assert len(_forms(seen["bicg_init_kernel"], False)) == 4 and len(seen["bicg_check_kernel"]) == 1 and len(seen["bicg_rv_kernel"]) == 2, seen
    assert len(_forms(seen["bicg_s_kernel"], False, True)) == 2 and len(seen["bicg_half_kernel"]) == 4, seen
    assert len(_forms(seen["bicg_update_kernel"], True)) == 4 and len(_forms(seen["bicg_direction_kernel"], False, True)) == 2, seen
    assert set(seen) == {"pbicg_apply_kernel", "bicg_init_kernel", "bicg_check_kernel", "bicg_rv_kernel", "bicg_s_kernel", "bicg_half_kernel",
                         "bicg_update_kernel", "bicg_direction_kernel"}, seen
    for k, v in seen.items():
        if k != "bicg_check_kernel":
            assert _types(v) == {"float", "double"}, (k, v)
    for k, v in (("bicg_init_kernel", _forms(seen["bicg_init_kernel"], False)), ("bicg_s_kernel", _forms(seen["bicg_s_kernel"], False, True)),
                 ("bicg_update_kernel", _forms(seen["bicg_update_kernel"], True)), ("bicg_direction_kernel", _forms(seen["bicg_direction_kernel"], False, True))):
        assert _types(v) == {"float", "double"}, (k, v)


def test_pgmres_kernels_without_scratch_or_spills():
    seen = _counts("cvr_gmres.hip", r"((?:pgmres|gmres)_\w+_kernel)<(float|double)")
    # T for the apply and the u kernel, T x alignment of the caller's x for the x kernel; beside them, among the gmres_* kernels of the merged file
    # (test_gmres_host.py pins them), the forms without a diagonal that the solver launches with an object
    assert {k: len(seen[k]) for k in ("pgmres_apply_kernel", "pgmres_u_kernel", "pgmres_x_kernel")} == dict(pgmres_apply_kernel=2, pgmres_u_kernel=2, pgmres_x_kernel=4), seen
    assert len(seen["gmres_dots_kernel"]) == 2 and len(seen["gmres_update_kernel"]) == 4 and len(seen["gmres_rr_kernel"]) == 6, seen
    assert len(_forms(seen["gmres_finish_kernel"], False, True)) == 2 and len(_forms(seen["gmres_begin_kernel"], False, True)) == 2, seen
    # (gmres_x_kernel is in the merged file for the plain and diagonal forms, so its absence from the object's path no longer shows in the
    # instantiations: tests/test_gpu_pgmres.py holds cvr_pgmres_device to its model step by step, where x is W u and not u)
    assert set(seen) == {"pgmres_apply_kernel", "pgmres_u_kernel", "pgmres_x_kernel", "gmres_dots_kernel", "gmres_update_kernel", "gmres_finish_kernel",
                         "gmres_rr_kernel", "gmres_begin_kernel", "gmres_x_kernel"}, seen
    for k, v in seen.items():
        assert _types(v) == {"float", "double"}, (k, v)
    for v in (_forms(seen["gmres_finish_kernel"], False, True), _forms(seen["gmres_begin_kernel"], False, True)):
        assert _types(v) == {"float", "double"}, v


def test_block_diag_nonsym_is_what_it_says():
    for n, bs in ((96, 8), (21, 4), (5, 8), (7, 1)):
        for dtype in (np.float64, np.float32):
            n2, nc, rp, ci, va = synth.block_diag_nonsym(n, bs, cond=1e3, dtype=dtype)
            assert (n2, nc) == (n, n) and va.dtype == dtype and rp[-1] == len(ci) == len(va)
            rows = np.repeat(np.arange(n), np.diff(rp))
            assert (rows // bs == ci // bs).all(), "an entry outside the blocks"
            assert len(ci) == (n // bs) * bs * bs + (n % bs) ** 2          # every block is dense, the short last one too
            A = np.zeros((n, n))
            A[rows, ci] = va
            tol = 1e-9 if dtype == np.float64 else 1e-3
            for k in range(-(-n // bs)):
                B = A[k * bs:(k + 1) * bs, k * bs:(k + 1) * bs]
                sv = np.linalg.svd(B.astype(np.float64), compute_uv=False)
                m = len(B)
                assert abs(sv[-1] - 1) <= tol and abs(sv[0] - (1e3 if m > 1 else 1)) <= tol * 1e3, (n, bs, k, sv[0], sv[-1])
                if m > 1:
                    assert not np.array_equal(B, B.T), (n, bs, k)
    a, b = synth.block_diag_nonsym(96, 8, seed=1)[4], synth.block_diag_nonsym(96, 8, seed=2)[4]
    assert not np.array_equal(a, b)
