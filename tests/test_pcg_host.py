"""The block-Jacobi preconditioner object and cvr_pcg_device / cvr_pcg -- what can be checked without a GPU: the ABI (exports, the ctypes view of the
structs against the header, the argument checks that come before any device work, cvr_precond_destroy(NULL)), the code of the new kernels for gfx950
(every fp32 / fp64 instantiation is there and runs without scratch or spills; the solver's own kernels in cvr_cg.hip are pinned by test_cg_host.py),
and the generator of the block-diagonal test family."""
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

NAMES = ("cvr_precond_block_jacobi", "cvr_precond_get_info", "cvr_precond_export", "cvr_precond_apply_device", "cvr_precond_destroy", "cvr_pcg_device",
         "cvr_pcg")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


def test_struct_sizes_match_the_header(tmp_path):
    """the ctypes struct against the C compiler's layout of include/cvr_amd.h"""
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cvr_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(cvr_precond_info), '
                   'offsetof(cvr_precond_info, block_size), offsetof(cvr_precond_info, is_f32), offsetof(cvr_precond_info, nblocks), '
                   'offsetof(cvr_precond_info, identity_blocks), offsetof(cvr_precond_info, device), CVR_PRECOND_MAX_BLOCK); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = capi.PrecondInfo
    assert got == [C.sizeof(P), P.block_size.offset, P.is_f32.offset, P.nblocks.offset, P.identity_blocks.offset, P.device.offset, capi.PRECOND_MAX_BLOCK]


def _view(nrows=4, ncols=4):
    rp = np.arange(nrows + 1, dtype=np.int64)
    ci = np.arange(nrows, dtype=np.int32)
    va = np.ones(nrows)
    return capi.CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0), (rp, ci, va)


def test_precond_argument_checks_come_before_any_device_work():
    L = capi.lib()
    view, keep = _view()
    out = C.c_void_p()
    assert L.cvr_precond_block_jacobi(None, C.byref(view), 2, 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_block_jacobi(C.byref(out), None, 2, 0, None) == capi.ERR_INVALID
    assert "null" in capi.last_error()
    for bs in (0, -1, capi.PRECOND_MAX_BLOCK + 1):
        out = C.c_void_p(1)
        assert L.cvr_precond_block_jacobi(C.byref(out), C.byref(view), bs, 0, None) == capi.ERR_INVALID, bs
        assert "block_size" in capi.last_error() and not out.value
    rect, keep2 = _view(4, 5)
    assert L.cvr_precond_block_jacobi(C.byref(out), C.byref(rect), 2, 0, None) == capi.ERR_INVALID
    assert "square" in capi.last_error()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the object)
    assert L.cvr_precond_apply_device(None, p, C.c_void_p(p.value + 8), None) == capi.ERR_INVALID
    assert L.cvr_precond_apply_device(fake, None, p, None) == capi.ERR_INVALID
    assert L.cvr_precond_apply_device(fake, p, None, None) == capi.ERR_INVALID
    assert L.cvr_precond_apply_device(fake, p, p, None) == capi.ERR_INVALID
    assert "same array" in capi.last_error()
    info = capi.PrecondInfo()
    assert L.cvr_precond_get_info(None, C.byref(info)) == capi.ERR_INVALID
    assert L.cvr_precond_get_info(fake, None) == capi.ERR_INVALID
    assert L.cvr_precond_export(None, p) == capi.ERR_INVALID
    assert L.cvr_precond_export(fake, None) == capi.ERR_INVALID
    del keep, keep2


def test_destroying_a_null_object_is_ok():
    assert capi.lib().cvr_precond_destroy(None) == capi.OK
    capi.Precond().close()          # (an object that was never built)


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_pcg_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first look neither at the handle nor at the object)
    ok, res = _options(), capi.CgResult()
    for call in (lambda h, pc, b, x, o, r: L.cvr_pcg_device(h, pc, b, x, o, r, None), L.cvr_pcg):
        assert call(None, fake, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, None, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, None, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        assert call(fake, None, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, fake, p, p, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, fake, p, p, C.byref(o), C.byref(res)) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()
        assert call(fake, fake, p, p, C.byref(_options(minv_dev=p.value)), C.byref(res)) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()
        # cvr_cg_device's checks come first: a bad option beside a null object is the option's error
        o = _options()
        o.reserved[0] = 1
        assert call(fake, None, p, p, C.byref(o), C.byref(res)) == capi.ERR_INVALID
        assert "reserved" in capi.last_error()


def test_block_diag_spd_is_what_it_says():
    for n, bs in ((96, 8), (21, 4), (5, 8)):
        for dtype in (np.float64, np.float32):
            n2, nc, rp, ci, va = synth.block_diag_spd(n, bs, cond=1e3, dtype=dtype)
            assert (n2, nc) == (n, n) and va.dtype == dtype and rp[-1] == len(ci) == len(va)
            rows = np.repeat(np.arange(n), np.diff(rp))
            assert (rows // bs == ci // bs).all(), "an entry outside the blocks"
            A = np.zeros((n, n))
            A[rows, ci] = va
            assert np.array_equal(A, A.T)
            ev = np.linalg.eigvalsh(A.astype(np.float64))
            assert ev[0] >= 1 - 1e-3 and ev[-1] <= 1e3 * (1 + 1e-3), (ev[0], ev[-1])
            if n % bs == 0:
                assert len(np.unique(np.round(ev, 6))) > n // 2          # (not a handful of eigenvalues: plain CG has work to do)


@pytest.fixture(scope="module")
def precond_md():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_precond.hip"))
    try:
        yield isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def test_new_kernels_without_scratch_or_spills(precond_md):
    names = list(precond_md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in precond_md.items():
        d = dem[name]
        m = re.search(r"((?:precond|pcg|cg)_\w+_kernel)(?:<(float|double)[^>]*>)?", d)          # (pcg before cg: pcg_apply_kernel is no cg_* kernel)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)
    # T for the build; T x alignment of the caller's z for the plain apply; T x (start, step) for the fused one -- and no cg_* kernel: the solver
    # that enqueues pcg_apply_kernel is cvr_cg.hip's, whose kernels test_cg_host.py pins
    assert {k: len(v) for k, v in seen.items()} == dict(precond_build_kernel=2, precond_apply_kernel=4, pcg_apply_kernel=4), seen
    assert precond_md and all(item.get("group_segment_fixed_size", 0) <= 20 * 1024 for item in precond_md.values())
