"""Batched conjugate gradients (cvr_cg_multi_device, cvr_cg_multi) -- what can be checked without a GPU: the ABI (exports, the argument checks
that come before any device work and before the handle is looked at), the code of the block solver's vector kernels for gfx950 (every fp32 /
fp64 instantiation is there and runs without scratch or spills inside a streaming pass's register budget), and the single-vector solvers'
kernel counts, which the block solver leaves alone (it shares cvr_krylov.h with them and adds nothing to their translation units)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_cg_multi_device", "cvr_cg_multi")


def test_library_exports_the_block_solver():
    L = C.CDLL(capi.lib_path())
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert callable(capi.CvrMatrix.cg_multi) and callable(capi.CvrMatrix.cg_multi_host)


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
    ok, res = _options(), (capi.CgResult * 8)()

    def device(h, b, x, o, r, nvec=2, ldb=2, ldx=2):
        return L.cvr_cg_multi_device(h, b, ldb, x, ldx, nvec, o, r, None)

    def host(h, b, x, o, r, nvec=2, ldb=None, ldx=None):
        return L.cvr_cg_multi(h, b, x, nvec, o, r)
    for call in (device, host):
        # check_solver_args' checks
        assert call(None, p, p, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, None, p, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, p, None, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, p, p, None, res) == capi.ERR_INVALID
        assert call(fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, p, p, C.byref(_options(**bad)), res) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, p, p, C.byref(o), res) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()
        # the block's own: nvec outside 1 .. 8
        for nvec in (0, -1, 9, 16):
            assert call(fake, p, p, C.byref(ok), res, nvec=nvec, ldb=16, ldx=16) == capi.ERR_INVALID, nvec
            assert "nvec" in capi.last_error()
    # ... and a leading dimension below nvec (the host twin has none: ld = nvec)
    for nvec, ldb, ldx in ((2, 1, 2), (2, 2, 1), (8, 7, 8), (8, 8, 0), (3, -3, 3)):
        assert device(fake, p, p, C.byref(ok), res, nvec=nvec, ldb=ldb, ldx=ldx) == capi.ERR_INVALID, (nvec, ldb, ldx)
        assert "ldb" in capi.last_error() and "ldx" in capi.last_error()
    # the options are looked at before the block's shape: a bad option with a bad nvec is the option's error
    assert device(fake, p, p, C.byref(_options(rtol=-1.0)), res, nvec=9) == capi.ERR_INVALID
    assert "rtol" in capi.last_error()


@pytest.fixture(scope="module")
def isa():
    import isa_check
    return isa_check


def _metadata(isa, name):
    path = isa.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", name))
    try:
        return isa.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def _demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def _by_kernel(md, prefix):
    dem = _demangled(list(md))
    seen = {}
    for name in md:
        m = re.search(r"(?<!\w)(p?%s_\w+_kernel)" % prefix, dem[name])          # (anchored: cvr_bicgstab.hip's pbicg_apply_kernel is no bicg_* kernel)
        assert m, dem[name]
        seen.setdefault(m.group(1), []).append(dem[name])
    return dem, seen


def test_block_solver_kernels_without_scratch_or_spills(isa):
    md = _metadata(isa, "cvr_cg_multi.hip")
    dem, seen = _by_kernel(md, "cgm")
    for name, item in md.items():
        d = dem[name]
        print(item.get("vgpr_count"), d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x preconditioner x 16-byte packets in the library's blocks x in the caller's, where a pass touches each; the strided copy-in and the
    # b == 0 columns' clear by T
    assert {k: len(v) for k, v in seen.items()} == dict(cgm_start_kernel=2, cgm_zero_kernel=2, cgm_init_kernel=16, cgm_check_kernel=1, cgm_pq_kernel=4,
                                                        cgm_update_kernel=16, cgm_direction_kernel=8), seen
    for k, v in seen.items():
        if k != "cgm_check_kernel":
            assert any("<float" in d for d in v) and any("<double" in d for d in v), k
    # among them the forms the solver launches with a block-Jacobi object (test_pcg_multi_host.py): PRE = false in the update, r.z in the direction
    assert len([d for d in seen["cgm_update_kernel"] if "false" in d.split("cgm_update_kernel<")[1].split(",")[1]]) == 8
    assert len([d for d in seen["cgm_direction_kernel"] if "true" in d.split("cgm_direction_kernel<")[1].split(",")[1]]) == 4
    # three vector launches per step beside the product
    assert set(seen) - {"cgm_start_kernel", "cgm_zero_kernel", "cgm_init_kernel", "cgm_check_kernel"} == {"cgm_pq_kernel", "cgm_update_kernel", "cgm_direction_kernel"}


def test_single_vector_solvers_kernel_counts_unchanged(isa):
    """what test_cg_host and test_bicgstab_host pin for cvr_cg.hip and cvr_bicgstab.hip"""
    _, cg = _by_kernel(_metadata(isa, "cvr_cg.hip"), "cg")
    assert {k: len(v) for k, v in cg.items()} == dict(cg_init_kernel=8, cg_check_kernel=1, cg_pq_kernel=2, cg_update_kernel=8, cg_direction_kernel=4), cg
    _, bi = _by_kernel(_metadata(isa, "cvr_bicgstab.hip"), "bicg")
    assert {k: len(v) for k, v in bi.items() if k.startswith("bicg_")} == dict(bicg_init_kernel=8, bicg_check_kernel=1, bicg_rv_kernel=2, bicg_s_kernel=6,
                                                                               bicg_half_kernel=4, bicg_update_kernel=8, bicg_direction_kernel=6), bi
