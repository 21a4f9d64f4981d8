"""New values for a converted handle (cvr_options.mutable_values, cvr_update_values*) -- what can be checked without a GPU: the ABI
(exports, the option in the former reserved word, argument checks that come before any device work) and the update kernels' code for
gfx950 (both precisions, no scratch, no spills)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_library_exports_the_update_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in ("cvr_update_values_device", "cvr_update_values", "cvr_update_values_supported"):
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


def test_option_takes_the_first_reserved_word_and_defaults_to_off():
    assert C.sizeof(capi.Options) == 88
    assert capi.Options.reserved.offset == capi.Options.nvec.offset + 4
    o = capi.Options()
    C.memset(C.byref(o), 0x5a, C.sizeof(o))
    capi.lib().cvr_default_options(C.byref(o))
    assert o.mutable_values == 0 and list(o.reserved) == [0, 0]
    o.mutable_values = 1
    assert list(o.reserved) == [1, 0]          # the bytes of C's mutable_values, reserved[1] untouched


def _tiny_view(vals):
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([0, 1, 1], dtype=np.int32)
    v = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, vals.ctypes.data, 0, 0)
    return v, (rp, ci, vals)


def test_create_reads_the_option_and_refuses_a_dictionary_before_any_device_work():
    vals = np.ones(3)
    view, keep = _tiny_view(vals)
    L = capi.lib()
    for mv, vd in ((1, 1), (1, 7), (2, -1)):
        o = capi.Options()
        L.cvr_default_options(C.byref(o))
        o.mutable_values, o.value_dict = mv, vd
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), C.byref(o)) == capi.ERR_INVALID
        assert not h.value
        assert "mutable_values" in capi.last_error()
    del keep


def test_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    assert L.cvr_update_values_device(None, p, None) == capi.ERR_INVALID
    assert L.cvr_update_values_device(fake, None, None) == capi.ERR_INVALID
    assert L.cvr_update_values(None, p) == capi.ERR_INVALID
    assert L.cvr_update_values(fake, None) == capi.ERR_INVALID
    assert L.cvr_update_values_supported(None) == 0


def test_update_kernels_every_precision_without_scratch():
    import isa_check
    src = os.path.join(ROOT, "cvr_amd", "csrc", "cvr_update.hip")
    path = isa_check.compile_to_asm(src)
    try:
        lines = open(path).read().split("\n")
    finally:
        os.unlink(path)
    md = isa_check.metadata(lines)
    for kern in ("update_values_kernel", "value_map_kernel"):
        names = [n for n in md if kern in n]
        assert sorted(n.split(kern)[1][:2] for n in names) == ["Ij", "Iy"], names          # u32 (fp32) and u64 (fp64) bits
        for n in names:
            item = md[n]
            assert item.get("private_segment_fixed_size") == 0, (n, item)
            assert item.get("vgpr_spill_count", 0) == 0 and item.get("sgpr_spill_count", 0) == 0, (n, item)
    # the stream's value blocks are written with vector stores to global memory (no flat instructions: the address space is known)
    body = [ln.strip().split()[0] for ln in lines if ln.strip() and not ln.strip().startswith((";", "."))]
    assert not [op for op in body if op.startswith(("flat_", "scratch_"))]
