"""The handle of A^T built on the device (cvr_options.transpose) -- what can be checked without a GPU: the ABI (the option in the last
reserved word, its default, the header's field), the refusals that come before any device work, and the transpose kernels' code for gfx950
(no scratch, no spills)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_option_takes_the_last_reserved_word_and_defaults_to_off():
    assert C.sizeof(capi.Options) == 88
    assert capi.Options.reserved.offset == capi.Options.nvec.offset + 4 and capi.Options.reserved.size == 8
    o = capi.Options()
    C.memset(C.byref(o), 0x5a, C.sizeof(o))
    capi.lib().cvr_default_options(C.byref(o))
    assert o.transpose == 0 and list(o.reserved) == [0, 0]
    o.transpose = 1
    assert list(o.reserved) == [0, 1]          # the bytes of C's transpose (offset 80, 4 bytes, the struct's last); mutable_values untouched
    assert capi.Options.reserved.offset + 4 == 80 and C.sizeof(capi.Options) == 80 + 4 + 4          # (+ the tail padding to 8)


def test_header_declares_the_field_and_no_reserved_word_is_left():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    body = hdr[hdr.index("typedef struct {\n    int32_t device;"):hdr.index("} cvr_options;")]
    fields = re.findall(r"^\s*(?:int32_t|int64_t)\s+(\w+)(\[\d+\])?;", body, re.M)
    assert fields[-2:] == [("mutable_values", ""), ("transpose", "")]
    assert not [f for f in fields if f[0].startswith("reserved")]
    assert "no reserved word is left" in body


def _tiny_view(on_device=0):
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([0, 1, 1], dtype=np.int32)
    va = np.ones(3)
    return capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, on_device), (rp, ci, va)


@pytest.mark.parametrize("value", [2, -1, 7])
def test_create_refuses_other_values_before_any_device_work(value):
    L = capi.lib()
    for on_device in (0, 1):
        view, keep = _tiny_view(on_device)
        o = capi.Options()
        L.cvr_default_options(C.byref(o))
        o.transpose = value
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), C.byref(o)) == capi.ERR_INVALID
        assert not h.value
        assert "transpose" in capi.last_error()
        best = capi.Options()
        assert L.cvr_tune(C.byref(view), C.byref(o), C.byref(best), None, None) == capi.ERR_INVALID
        del keep


def test_create_checks_a_and_the_limits_before_any_device_work():
    L = capi.lib()
    o = capi.Options()
    L.cvr_default_options(C.byref(o))
    o.transpose = 1
    h = C.c_void_p()
    # a malformed CSR of A: the same checks and codes as without the option
    rp = np.array([0, 2, 1], dtype=np.int64)
    ci = np.array([0, 1, 1], dtype=np.int32)
    va = np.ones(3)
    bad = capi.CsrView(2, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_create(C.byref(h), C.byref(bad), C.byref(o)) == capi.ERR_INVALID
    assert "decreases" in capi.last_error()
    rp2 = np.array([0, 2, 3], dtype=np.int64)
    ci2 = np.array([0, 3, 1], dtype=np.int32)          # column 3 of a 3-column matrix
    bad2 = capi.CsrView(2, 3, rp2.ctypes.data, ci2.ctypes.data, va.ctypes.data, 0, 0)
    assert L.cvr_create(C.byref(h), C.byref(bad2), C.byref(o)) == capi.ERR_INVALID
    assert "outside" in capi.last_error()
    # A's rows become the column indices of A^T: nrows must fit them
    many = capi.CsrView(0x7fffffff, 3, None, None, None, 0, 1)
    assert L.cvr_create(C.byref(h), C.byref(many), C.byref(o)) == capi.ERR_INVALID
    assert "transpose" in capi.last_error()
    assert not h.value
    del rp, ci, rp2, ci2, va


def test_create_multi_refuses_transpose_before_any_device_work():
    L = capi.lib()
    view, keep = _tiny_view()
    o = capi.Options()
    L.cvr_default_options(C.byref(o))
    o.transpose = 1
    m = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    assert L.cvr_create_multi(C.byref(m), C.byref(view), C.byref(o), devs, 1) == capi.ERR_INVALID
    assert not m.value
    assert "transpose" in capi.last_error()
    del keep


def test_without_a_device_the_option_reaches_the_device_check():
    """a valid A with transpose = 1 passes every host check and stops where any create stops without a GPU"""
    if capi.lib().cvr_device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests cover the create")
    L = capi.lib()
    view, keep = _tiny_view()
    o = capi.Options()
    L.cvr_default_options(C.byref(o))
    o.transpose = 1
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), C.byref(o)) == capi.ERR_NO_DEVICE
    del keep


def test_transpose_kernels_every_precision_without_scratch():
    import isa_check
    src = os.path.join(ROOT, "cvr_amd", "csrc", "cvr_transpose.hip")
    path = isa_check.compile_to_asm(src)
    try:
        lines = open(path).read().split("\n")
    finally:
        os.unlink(path)
    md = isa_check.metadata(lines)
    ours = [n for n in md if "transpose_" in n and "_kernel" in n]
    gathers = [n for n in ours if "transpose_gather_kernel" in n]
    assert len(gathers) == 4, gathers          # u32 / u64 bits x values / positions
    assert [n for n in ours if "transpose_rows_kernel" in n] and [n for n in ours if "transpose_iota_kernel" in n]
    for n in ours:          # (the radix sort's own kernels are hipCUB's, as in the column-panel split)
        item = md[n]
        assert item.get("private_segment_fixed_size") == 0, (n, item)
        assert item.get("vgpr_spill_count", 0) == 0 and item.get("sgpr_spill_count", 0) == 0, (n, item)
