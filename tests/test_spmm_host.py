"""Several vectors at once (cvr_spmm_device, cvr_options.nvec) -- what can be checked without a GPU: the ABI (exports, option struct,
argument checks that come before any device work) and the k-wide kernel's code for gfx950 (every block width and precision is there and
runs without scratch)."""
import ctypes as C
import os
import re
import sys

import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_library_exports_the_spmm_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in ("cvr_spmm_device", "cvr_spmm", "cvr_spmm_supported"):
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


def test_options_keep_their_size_and_default_to_one_vector():
    # nvec took the first of the three reserved words: the struct (and every caller compiled against it) is unchanged
    assert C.sizeof(capi.Options) == 88
    assert capi.Options.nvec.offset == capi.Options.gang.offset + 4
    assert capi.Options.reserved.offset == capi.Options.nvec.offset + 4 and capi.Options.reserved.size == 8
    o = capi.Options()
    C.memset(C.byref(o), 0x5a, C.sizeof(o))
    capi.lib().cvr_default_options(C.byref(o))
    assert o.nvec == 0 and list(o.reserved) == [0, 0]


def test_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    assert L.cvr_spmm_device(None, p, 1, p, 1, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm_device(fake, None, 1, p, 1, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm_device(fake, p, 1, None, 1, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm_device(fake, p, 4, p, 4, 0, None) == capi.ERR_INVALID
    assert L.cvr_spmm_device(fake, p, 3, p, 4, 4, None) == capi.ERR_INVALID
    assert L.cvr_spmm_device(fake, p, 4, p, 3, 4, None) == capi.ERR_INVALID
    assert "nvec" in capi.last_error()
    assert L.cvr_spmm(None, p, p, 2, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm(fake, None, p, 2, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm(fake, p, None, 2, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm(fake, p, p, 0, 1, None) == capi.ERR_INVALID
    assert L.cvr_spmm_supported(None) == 0


@pytest.fixture(scope="module")
def spmv_asm():
    import isa_check
    path = isa_check.compile_to_asm()
    try:
        yield open(path).read().split("\n")
    finally:
        os.unlink(path)


def test_spmm_kernel_every_width_and_precision_without_scratch(spmv_asm):
    import isa_check
    md = isa_check.metadata(spmv_asm)
    seen = {}
    for name, item in md.items():
        m = re.search(r"spmm_kernelI([df])Li(\d+)E", name)
        if not m:
            continue
        seen.setdefault((m.group(1), int(m.group(2))), []).append(name)
        assert item.get("private_segment_fixed_size") == 0, (name, item)
        assert item.get("vgpr_spill_count", 0) == 0 and item.get("sgpr_spill_count", 0) == 0, (name, item)
    for t in "df":
        for kb in (1, 2, 4, 8):
            assert seen.get((t, kb)), f"no spmm_kernel instantiation for {'double' if t == 'd' else 'float'} x {kb}"
    fix = [n for n in md if "spmm_fixup_kernel" in n]
    assert len(fix) == 2 and all(md[n].get("private_segment_fixed_size") == 0 for n in fix)
