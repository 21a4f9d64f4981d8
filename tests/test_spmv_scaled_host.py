"""The scaled product y = alpha A x + beta y (cvr_spmv_scaled_device, cvr_spmv_scaled) -- what can be checked without a GPU: the ABI (exports,
argument checks that come before any device work) and the code of the kernels that take the scaling in their write-out for gfx950 (every
scaled instantiation is there and runs without scratch or spills; the ring kernels keep their instantiations)."""
import ctypes as C
import os
import re
import sys

import pytest

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_library_exports_the_scaled_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in ("cvr_spmv_scaled_device", "cvr_spmv_scaled"):
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


def test_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    assert L.cvr_spmv_scaled_device(None, 1.0, p, 0.0, p, None) == capi.ERR_INVALID
    assert L.cvr_spmv_scaled_device(fake, 1.0, p, 0.0, None, None) == capi.ERR_INVALID
    assert L.cvr_spmv_scaled_device(fake, 2.0, None, 1.0, p, None) == capi.ERR_INVALID          # null x with alpha != 0
    assert L.cvr_spmv_scaled_device(fake, -1e-300, None, 0.0, p, None) == capi.ERR_INVALID
    assert "null" in capi.last_error()
    assert L.cvr_spmv_scaled(None, 1.0, p, 0.0, p) == capi.ERR_INVALID
    assert L.cvr_spmv_scaled(fake, 1.0, p, 0.0, None) == capi.ERR_INVALID
    assert L.cvr_spmv_scaled(fake, 0.5, None, 0.0, p) == capi.ERR_INVALID


@pytest.fixture(scope="module")
def scaled_asm():
    import isa_check
    path = isa_check.compile_to_asm()
    try:
        yield open(path).read().split("\n")
    finally:
        os.unlink(path)


def _demangled(names):
    import subprocess
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def test_scaled_instantiations_without_scratch_or_spills(scaled_asm):
    import isa_check
    md = isa_check.metadata(scaled_asm)
    dem = _demangled(list(md))
    seen = {}
    for name, item in md.items():
        d = dem[name].replace("(anonymous namespace)", "anon").split("(")[0]
        m = re.search(r"::(spmv_kernel|spmv_seg_kernel|combine_kernel|combine_bits_kernel)<(float|double), .*, true>$", d)
        if not m:
            continue
        seen.setdefault((m.group(1), m.group(2)), []).append(d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        # (the bitmap pass of 16 panels in fp64 moves scalar registers into vector lanes in its plain form already: no scratch either way)
        if "combine_bits_kernel<double, 16" not in d:
            assert item.get("sgpr_spill_count", 0) == 0, (d, item)
    for k in ("spmv_kernel", "spmv_seg_kernel", "combine_kernel", "combine_bits_kernel"):
        for t in ("float", "double"):
            assert seen.get((k, t)), f"no scaled instantiation of {k} for {t}"
    # narrow columns, every table of x (none, window, hub table, hub table with a non-temporal stream), several waves: all scaled
    kern = {d for (k, _), ds in seen.items() if k == "spmv_kernel" for d in ds}
    assert len(kern) == 2 * (2 * 4 * 2 + 1), sorted(kern)          # T x (dictionary x WIN x several waves + narrow columns)
    for name, item in md.items():
        if "axpby_kernel" in name:
            assert item.get("private_segment_fixed_size") == 0 and item.get("vgpr_spill_count", 0) == 0


def test_ring_kernels_keep_their_instantiations(scaled_asm):
    """the ring kernels take the scaling as a run-time argument: still 16 instantiations each, all through the register guard"""
    import isa_check
    ks = isa_check.kernels(scaled_asm)
    ilv = [k for k in ks if "spmv_ilv_kernel" in k]
    gang = [k for k in ks if "spmv_gang_kernel" in k]
    assert len(ilv) == 16 and len(gang) == 16
    assert all("ScaleEpi" in k for k in ilv + gang)
