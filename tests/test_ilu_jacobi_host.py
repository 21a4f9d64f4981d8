"""CPU: what cvr_precond_ilu0_jacobi and cvr_precond_ilu0_jacobi_info do without a device -- the symbols, the header, the struct, and every
argument they decline before any device work."""
import ctypes as C
import os
import re

import numpy as np

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_ilu0_jacobi", "cvr_precond_ilu0_jacobi_info"]


def test_symbols_header_and_struct():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert re.search(r"#define CVR_ILU0_MAX_SWEEPS\s+64\b", hdr) and capi.ILU0_MAX_SWEEPS == 64
    assert re.search(r"\}\s*cvr_ilu0_jacobi_info;", hdr)
    assert C.sizeof(capi.Ilu0JacobiInfo) == 72          # two int64, six int32, eight reserved
    assert [f[0] for f in capi.Ilu0JacobiInfo._fields_] == ["n", "nnz", "sweeps", "launches_per_apply", "lanes_per_row", "levels_lower", "levels_upper", "is_f32", "reserved"]
    for name in ("ilu0_jacobi", "ilu0_jacobi_from_device", "ilu0_jacobi_info"):
        assert hasattr(capi.Precond, name), name


def test_null_arguments_and_sweeps_out_of_range_need_no_device():
    L = capi.lib()
    rp, ci, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    p = C.c_void_p()
    assert L.cvr_precond_ilu0_jacobi(None, C.byref(view), 3, 0, None) == capi.ERR_INVALID
    assert L.cvr_precond_ilu0_jacobi(C.byref(p), None, 3, 0, None) == capi.ERR_INVALID
    for sweeps in (0, -1, 65):
        p = C.c_void_p(1)
        assert L.cvr_precond_ilu0_jacobi(C.byref(p), C.byref(view), sweeps, 0, None) == capi.ERR_INVALID, sweeps
        assert "sweeps" in capi.last_error() and not p.value, (sweeps, capi.last_error())
    assert L.cvr_precond_ilu0_jacobi_info(None, C.byref(capi.Ilu0JacobiInfo())) == capi.ERR_INVALID
    assert L.cvr_precond_ilu0_jacobi_info(None, None) == capi.ERR_INVALID
