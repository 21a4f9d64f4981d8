"""CPU: cvr_precond_amg_block and cvr_precond_amg_block_info through the ABI without a device -- the names, the struct, and the constructor's argument
errors in the header's order: the nulls, setup, nvec, then what the constructor named by `setup` checks (the options, omega for the smoothed set-ups,
the view), all before the handle is looked at and before any device work."""
import ctypes as C
import os
import re

import numpy as np

from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvr_precond_amg_block", "cvr_precond_amg_block_info"]
BAD_OPTIONS = [("max_levels", 0), ("max_levels", 17), ("coarse_size", 0), ("coarse_size", 257), ("sweeps", 0), ("sweeps", 5), ("reserved0", 1), ("strength", -0.1),
               ("strength", 1.0), ("strength", np.nan), ("coarse_scale", 0.0), ("coarse_scale", -1.0), ("coarse_scale", np.inf), ("coarse_scale", np.nan)]
BAD_OMEGAS = [np.nan, -0.5, 2.0, np.inf, -np.inf, 2.5]


def test_symbols_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint " + s + r"\(", hdr), s
    assert hasattr(capi, "AmgBlockInfo") and C.sizeof(capi.AmgBlockInfo) == 48          # two int32, an int64, eight reserved
    assert [f[0] for f in capi.AmgBlockInfo._fields_] == ["nvec", "setup", "buffer_bytes", "reserved"]
    assert [getattr(capi.AmgBlockInfo, f).offset for f in ("nvec", "setup", "buffer_bytes", "reserved")] == [0, 4, 8, 16]
    for name, v in (("PLAIN", 0), ("SMOOTHED", 1), ("MIS2", 2)):
        assert re.search(r"#define CVR_AMG_SETUP_" + name + r"\s+" + str(v) + r"\b", hdr) and getattr(capi, "AMG_SETUP_" + name) == v
    assert capi.AMG_SETUPS == {"plain": 0, "smoothed": 1, "mis2": 2}
    assert C.sizeof(capi.AmgOptions) == 64 and C.sizeof(capi.AmgInfo) == 336 and C.sizeof(capi.AmgSmoothedInfo) == 176 and C.sizeof(capi.AmgMis2Info) == 104          # as they were
    for m in ("amg_block", "amg_block_from_device", "amg_block_info"):
        assert callable(getattr(capi.Precond, m))


def _view(n=2, ncols=2):
    rp, ci, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    return capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0), (rp, ci, va)


def _bad(p, h, view, opt, setup, omega, nvec):
    rc = capi.lib().cvr_precond_amg_block(p, h, view, opt, setup, omega, nvec, None)
    assert rc == capi.ERR_INVALID, (rc, capi.last_error())
    return capi.last_error()


def test_the_constructors_argument_errors_in_their_order_before_any_device_work():
    view, keep = _view()
    rect, keep2 = _view(2, 3)
    p, fake = C.c_void_p(7), C.c_void_p(1)          # (a handle that is never looked at)
    v, r = C.byref(view), C.byref(rect)
    bad_opt, bad_nan = C.byref(capi.amg_options(reserved0=1)), float("nan")
    # the nulls come first, whatever else is wrong
    _bad(None, fake, v, None, 7, bad_nan, 0)
    _bad(C.byref(p), None, v, None, 7, bad_nan, 0)
    _bad(C.byref(p), fake, None, None, 7, bad_nan, 0)
    assert p.value == 7          # (out is cleared only behind the null checks)
    # ... then setup, before nvec, the options, omega and the view
    for setup in (-1, 3):
        p = C.c_void_p(7)
        msg = _bad(C.byref(p), fake, r, bad_opt, setup, bad_nan, 0)
        assert msg.startswith("cvr_precond_amg_block:") and "setup" in msg and "nvec" not in msg, msg
        assert not p.value
    # ... then nvec, before the options, omega and the view
    for setup in (0, 1, 2):
        for nvec in (0, 9, -1):
            msg = _bad(C.byref(p), fake, r, bad_opt, setup, bad_nan, nvec)
            assert msg.startswith("cvr_precond_amg_block:") and f"nvec = {nvec}" in msg and "reserved0" not in msg, msg
    # ... then the named constructor's checks in its order: the options, omega (the smoothed set-ups only), the view's shape
    for setup in (0, 1, 2):
        for field, val in BAD_OPTIONS:
            msg = _bad(C.byref(p), fake, r, C.byref(capi.amg_options(**{field: val})), setup, bad_nan, 4)
            assert msg.startswith("cvr_precond_amg_block:") and field in msg and "omega" not in msg, (setup, field, msg)
        o = capi.amg_options()
        o.reserved[7] = -1
        assert "reserved[7]" in _bad(C.byref(p), fake, v, C.byref(o), setup, 0.0, 1)
    for setup in (1, 2):
        for omega in BAD_OMEGAS:
            msg = _bad(C.byref(p), fake, r, None, setup, omega, 8)
            assert msg.startswith("cvr_precond_amg_block:") and "omega" in msg, (setup, omega, msg)
    for omega in BAD_OMEGAS + [0.0]:          # the plain set-up ignores omega: the next check answers
        assert "square" in _bad(C.byref(p), fake, r, None, 0, omega, 8)
    for setup in (1, 2):
        assert "square" in _bad(C.byref(p), fake, r, None, setup, 0.0, 1)
        assert "square" in _bad(C.byref(p), fake, r, None, setup, 1.0, 8)
    neg = capi.CsrView(-1, -1, None, None, None, 0, 0)
    assert "negative" in _bad(C.byref(p), fake, C.byref(neg), None, 0, 0.0, 2)
    del keep, keep2


def test_the_info_call_without_an_object():
    L = capi.lib()
    info = capi.AmgBlockInfo()
    assert L.cvr_precond_amg_block_info(None, C.byref(info)) == capi.ERR_INVALID
    assert L.cvr_precond_amg_block_info(None, None) == capi.ERR_INVALID
