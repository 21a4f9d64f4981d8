"""GPU (MI355X): cvr_color_device through the ABI against tests/mcsgs_model.py -- color, perm, color_ptr, ncolors and rounds byte for byte on every
case, from host and from device arrays; the same bytes whatever CVR_DEBUG=color_check is (each value in a fresh child process); the errors of the
host twin from device arrays, with their texts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mcsgs_model as M
from cvr_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, name):
    n, rp, ci, va, color, ncolors, rounds, perm, ptr = M.case(name)
    assert (got[3], got[4]) == (ncolors, rounds), (name, got[3], got[4], ncolors, rounds)
    assert got[0].dtype == np.int32 and got[0].tobytes() == color.tobytes(), (name, "color", int(np.flatnonzero(got[0] != color)[0]))
    assert got[1].tobytes() == perm.tobytes(), (name, "perm")
    assert got[2].tobytes() == ptr.tobytes(), (name, "color_ptr", got[2].tolist(), ptr.tolist())


@pytest.mark.parametrize("name", M.CASES)
def test_every_case_from_host_and_from_device_arrays(name):
    n, rp, ci = M.case(name)[:3]
    _same(capi.color_device(rp, ci), name)
    rt, ct = torch.from_numpy(np.array(rp)).cuda(), torch.from_numpy(np.array(ci)).cuda()
    torch.cuda.synchronize()
    _same(capi.color_device(rt.data_ptr(), ct.data_ptr(), on_device=True, n=n), name)


def test_n_zero_and_a_shifted_first_row_pointer():
    color, perm, ptr, nc, rounds = capi.color_device(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    assert (len(color), len(perm), ptr.tolist(), nc, rounds) == (0, 0, [0], 0, 0)
    n, rp, ci = M.case("laplacian-24")[:3]
    shifted = (rp + 11, np.concatenate([np.full(11, 3, dtype=np.int32), ci]))
    _same(capi.color_device(*shifted), "laplacian-24")
    rt, ct = torch.from_numpy(shifted[0]).cuda(), torch.from_numpy(shifted[1]).cuda()
    torch.cuda.synchronize()
    _same(capi.color_device(rt.data_ptr(), ct.data_ptr(), on_device=True, n=n), "laplacian-24")


_CHILD = """
import hashlib, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import mcsgs_model as M
from cvr_amd import capi
for name in ("laplacian-40", "irr-sym-3000", "clique-70"):
    n, rp, ci = M.matrix(name)[:3]
    color, perm, ptr, nc, rounds = capi.color_device(rp, ci)
    print(name, nc, rounds, hashlib.sha256(color.tobytes() + perm.tobytes() + ptr.tobytes()).hexdigest())
"""


def test_the_check_interval_changes_no_bit_and_no_count():
    """CVR_DEBUG=color_check=1 and =1000, each in a fresh child process: the lines the children print are the model's"""
    import hashlib
    want = []
    for name in ("laplacian-40", "irr-sym-3000", "clique-70"):
        c = M.case(name)
        want.append(f"{name} {c[5]} {c[6]} {hashlib.sha256(c[4].tobytes() + c[7].tobytes() + c[8].tobytes()).hexdigest()}")
    for k in (1, 1000):
        env = dict(os.environ, CVR_DEBUG=f"color_check={k}")
        out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (k, out.stderr[-2000:])
        assert out.stdout.strip().splitlines() == want, (k, out.stdout)


def _call(n, ncols, rp, ci, on_device=True, device=0):
    L = capi.lib()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32)
    color, perm, ptr = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    a, b = C.c_int32(7), C.c_int32(7)
    if on_device:
        rt, ct = torch.from_numpy(np.array(rp)).cuda(), torch.from_numpy(np.array(ci)).cuda()
        torch.cuda.synchronize()
        view = capi.CsrView(n, ncols, rt.data_ptr(), ct.data_ptr(), None, 0, 1)
    else:
        view = capi.CsrView(n, ncols, rp.ctypes.data, ci.ctypes.data, None, 0, 0)
    rc = L.cvr_color_device(C.byref(view), device, None, color.ctypes.data, perm.ctypes.data, ptr.ctypes.data, C.byref(a), C.byref(b))
    assert rc == 0 or (a.value, b.value) == (0, 0)
    return rc, capi.last_error()


@pytest.mark.parametrize("on_device", [True, False])
def test_every_error_and_its_text(on_device):
    rc, msg = _call(3, 4, [0, 1, 2, 3], [0, 1, 2], on_device)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: the colouring needs a square matrix (3 x 4)"
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 1, 3], on_device)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: row 2: the columns are not strictly increasing (1 behind 2)"
    rc, msg = _call(4, 4, [0, 1, 3, 5, 6], [0, 0, 1, 2, 2, 3], on_device)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: row 2: the columns are not strictly increasing (2 behind 2)"
    rc, msg = _call(4, 4, [0, 1, 2, 4, 5], [0, 1, 1, 3, 3], on_device)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: row 2 has no diagonal entry"
    rc, msg = _call(3, 3, [0, 1, 1, 2], [0, 2], on_device)
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: row 1 has no diagonal entry"
    rc, msg = _call(2, 2, [0, 1, 2], [0, 5], on_device)          # cvr_create's check: a column outside the matrix
    assert rc == capi.ERR_INVALID
    rc, msg = _call(2, 2, [0, 1, 2], [0, 1], on_device, device=capi.lib().cvr_device_count())
    assert rc == capi.ERR_NO_DEVICE
    # asymmetric: rows 1 and 3 both have entries without an answer; the lowest row and its lowest such column are named
    rc, msg = _call(5, 5, [0, 1, 4, 5, 7, 8], [0, 1, 2, 3, 2, 3, 4, 4], on_device)
    assert rc == capi.ERR_INVALID
    assert msg == "cvr_color_device: row 1 has an entry in column 2, row 2 none in column 1: the off-diagonal pattern must be structurally symmetric"
    rc, msg = _call(3, 3, [0, 2, 3, 4], [0, 2, 1, 1], on_device)          # the structure rules come first
    assert rc == capi.ERR_INVALID and msg == "cvr_color_device: row 2 has no diagonal entry"
    # a large case with one answer removed far from the start: row 40000's entry in column 39999 (row 39999 still has its own in column 40000)
    n, rp, ci = M.case("ties-62291")[:3]
    q = int(rp[40000]) + int(np.flatnonzero(ci[rp[40000]: rp[40001]] == 39999)[0])
    rp2 = rp.copy()
    rp2[40001:] -= 1
    rc, msg = _call(n, n, rp2, np.delete(ci, q), on_device)
    assert rc == capi.ERR_INVALID and "row 39999 has an entry in column 40000, row 40000 none in column 39999" in msg, msg


def test_null_arguments():
    L = capi.lib()
    rp, ci = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    color, perm, ptr = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)
    a, b = C.c_int32(), C.c_int32()
    view = capi.CsrView(2, 2, rp.ctypes.data, ci.ctypes.data, None, 0, 0)
    args = [C.byref(view), 0, None, color.ctypes.data, perm.ctypes.data, ptr.ctypes.data, C.byref(a), C.byref(b)]
    for k in (0, 3, 4, 5, 6, 7):
        bad = list(args)
        bad[k] = None
        assert L.cvr_color_device(*bad) == capi.ERR_INVALID and capi.last_error() == "null argument", k
    assert L.cvr_color_device(*args) == 0 and (a.value, b.value, color.tolist(), ptr.tolist()[:2]) == (1, 1, [0, 0], [0, 2])
