"""Conjugate gradients on the device (cvr_cg_device, cvr_cg) -- what can be checked without a GPU: the ABI (exports, the argument checks
that come before any device work and before the handle is looked at, the default options), the code of the solver's vector kernels for
gfx950 (every fp32 / fp64 instantiation is there and runs without scratch or spills) and the SpMV kernels' instantiation counts, which
the solver leaves alone (it adds no template parameter to an existing kernel), and the generator of its test matrices."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cvr_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_cg_default_options", "cvr_cg_device", "cvr_cg")


def test_library_exports_the_solver_entry_points():
    L = C.CDLL(capi.lib_path())
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options():
    o = capi.CgOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    capi.lib().cvr_cg_default_options(C.byref(o))
    assert o.max_iters >= 0 and o.check_every >= 0
    assert math.isfinite(o.rtol) and o.rtol >= 0
    assert not o.minv_dev
    assert list(o.reserved) == [0, 0, 0, 0]
    capi.lib().cvr_cg_default_options(None)          # (a null pointer is ignored)


def test_struct_sizes_match_the_header(tmp_path):
    """the ctypes structs against the C compiler's layout of include/cvr_amd.h"""
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cvr_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(cvr_cg_options), '
                   'offsetof(cvr_cg_options, rtol), offsetof(cvr_cg_options, reserved), sizeof(cvr_cg_result), offsetof(cvr_cg_result, residual_norm), '
                   'offsetof(cvr_cg_result, seconds)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, R = capi.CgOptions, capi.CgResult
    assert got == [C.sizeof(O), O.rtol.offset, O.reserved.offset, C.sizeof(R), R.residual_norm.offset, R.seconds.offset]


def test_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the handle)
    ok, res = _options(), capi.CgResult()
    for call in (lambda h, b, x, o, r: L.cvr_cg_device(h, b, x, o, r, None), L.cvr_cg):
        assert call(None, p, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, None, p, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, None, C.byref(ok), C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, None, C.byref(res)) == capi.ERR_INVALID
        assert call(fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, p, p, C.byref(_options(**bad)), C.byref(res)) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, p, p, C.byref(o), C.byref(res)) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()


def test_spd_from_pattern_is_symmetric_with_its_spectrum_in_bounds():
    """A = I + c D^-1/2 W D^-1/2: symmetric bit for bit, unit diagonal, and x.Ax / x.x inside [0.5, 1.5] (Gershgorin bounds the
    normalised adjacency's spectrum by 1 after the similarity D^1/2 . D^-1/2); S A S has the diagonal s^2"""
    n, _, rp, ci, _ = synth.rmat(9, dedupe=True)
    for dtype in (np.float64, np.float32):
        n2, nc, rp2, ci2, va = synth.spd_from_pattern(n, rp, ci, dtype=dtype)
        assert (n2, nc) == (n, n) and va.dtype == dtype and rp2[-1] == len(ci2) == len(va)
        A = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(rp2))
        assert len(set(zip(rows.tolist(), ci2.tolist()))) == len(ci2), "duplicates"
        for r in range(n):
            assert np.all(np.diff(ci2[rp2[r]:rp2[r + 1]]) > 0), "columns of a row sorted"
        A[rows, ci2] = va
        assert np.array_equal(A, A.T)
        assert np.array_equal(np.diag(A), np.ones(n))
        ev = np.linalg.eigvalsh(A)
        assert ev[0] >= 0.5 - 1e-6 and ev[-1] <= 1.5 + 1e-6, (ev[0], ev[-1])
    s = 10.0 ** (2 * np.random.default_rng(1).random(n))
    _, _, rp3, ci3, vs = synth.spd_from_pattern(n, rp, ci, dscale=s)
    assert np.array_equal(rp3, rp2) and np.array_equal(ci3, ci2)
    B = np.zeros((n, n))
    B[rows, ci3] = vs
    assert np.array_equal(B, B.T)
    assert np.allclose(np.diag(B), s * s, rtol=1e-15)


@pytest.fixture(scope="module")
def cg_md():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_cg.hip"))
    try:
        yield isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def _demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def test_solver_kernels_without_scratch_or_spills(cg_md):
    dem = _demangled(list(cg_md))
    seen = {}
    for name, item in cg_md.items():
        d = dem[name]
        m = re.search(r"(cg_\w+_kernel)(?:<(float|double)[^>]*>)?", dem[name])
        assert m, dem[name]
        seen.setdefault(m.group(1), []).append(dem[name])
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
    # T x preconditioner x alignment of the caller's arrays for the passes that touch them; T (x preconditioner) for the others
    assert {k: len(v) for k, v in seen.items()} == dict(cg_init_kernel=8, cg_check_kernel=1, cg_pq_kernel=2, cg_update_kernel=8, cg_direction_kernel=4), seen
    for k, v in seen.items():
        if k != "cg_check_kernel":
            assert any("<float" in d for d in v) and any("<double" in d for d in v), k


def test_spmv_kernel_instantiations_unchanged():
    """the solver goes through run_spmv as it is: 16 + 16 ring kernels, 2 * (2*4*2 + 1) scaled spmv_kernels, as test_spmv_scaled_host pins them"""
    import isa_check
    path = isa_check.compile_to_asm()
    try:
        lines = open(path).read().split("\n")
    finally:
        os.unlink(path)
    ks = isa_check.kernels(lines)
    assert len([k for k in ks if "spmv_ilv_kernel" in k]) == 16
    assert len([k for k in ks if "spmv_gang_kernel" in k]) == 16
    md = isa_check.metadata(lines)
    dem = _demangled(list(md))
    scaled = {dem[n].replace("(anonymous namespace)", "anon").split("(")[0] for n in md}
    scaled = {d for d in scaled if re.search(r"::spmv_kernel<(float|double), .*, true>$", d)}
    assert len(scaled) == 2 * (2 * 4 * 2 + 1), sorted(scaled)
