"""The block-Jacobi object with several right-hand sides (cvr_precond_apply_multi_device, cvr_pcg_multi_device, cvr_pcg_multi) -- what can be checked
without a GPU: the ABI (exports, the argument checks in their order, before any device work and before the handle or the object is looked at), the code
of cvr_pcg_multi.hip for gfx950 (every instantiation is there and runs without scratch or spills inside a streaming pass's budget; metadata only), and
the numpy model of the k-wide apply and of the batched solver (pcg_multi_model.py) against the single models, with two mutants it must catch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import krylov_model as KM
import pcg_multi_model as MM
import precond_model as PM
from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("cvr_precond_apply_multi_device", "cvr_pcg_multi_device", "cvr_pcg_multi")


def test_library_exports_the_entry_points():
    L = C.CDLL(capi.lib_path())
    hdr = open(os.path.join(ROOT, "include", "cvr_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert callable(capi.Precond.apply_multi) and callable(capi.CvrMatrix.pcg_multi) and callable(capi.CvrMatrix.pcg_multi_host)


def _options(**kw):
    o = capi.CgOptions()
    capi.lib().cvr_cg_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_apply_argument_checks_come_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 256)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first do not look at the object)
    assert L.cvr_precond_apply_multi_device(None, p, 2, q, 2, 2, None) == capi.ERR_INVALID
    assert L.cvr_precond_apply_multi_device(fake, None, 2, q, 2, 2, None) == capi.ERR_INVALID
    assert L.cvr_precond_apply_multi_device(fake, p, 2, None, 2, 2, None) == capi.ERR_INVALID
    assert "null" in capi.last_error()
    assert L.cvr_precond_apply_multi_device(fake, p, 2, p, 2, 2, None) == capi.ERR_INVALID
    assert "same block" in capi.last_error()
    assert L.cvr_precond_apply_multi_device(fake, p, 2, p, 2, 9, None) == capi.ERR_INVALID          # R == Z comes before nvec
    assert "same block" in capi.last_error()
    for nvec in (0, -1, 9, 16):
        assert L.cvr_precond_apply_multi_device(fake, p, 16, q, 16, nvec, None) == capi.ERR_INVALID, nvec
        assert "nvec" in capi.last_error()
    for nvec, ldr, ldz in ((2, 1, 2), (2, 2, 1), (8, 7, 8), (8, 8, 0), (3, -3, 3)):
        assert L.cvr_precond_apply_multi_device(fake, p, ldr, q, ldz, nvec, None) == capi.ERR_INVALID, (nvec, ldr, ldz)
        assert "ldr" in capi.last_error() and "ldz" in capi.last_error()


def test_solver_argument_checks_come_in_order_before_any_device_work():
    L = capi.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(C.addressof(buf))          # (never dereferenced: the checks that fail first look neither at the handle nor at the object)
    ok, res = _options(), (capi.CgResult * 8)()

    def device(h, pc, b, x, o, r, nvec=2, ldb=2, ldx=2):
        return L.cvr_pcg_multi_device(h, pc, b, ldb, x, ldx, nvec, o, r, None)

    def host(h, pc, b, x, o, r, nvec=2, ldb=None, ldx=None):
        return L.cvr_pcg_multi(h, pc, b, x, nvec, o, r)
    for call in (device, host):
        # 1. cvr_cg_device's argument checks
        assert call(None, fake, p, p, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, fake, None, p, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, fake, p, None, C.byref(ok), res) == capi.ERR_INVALID
        assert call(fake, fake, p, p, None, res) == capi.ERR_INVALID
        assert call(fake, fake, p, p, C.byref(ok), None) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        for bad in (dict(rtol=-1.0), dict(rtol=float("nan")), dict(rtol=float("inf")), dict(max_iters=-1), dict(check_every=-1)):
            assert call(fake, fake, p, p, C.byref(_options(**bad)), res) == capi.ERR_INVALID, bad
        for i in range(4):
            o = _options()
            o.reserved[i] = 1
            assert call(fake, fake, p, p, C.byref(o), res) == capi.ERR_INVALID
            assert "reserved" in capi.last_error()
        # 2. the object
        assert call(fake, None, p, p, C.byref(ok), res) == capi.ERR_INVALID
        assert "null" in capi.last_error()
        assert call(fake, fake, p, p, C.byref(_options(minv_dev=p.value)), res) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error() and "cvr_pcg_multi" in capi.last_error()
        # 3. the block
        for nvec in (0, -1, 9, 16):
            assert call(fake, fake, p, p, C.byref(ok), res, nvec=nvec, ldb=16, ldx=16) == capi.ERR_INVALID, nvec
            assert "nvec" in capi.last_error()
        # the order: a bad option beside a null object is the option's error; minv_dev beside a bad nvec is minv_dev's
        o = _options()
        o.reserved[0] = 1
        assert call(fake, None, p, p, C.byref(o), res) == capi.ERR_INVALID
        assert "reserved" in capi.last_error()
        assert call(fake, fake, p, p, C.byref(_options(minv_dev=p.value)), res, nvec=9, ldb=16, ldx=16) == capi.ERR_INVALID
        assert "minv_dev" in capi.last_error()
        assert call(fake, None, p, p, C.byref(ok), res, nvec=9, ldb=16, ldx=16) == capi.ERR_INVALID
        assert "null" in capi.last_error()
    for nvec, ldb, ldx in ((2, 1, 2), (2, 2, 1), (8, 7, 8), (8, 8, 0), (3, -3, 3)):          # (the host twin has no leading dimension: ld = nvec)
        assert device(fake, fake, p, p, C.byref(ok), res, nvec=nvec, ldb=ldb, ldx=ldx) == capi.ERR_INVALID, (nvec, ldb, ldx)
        assert "ldb" in capi.last_error() and "ldx" in capi.last_error()


# ---- the code for gfx950 ----
@pytest.fixture(scope="module")
def md():
    import isa_check
    path = isa_check.compile_to_asm(os.path.join(ROOT, "cvr_amd", "csrc", "cvr_pcg_multi.hip"))
    try:
        yield isa_check.metadata(open(path).read().split("\n"))
    finally:
        os.unlink(path)


def test_kernels_without_scratch_or_spills(md):
    names = list(md)
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    seen = {}
    for name, item in md.items():
        d = dem[name]
        m = re.search(r"((?:precond_apply_multi|pcgm_\w+|cgm_\w+)_kernel)", d)
        assert m, d
        seen.setdefault(m.group(1), []).append(d)
        print(item.get("vgpr_count"), item.get("group_segment_fixed_size"), d)
        assert item.get("private_segment_fixed_size") == 0, (d, item)
        assert item.get("vgpr_spill_count", 0) == 0, (d, item)
        assert item.get("sgpr_spill_count", 0) == 0, (d, item)
        assert item.get("vgpr_count", 999) <= 128, (d, item)          # streaming passes live on occupancy
        assert "group_segment_fixed_size" in item and item["group_segment_fixed_size"] <= 20 * 1024, (d, item)
    # T x 16-byte sub-blocks of R x of Z for the plain apply; T x (start, step) x 16-byte packets in the library's blocks for the solver's -- and no
    # cgm_* kernel: the solver that enqueues pcgm_apply_kernel is cvr_cg_multi.hip's, whose kernels test_cg_multi_host.py pins (the forms it launches
    # with an object, PRE = false in the start and the update, r.z present in the direction, among them)
    assert {k: len(v) for k, v in seen.items()} == dict(precond_apply_multi_kernel=8, pcgm_apply_kernel=8), seen
    for k, v in seen.items():
        assert any("<float" in d for d in v) and any("<double" in d for d in v), k


# ---- the model ----
def _system(n, bs, dtype):
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    return PM.host_product(n, rp, ci, va, dtype), PM.inverse_blocks(rp, ci, va, bs, dtype)


def _columns(n, dtype, seed):
    """a block whose columns stop at different steps: ordinary ones from a zero and a random start, b = 0 from a random start, a NaN in b"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, 5))
    X0 = np.zeros((n, 5))
    X0[:, 1] = rng.random(n) * 2 - 1
    B[:, 2] = 0
    X0[:, 2] = rng.random(n) * 2 - 1
    B[n // 2, 3] = np.nan
    X0[:, 3] = X0[:, 1]
    return B.astype(dtype), X0.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,bs", [(n, bs) for n in (1, 5, 250) for bs in (1, 3, 32)])
def test_model_equals_the_single_models_column_for_column(n, bs, dtype):
    product, W = _system(n, bs, dtype)
    B, X0 = _columns(n, dtype, seed=n * 100 + bs)
    R = B.copy()
    R[0, 0] = -0.0
    Z = MM.apply_multi(W, R, bs, dtype)
    for c in range(R.shape[1]):
        assert Z[:, c].tobytes() == PM.apply(W, R[:, c], bs, dtype).tobytes(), (n, bs, c)
    rtol = 1e-10 if dtype == np.float64 else 1e-4
    for max_iters in (0, 2, 40):
        model = MM.PcgMulti(product, dtype, W, bs)
        got = model.run(B, X0, rtol=rtol, max_iters=max_iters)
        for c, g in enumerate(got):
            tr = PM.Pcg(product, dtype, W, bs).run(B[:, c], X0[:, c], rtol=rtol, max_iters=max_iters)
            msg = KM.compare(g, tr.at(max_iters))
            assert msg == "", (n, bs, max_iters, c, msg)
        assert MM.writes_after_stop(model) == []
        if max_iters == 40:
            assert [g.status for g in got] == [KM.CONVERGED, KM.CONVERGED, KM.CONVERGED, KM.BREAKDOWN, KM.CONVERGED], [g.status for g in got]
            assert got[3].iterations == 0 and got[3].x.tobytes() == X0[:, 3].tobytes() and not got[2].x.any()


def test_model_catches_a_sum_started_from_plus_zero():
    """s = +0 + t_0 gives +0 where the header's s = t_0 gives -0"""
    n, bs, dtype = 5, 1, np.float64
    _, W = _system(n, bs, dtype)
    assert (W > 0).all()
    R = np.ones((n, 3))
    R[2, 1] = -0.0

    def from_zero(terms):
        return np.zeros(terms.shape[:-1]) + PM.left_to_right(terms)
    good, bad = MM.apply_multi(W, R, bs, dtype), MM.apply_multi(W, R, bs, dtype, zsum=from_zero)
    assert np.signbit(good[2, 1]) and good[2, 1] == 0
    assert np.array_equal(good, bad) and good.tobytes() != bad.tobytes()          # (equal as numbers: only the bits tell)
    for c in range(3):
        assert good[:, c].tobytes() == PM.apply(W, R[:, c], bs, dtype).tobytes()
    assert bad[:, 1].tobytes() != PM.apply(W, R[:, 1], bs, dtype).tobytes()


def test_model_catches_a_stopped_column_whose_z_is_still_written():
    n, bs, dtype = 250, 3, np.float64
    product, W = _system(n, bs, dtype)
    B, X0 = _columns(n, dtype, seed=7)

    class Mutant(MM.PcgMulti):
        def apply_columns(self, live, nvec):
            return list(range(nvec))
    good, bad = MM.PcgMulti(product, dtype, W, bs), Mutant(product, dtype, W, bs)
    a, b = good.run(B, X0, rtol=1e-10, max_iters=40), bad.run(B, X0, rtol=1e-10, max_iters=40)
    for g, h in zip(a, b):          # the values cannot tell: a stopped column's r no longer changes
        assert KM.compare(g, h) == ""
    assert MM.writes_after_stop(good) == []
    late = MM.writes_after_stop(bad)
    assert late and {blk for _, blk, _ in late} == {"z"}
    assert {c for _, _, c in late} >= {2, 3}          # b = 0 (stopped at the start) and the NaN (stopped by the update of step 0)
    assert (0, "z", 3) in late
