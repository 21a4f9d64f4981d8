"""GPU (MI355X): cvr_power_iteration step by step against the numpy model of include/cvr_amd.h (tests/power_model.py; tests/test_power_model_host.py
shows on the CPU that the comparison used here rejects a wrong norm, parity, sum or shard lookup, and that the fused and the dense tree differ on every
matrix of the fused cases).

The model's product is the handle's own cvr_spmv_device; everything else -- the start, the lagged norm, the sums in their trees, the exact last step,
the fp32 range rule, lambda -- is the model's own arithmetic.  Every case checks x byte for byte, lambda bit for bit, x_dev[ncols] == 0 and the values
between ncols + 1 and info.x_elems unchanged (`Dev.power`).  No tolerance anywhere: the device's 1 / sqrt(s) is compared with numpy's
`1.0 / np.sqrt(s)` through x itself (0 ulp on every input of this file as measured; a difference would show as a failure, not be absorbed).

The fused tree is obtained from the exported descriptors: desc[k][0] is the first row of chunk k, and with no row cut over chunks (info.nshared == 0,
asserted) desc[k][2] and desc[k][3] are the chunk's first and last row themselves (asserted), so the chunks' row ranges are known without reading the
kernel; info.waves_per_block is the chunks per workgroup.  They are asserted equal to the chunks of the CPU mirror's planner for the same matrix
(power_model.mirror_chunks), with which tests/test_power_model_host.py shows the fused and the dense model to differ on every matrix and start
vector used here for a fused claim (power_model.fused_claims): matching the fused model says that the one-launch step ran.

The sharded form runs through cvr_power_step_selfcheck (the loop's own launch_power_step, launch_power_sums and launch_unpad on the caller's
arrays): RCCL refuses two ranks on one device, so more than one shard never meets cvr_power_iteration on one GPU.  For the same reason the loop's
own refusal of 65 shards cannot be reached here (it would take a communicator of 65 ranks); both entries validate the shards with one function
(cvr_comm.hip: iter_shards), and it is that function which is tested, through the self-check."""
import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import power_model as PM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

G = KM.GRID
SENTINEL = 3.25
PRECS = ["fp64", "fp32"]


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


class Dev:
    """a handle with the buffers of the model's product, and cvr_power_iteration in the model's terms"""

    def __init__(self, H):
        self.H, self.n = H, H.nrows
        self.tdt = torch.float64 if H.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(H.info.x_elems, self.n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, self.n, 1), dtype=self.tdt, device="cuda")

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def power(self, x0, iters, shift=0, stream=None):
        """(x, lambda) of cvr_power_iteration from x0; the pad element and the tail of the x buffer are checked here"""
        n, ne = self.n, max(self.H.info.x_elems, self.n + 1)
        host = np.full(ne, SENTINEL, dtype=self.H.dtype)
        host[:n], host[n] = x0, 0
        xt = torch.empty(ne + shift, dtype=self.tdt, device="cuda")[shift:]
        xt.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        if stream is None:
            lam, _ = self.H.power_iteration(xt.data_ptr(), iters)
        else:
            with torch.cuda.stream(stream):
                lam, _ = self.H.power_iteration(xt.data_ptr(), iters, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        got = xt.cpu().numpy()
        assert got[n] == 0 and not np.signbit(got[n]), ("x_dev[ncols]", got[n])
        assert got[n + 1:].tobytes() == host[n + 1:].tobytes(), "the values beyond ncols changed"
        return got[:n].copy(), lam


def _check(dev, model, x0, ks, ctx, **kw):
    want = model.sweep(x0, max(ks), ks)
    for k, w in zip(ks, want):
        x, lam = dev.power(x0, k, **kw)
        msg = PM.compare(x, lam, w)
        assert msg == "", (ctx, "iters", k, msg)
        assert np.isfinite(x).all() and np.isfinite(lam), (ctx, "iters", k)
    return want


def _chunks(H):
    """the first row of every chunk and the chunks per workgroup of a handle that takes the one-launch step, from its exported descriptors"""
    i = H.info
    assert i.col_phases > 1 and i.nshared == 0 and i.hub_entries == 0 and i.col_panels == 1 and not i.interleave, (i.col_phases, i.nshared)
    d = H.export_image()["desc"].astype(np.int64)
    first = d[:, 0]
    nxt = np.append(first[1:], H.nrows)
    assert first[0] == 0 and (nxt > first).all() and np.array_equal(d[:, 2], first) and np.array_equal(d[:, 3], nxt - 1)
    return first, max(1, i.waves_per_block)


def _fused_model(dev, dtype, opt, mat, expect_fused=True):
    """the fused model of a handle whose exported chunks are those of the CPU mirror's planner for `mat` (n, n, row_ptr, col_idx, vals)"""
    first, wpb = _chunks(dev.H)
    mfirst, mwpb = PM.mirror_chunks(opt, mat[0], *mat[2:])
    assert np.array_equal(first, mfirst) and wpb == mwpb == opt["waves_per_block"] and dev.H.info.steps_per_chunk == opt["steps_per_chunk"]
    m = PM.PowerModel(dev.product, dtype, sums="fused", chunks=first, wpb=wpb)
    assert (m.sums == "fused") == expect_fused
    return m, first, wpb


# ---- the unfused loop ----
SMALL = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]
UNFUSED = ["plain", "narrow", "hub", "panels", "interleaved", "gang"]


def _unfused_one(H, dtype, ctx, full=True):
    dev = Dev(H)
    model = PM.PowerModel(dev.product, dtype)
    starts = PM.start_vectors(dev.n, dtype)
    _check(dev, model, starts[0][1], list(range(7)) if full else [0, 1, 2, 3], (ctx, "random"))
    for name, x0 in starts[1:]:
        got = _check(dev, model, x0, list(range(7)), (ctx, name))
        if name == "zero":
            assert all(r.lam == 0 and not r.x.any() for r in got)
    return dev, model, starts[0][1]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", UNFUSED)
def test_unfused_loop_against_the_model(layout, prec):
    """every layout takes every size (a creation that fails is an error here).  The power-law matrix, from n = 63 on, has about 25 % empty rows and,
    built with split_threshold = 16, rows cut over chunks at n = 1025 and 4097 on every layout (info.nshared > 0, asserted)"""
    dtype = _dtype(prec)
    for n in SMALL:
        mats = [("banded", KM.banded("nonsym", n, dtype), {})]
        if n >= 63:
            mats.append(("power_law", PM.power_law(n, dtype), dict(split_threshold=16)))
        for mname, (_, _, rp, ci, va), extra in mats:
            H = cvr_amd.CvrMatrix(n, n, rp, ci, va, **dict(K.LAYOUTS[layout], **extra))
            try:
                if mname == "power_law":
                    assert (np.diff(rp) == 0).mean() > 0.2
                    if n >= 1025:
                        assert H.info.nshared > 0, (layout, n)
                dev, model, x0 = _unfused_one(H, dtype, (layout, prec, mname, n))
                if n == 257:          # the x tensor off the 16-byte grid by one value, and a stream of the caller's
                    _check(dev, model, x0, [2, 5], (layout, prec, mname, n, "shifted"), shift=1)
                    _check(dev, model, x0, [2, 5], (layout, prec, mname, n, "stream"), stream=torch.cuda.Stream())
            finally:
                H.close()


@pytest.mark.parametrize("prec,n", [(p, n) for p in PRECS for n in (G - 1, G, G + 1, 2 * G + 1)])
def test_unfused_loop_around_one_trip_of_the_grid(prec, n):
    """every thread with one value but the last; every thread with one; a second trip for thread 0 alone; a third"""
    dtype = _dtype(prec)
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    H = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.LAYOUTS["plain"])
    try:
        dev = Dev(H)
        _check(dev, PM.PowerModel(dev.product, dtype), PM.start_vectors(n, dtype)[0][1], list(range(7)), ("plain", prec, n))
    finally:
        H.close()


@pytest.mark.parametrize("prec", PRECS)
def test_phases_layout_with_the_step_as_a_pass_of_its_own(prec, monkeypatch):
    dtype = _dtype(prec)
    assert K.LAYOUTS["phases"] == PM.PHASES
    for n in (1025, 4097):
        opt, mat, x0, iters = PM.fused_claim(f"banded/{n}", dtype)
        H = cvr_amd.CvrMatrix(n, n, *mat[2:], **opt)
        try:
            dev = Dev(H)
            fused, _, _ = _fused_model(dev, dtype, opt, mat)
            monkeypatch.setenv("CVR_DEBUG", "iter_unfused")
            _check(dev, PM.PowerModel(dev.product, dtype), x0, iters, ("phases", "iter_unfused", prec, n))
            monkeypatch.delenv("CVR_DEBUG")
            _check(dev, fused, x0, iters, ("phases", "fused", prec, n))
        finally:
            monkeypatch.delenv("CVR_DEBUG", raising=False)
            H.close()


# ---- the fused loop ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(PM.fused_cases()))
def test_fused_loop_against_the_model(name, prec):
    """the device equals the fused model, which test_power_model_host.py shows to differ from the dense one on this very matrix and start vector
    (1025 workgroups: the dense one)"""
    dtype = _dtype(prec)
    opt, lens, nch, nwg, fused = PM.fused_cases()[name]
    mat = PM.square(lens, dtype)
    n = mat[0]
    H = cvr_amd.CvrMatrix(n, n, *mat[2:], **opt)
    try:
        dev = Dev(H)
        model, first, wpb = _fused_model(dev, dtype, opt, mat, fused)
        if nch is not None:
            assert (len(first), -(-len(first) // wpb)) == (nch, nwg)
        starts = PM.start_vectors(n, dtype)
        if fused:
            assert starts[0][1].tobytes() == PM.fused_claim(name, dtype)[2].tobytes()
        _check(dev, model, starts[0][1], list(range(7)), (name, prec, "random"))
        if n < 10000:
            for sname, x0 in starts[1:]:
                _check(dev, model, x0, list(range(7)), (name, prec, sname))
            _check(dev, model, starts[0][1], [2, 5], (name, prec, "shifted"), shift=1)
            _check(dev, model, starts[0][1], [2, 5], (name, prec, "stream"), stream=torch.cuda.Stream())
    finally:
        H.close()


@pytest.mark.parametrize("prec", PRECS)
def test_fused_loop_on_mutable_transposed_and_loaded_handles(prec, tmp_path):
    """a mutable handle after cvr_update_values (the matrix of the claim variant/new_values), a transposed handle (variant/transposed: built from
    the base matrix with cvr_options.transpose, chunks and model of the transpose), and a handle from cvr_load_image (the base matrix itself)"""
    dtype = _dtype(prec)
    opt, base, x0, iters = PM.fused_claim(PM.VARIANT, dtype)
    _, new, x0n, _ = PM.fused_claim("variant/new_values", dtype)
    _, tr, x0t, _ = PM.fused_claim("variant/transposed", dtype)
    n = base[0]
    assert np.array_equal(base[2], new[2]) and np.array_equal(base[3], new[3]) and x0.tobytes() == x0n.tobytes() == x0t.tobytes()

    def run(H, mat, ctx):
        try:
            dev = Dev(H)
            model, _, _ = _fused_model(dev, dtype, opt, mat)
            return _check(dev, model, x0, iters, (ctx, prec))
        finally:
            H.close()

    A = cvr_amd.CvrMatrix(n, n, *base[2:], mutable_values=1, **opt)
    A.update_values(new[4])
    a = run(A, new, "updated")
    b = run(cvr_amd.CvrMatrix(n, n, *new[2:], **opt), new, "fresh")
    assert all(PM.compare(p.x, p.lam, q) == "" for p, q in zip(a, b))
    run(cvr_amd.CvrMatrix(n, n, *base[2:], transpose=1, **opt), tr, "transposed")
    S = cvr_amd.CvrMatrix(n, n, *base[2:], **opt)
    path, key = str(tmp_path / "m.cvrimg"), capi.SourceKey(size=1, mtime_ns=2, hash=3, mode=0)
    S.save_image(path, key)
    S.close()
    run(cvr_amd.CvrMatrix.from_image(path, key, **opt), base, "loaded")


# ---- the fp32 range rule ----
@pytest.mark.parametrize("loop", ["unfused", "fused"])
@pytest.mark.parametrize("name,scale,exact", PM.RULE)
def test_fp32_range_rule(name, scale, exact, loop):
    """est = |A x| / |x| of step 0 on either side of both thresholds and far outside (power_model.RULE; test_power_model_host.py shows on the CPU
    that est falls on the intended side by at least 1e-3 relative); the model's `exact` flag says which trajectory is expected, and the device's
    result is finite and the model's for iters = 1, 2 and 5"""
    n = PM.RULE_N[loop]
    mat = PM.diag_dominant(n, scale)
    opt = PM.PHASES if loop == "fused" else K.LAYOUTS["plain"]
    H = cvr_amd.CvrMatrix(n, n, *mat[2:], **opt)
    try:
        dev = Dev(H)
        model = _fused_model(dev, np.float32, opt, mat)[0] if loop == "fused" else PM.PowerModel(dev.product, np.float32)
        x0 = PM.start_vectors(n, np.float32, PM.RULE_SEED)[0][1]
        if loop == "fused":
            assert x0.tobytes() == PM.fused_claim("rule/" + name, np.float32)[2].tobytes()
        want = _check(dev, model, x0, PM.RULE_ITERS, (name, loop))
        assert [w.exact for w in want] == [False, exact, exact], (name, [w.exact for w in want])
        est, edge = want[1].est, (1e15 if scale > 1 else 1e-15)
        assert (est > edge * (1 + 1e-3)) if scale > edge else (est < edge * (1 - 1e-3)), (name, est)
    finally:
        H.close()


# ---- the sharded form on one GPU ----
def _bounds_cases(n):
    """name -> (bounds, max_rows or None)"""
    def even(p):
        return [n * i // p for i in range(p + 1)]
    c = {"one": ([0, n], None), "two_equal": (even(2), None), "three": (even(3), None), "eight": (even(8), None), "sixty_four": (even(64), None),
         "wider_max_rows": (even(3), n // 3 + 7)}
    if n >= 4:
        a, b = n // 3, n - 1
        c.update(unequal=([0, 1, a, n], None), one_row_shard=([0, a, a + 1, n], None), empty_first=([0, 0, a, n], None), empty_middle=([0, a, a, n], None),
                 empty_last=([0, a, n, n], None), two_empty_in_a_row=([0, a, a, a, b, n], None), empty_everywhere=([0, 0, 0, a, a, b, n, n], n + 3))
    return c


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 65, 4097, G + 1])
def test_sharded_step_on_one_gpu(n, prec):
    """for every set of bounds: the padded step on pad(y) gives byte for byte the x and bit for bit the three sums of the dense step on y (the
    header's claim), both equal the model, with and without the partial sums of a step before; unpad(pad(y)) == y byte for byte, the padding slots
    holding NaN so that a read of one shows in the sums and in x"""
    dtype = _dtype(prec)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(n)
    x, y, yprev = (rng.standard_normal(n).astype(dtype) for _ in range(3))
    model = PM.PowerModel(None, dtype)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # the step before (dense), whose partial sums feed inv of the steps below
    prev, scratch = torch.zeros(3 * 1024, dtype=torch.float64, device="cuda"), torch.full((3 * 1024,), np.nan, dtype=torch.float64, device="cuda")
    xt, ypt = dev(x), dev(yprev)
    s_prev = cvr_amd.power_step_selfcheck(n, dtype == np.float32, xt.data_ptr(), ypt.data_ptr(), prev.data_ptr())
    want_prev = model.step(x, yprev)
    assert tuple(s_prev) == want_prev[1] and xt.cpu().numpy().tobytes() == want_prev[0].tobytes()
    for with_prev in (False, True):
        want_x, want_s = model.step(x, y, want_prev[1][1] if with_prev else None)
        pp = prev.data_ptr() if with_prev else None
        xt, yt = dev(x), dev(y)
        s = cvr_amd.power_step_selfcheck(n, dtype == np.float32, xt.data_ptr(), yt.data_ptr(), scratch.data_ptr(), prev_ptr=pp)
        dense_x = xt.cpu().numpy()
        assert tuple(s) == want_s and dense_x.tobytes() == want_x.tobytes(), ("dense", n, prec, with_prev)
        for name, (bounds, mr) in _bounds_cases(n).items():
            sh = PM.Shards(bounds, mr)
            padded = sh.pad(y)
            xt, pt, dt = dev(x), dev(padded), torch.full((n,), np.nan, dtype=tdt, device="cuda")
            s2 = cvr_amd.power_step_selfcheck(n, dtype == np.float32, xt.data_ptr(), pt.data_ptr(), scratch.data_ptr(), prev_ptr=pp, bounds=bounds,
                                              max_rows=sh.max_rows, dense_ptr=dt.data_ptr())
            mx, ms = PM.sharded_step(model, sh, x, padded, want_prev[1][1] if with_prev else None)
            ctx = (name, n, prec, with_prev)
            assert s2.tobytes() == s.tobytes() and xt.cpu().numpy().tobytes() == dense_x.tobytes(), ctx          # padded == dense
            assert tuple(s2) == ms and mx.tobytes() == dense_x.tobytes(), ctx                                    # == the model
            assert dt.cpu().numpy().tobytes() == y.tobytes(), ctx                                                # unpad(pad(y)) == y
            assert pt.cpu().numpy().tobytes() == padded.tobytes(), ctx


def test_shard_validation_through_the_self_check():
    """iter_shards, the one validation of cvr_power_iteration and of the self-check: 65 shards, bounds that do not end at n, decrease or do not start at
    0 are CVR_ERR_INVALID and nothing is written; so is the self-check's own rule, a max_rows below the longest shard (the loop computes max_rows
    itself).  The loop's call of iter_shards with 65 shards is not run by any test: no communicator of 65 ranks exists on one GPU."""
    n = 130
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.ones(65 * 2, dtype=torch.float64, device="cuda")
    part = torch.zeros(3 * 1024, dtype=torch.float64, device="cuda")
    for bounds, mr in ((list(range(0, 131, 2)), 2), ([0, 100, 130], 50), ([0, 70, 60, 130], 70), ([0, 130, 131], 130), ([1, 130], 130)):
        with pytest.raises(cvr_amd.CvrError) as e:
            cvr_amd.power_step_selfcheck(n, False, x.data_ptr(), y.data_ptr(), part.data_ptr(), bounds=bounds, max_rows=mr)
        assert e.value.code == capi.ERR_INVALID, bounds
    assert (x.cpu().numpy() == 1).all()
