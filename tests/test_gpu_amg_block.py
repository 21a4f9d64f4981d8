"""GPU (MI355X): the AMG object for blocks of right-hand sides -- cvr_precond_amg_block, cvr_precond_amg_block_info, and
cvr_precond_apply_device / cvr_precond_apply_multi_device / cvr_pcg_device / cvr_pcg_multi_device / cvr_pcg_multi with such an object, through the ABI.

  * the hierarchy: info, every exported level and prolongator of a block object are the ordinary constructor's byte for byte, for the three set-ups,
    fp64 and fp32, on the Laplacian at m = 3 and 24 and banded "spd" at n = 1, 2, 65, 1025
  * the single-vector apply of a K = 4 object bit for bit against the cycle the test carries out itself (amg_model / sa_amg_model) with products through
    CvrMatrix handles made from the exported levels with nvec = 4, every product held to the CSR loop by fuzz_checks; r and z off the 16-byte grid one
    at a time; again behind a block call (which writes where the single-vector pads lie)
  * the block apply: K in {1, 2, 3, 8}, every nvec <= K from the widest down (stale columns stay in the buffers), both leading-dimension pairs, both
    offsets; column c is cvr_precond_apply_device's on column c bit for bit; the padding columns and the rows behind n keep their NaN
  * block PCG on m = 24 with K = 4, nvec = 3: a generic column, b = 0 and an easy one, against three cvr_pcg_device calls, bit for bit
  * the errors, the entry points that still decline, an ordinary object still declined in the pinned words"""
import ctypes as C

import numpy as np
import pytest
import torch

import amg_model as AM
import cvr_amd
import fuzz_checks as FC
import krylov_model as KM
import mis2_amg_model as M2          # noqa: F401  (the MIS(2) model's cases are the smoothed model's cycle)
import pkrylov_gpu as G
import sa_amg_model as SA
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

SETUPS = ["plain", "smoothed", "mis2"]
ORDINARY = {"plain": capi.Precond.amg, "smoothed": capi.Precond.amg_smoothed, "mis2": capi.Precond.amg_mis2}


def _matrix_handle(n, rp, ci, va, K):
    """level 0's handle: the plain layout for K >= 2, the default one for K = 1"""
    return cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8) if K >= 2 else cvr_amd.CvrMatrix(n, n, rp, ci, va)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _export(P, setup):
    info = P.amg_info()
    out = dict(info=bytes(info), levels=[P.amg_export_level(l) for l in range(info.levels)], sinfo=bytes(P.amg_smoothed_info()), minfo=bytes(P.amg_mis2_info()), pro=[])
    if setup != "plain":
        out["pro"] = [P.amg_export_prolongator(l) for l in range(info.levels - 1)]
    return out


def _same_exports(a, b):
    for f in ("info", "sinfo", "minfo"):
        if a[f] != b[f]:
            return f
    if len(a["levels"]) != len(b["levels"]) or len(a["pro"]) != len(b["pro"]):
        return "the number of levels"
    for l, (x, y) in enumerate(zip(a["levels"], b["levels"])):
        for f in ("rp", "ci", "va", "dinv", "agg", "winv"):
            u, v = getattr(x, f), getattr(y, f)
            if (u is None) != (v is None) or (u is not None and (u.dtype != v.dtype or u.tobytes() != v.tobytes())):
                return f"level {l}: {f}"
    for l, (x, y) in enumerate(zip(a["pro"], b["pro"])):
        for f in ("rp", "ci", "va"):
            if getattr(x, f).tobytes() != getattr(y, f).tobytes():
                return f"P_{l}: {f}"
    return ""


# ---- the hierarchy ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("name, K", [("laplacian-3", 2), ("laplacian-24", 4), ("spd-1", 8), ("spd-2", 3), ("spd-65", 1), ("spd-1025", 8)])
def test_the_hierarchy_is_the_ordinary_constructors_byte_for_byte(name, K, setup, prec):
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = AM.matrix(name, dtype)
    A = _matrix_handle(n, rp, ci, va, K)
    kw = {} if setup == "plain" else dict(omega=0.9)
    P = ORDINARY[setup](A, rp, ci, va, sweeps=2, **kw)
    B = capi.Precond.amg_block(A, rp, ci, va, K, setup=setup, sweeps=2, **kw)
    rt, ct, vt = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    D = capi.Precond.amg_block_from_device(A, n, rt.data_ptr(), ct.data_ptr(), vt.data_ptr(), K, is_f32=dtype == np.float32, setup=setup, sweeps=2, **kw)
    del rt, ct, vt
    try:
        want = _export(P, setup)
        for obj in (B, D):
            assert _same_exports(_export(obj, setup), want) == "", (name, K, setup, prec)
            bi = obj.amg_block_info()
            assert (bi.nvec, bi.setup, list(bi.reserved)) == (K, capi.AMG_SETUPS[setup], [0] * 8) and bi.buffer_bytes > 0
            pi = obj.info
            assert (pi.n, pi.block_size, pi.is_f32, pi.nblocks, pi.identity_blocks) == (n, 0, int(dtype == np.float32), 0, 0)
        with pytest.raises(capi.CvrError) as e:
            P.amg_block_info()
        assert e.value.code == capi.ERR_INVALID and "was not built by cvr_precond_amg_block" in str(e.value)
    finally:
        for o in (P, B, D):
            o.close()
        A.close()


# ---- the single-vector apply ----
class RectDev:
    """a handle of any shape with the buffers of a product through cvr_spmv_device"""

    def __init__(self, H, nrows, ncols):
        self.H, self.nrows, self.ncols = H, nrows, ncols
        self.xbuf = torch.zeros(max(H.info.x_elems, ncols + 1), dtype=G.tdt(H.dtype), device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, nrows, 1), dtype=G.tdt(H.dtype), device="cuda")

    def product(self, x):
        self.xbuf[: self.ncols].copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.nrows].cpu().numpy()


class Levels:
    """what a caller makes of a block object's exports: the model's hierarchy and handles of A_l (l >= 1) and, for the smoothed set-ups, P_l and
    R_l = P_l^T, made as the object makes its own: device arrays, cvr_options.nvec = K.  Every product is held to the CSR loop."""

    def __init__(self, A, P, setup, K):
        self.K, self.count, self.handles, self.keep = K, 0, [], []
        info = P.amg_info()
        exp = [P.amg_export_level(l) for l in range(info.levels)]
        if setup == "plain":
            self.H = AM.from_export(info, exp, P.dtype)
        else:
            self.H = SA.from_export(info, P.amg_smoothed_info(), exp, [P.amg_export_prolongator(l) for l in range(info.levels - 1)], P.dtype)
        self.smoothed = setup != "plain"
        self.A = [self._checked(RectDev(A, A.nrows, A.nrows).product, exp[0].rp, exp[0].ci, exp[0].va)]
        for l, e in enumerate(exp[1:], 1):
            self.A.append(None if l == info.levels - 1 and info.coarse_direct else self._handle(e.n, e.n, e.rp, e.ci, e.va))
        if self.smoothed:
            self.P = [self._handle(p.nrows, p.ncols, p.rp, p.ci, p.va) for p in self.H.P]
            self.R = [self._handle(r.nrows, r.ncols, r.rp, r.ci, r.va) for r in self.H.R]

    def _checked(self, product, rp, ci, va):
        def checked(x):
            y = product(x)
            self.count += 1
            FC.assert_oracle(y, rp, ci, va, x, ctx=("a product of", len(rp) - 1, "rows"))
            return y
        return checked

    def _handle(self, nrows, ncols, rp, ci, va):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, va)]
        torch.cuda.synchronize()
        self.keep.append(t)
        h = cvr_amd.CvrMatrix.from_device(nrows, ncols, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), is_f32=va.dtype == np.float32, nvec=self.K)
        self.handles.append(h)
        return self._checked(RectDev(h, nrows, ncols).product, rp, ci, va)

    def apply(self, r):
        return SA.apply(self.H, self.A, self.P, self.R, r) if self.smoothed else AM.apply(self.H, self.A, r)

    def close(self):
        for h in self.handles:
            h.close()


def _apply(P, r, dtype, rshift=0, zshift=0):
    rt = G.put(r, dtype, rshift)
    zt = G.put(np.full(len(r), np.nan), dtype, zshift)
    torch.cuda.synchronize()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    return zt.cpu().numpy()


def _apply_multi(P, R, ldr, ldz, shift=0):
    """cvr_precond_apply_multi_device on R of exactly n rows and Z of n + 2; every value the call must not read or write is a NaN and stays one"""
    n, nvec = R.shape
    hr = np.full((n, ldr), np.nan, dtype=P.dtype)
    hr[:, :nvec] = R
    hz = np.full((n + 2, ldz), np.nan, dtype=P.dtype)
    rt, zt = G.put(hr.reshape(-1), P.dtype, shift), G.put(hz.reshape(-1), P.dtype, shift)
    torch.cuda.synchronize()
    P.apply_multi(rt.data_ptr(), ldr, zt.data_ptr(), ldz, nvec)
    torch.cuda.synchronize()
    assert _bits(rt.cpu().numpy()) == _bits(hr), "R was written"
    Z = zt.cpu().numpy().reshape(n + 2, ldz)
    assert _bits(Z[:n, nvec:]) == _bits(hz[:n, nvec:]), "the padding columns of Z were written"
    assert _bits(Z[n:]) == _bits(hz[n:]), "rows behind n were written"
    return np.ascontiguousarray(Z[:n, :nvec])


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("setup", SETUPS)
def test_the_single_vector_apply_is_the_cycle_with_handles_of_nvec_4(setup, prec):
    dtype, K = G.dtype_of(prec), 4
    n, _, rp, ci, va = synth.laplacian_2d(24, dtype)
    A = _matrix_handle(n, rp, ci, va, K)
    P = capi.Precond.amg_block(A, rp, ci, va, K, setup=setup)
    lv = Levels(A, P, setup, K)
    try:
        r = KM.inputs(n, dtype)[0]
        want = lv.apply(r)
        per_apply = P.amg_smoothed_info().products_per_apply if setup != "plain" else lv.H.products_per_apply()
        assert lv.count == per_apply and np.isfinite(want).all() and want.any()
        for rshift, zshift in ((0, 0), (1, 0), (0, 1), (0, 0)):
            got = _apply(P, r, dtype, rshift, zshift)
            assert _bits(got) == _bits(want), (setup, prec, rshift, zshift, int(np.sum(got != want)))
        R = np.random.default_rng(3).standard_normal((n, K)).astype(dtype)          # a block call writes the elements that are pads at ld = 1
        R[:, 2] = r
        Z = _apply_multi(P, R, K, K)
        assert _bits(Z[:, 2]) == _bits(want)
        assert _bits(_apply(P, r, dtype)) == _bits(want)
    finally:
        lv.close()
        P.close()
        A.close()


# ---- the block apply ----
BLOCK_CASES = [("laplacian-3", dict(coarse_size=1, max_levels=2)), ("laplacian-24", {}), ("spd-1025", {}), ("blocks", {}), ("diagonal", {}), ("laplacian-24", dict(coarse_size=1)),
               ("laplacian-24", dict(sweeps=2, coarse_scale=1.5))]
BLOCK_PARAMS = [(c, s, "fp64") for c in BLOCK_CASES for s in ("plain", "smoothed")] + [(("laplacian-24", {}), "mis2", "fp64")] + [
    (("laplacian-24", {}), s, "fp32") for s in SETUPS] + [(("spd-1025", {}), "plain", "fp32")]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("case, setup, prec", BLOCK_PARAMS, ids=lambda v: AM.case_id(v) if isinstance(v, tuple) else str(v))
def test_block_apply_is_the_single_apply_column_by_column(case, setup, prec, K):
    name, options = case
    dtype = G.dtype_of(prec)
    n, _, rp, ci, va = AM.matrix(name, dtype)
    A = _matrix_handle(n, rp, ci, va, K)
    P = capi.Precond.amg_block(A, rp, ci, va, K, setup=setup, **options)
    try:
        info = P.amg_info()
        if name == "laplacian-3":
            assert (info.levels, info.coarse_direct) == (2, 1)          # a direct coarsest level right below level 0
        if name == "diagonal":
            assert info.levels == 1
        R = np.random.default_rng(n * 10 + K).standard_normal((n, K)).astype(dtype)
        R[n // 2, 0] = -0.0
        refs = [_apply(P, R[:, c], dtype) for c in range(K)]
        assert all(np.isfinite(z).all() and z.any() for z in refs)
        for nvec in list(range(K, 0, -1)) + [K]:          # the widest first: a narrower call meets stale columns in the buffers
            for ldr, ldz in ((nvec, nvec), (nvec + 3, nvec + 1)):
                for shift in (0, 1):
                    Z = _apply_multi(P, R[:, :nvec], ldr, ldz, shift)
                    for c in range(nvec):
                        assert _bits(Z[:, c]) == _bits(refs[c]), (name, setup, prec, K, nvec, ldr, ldz, shift, c, int(np.sum(Z[:, c] != refs[c])))
        assert _bits(_apply(P, R[:, 0], dtype)) == _bits(refs[0])          # ... and the single-vector call behind them
    finally:
        P.close()
        A.close()


# ---- block PCG ----
def _single(H, P, b, x0, **kw):
    bt, xt = G.put(b, H.dtype), G.put(x0, H.dtype)
    torch.cuda.synchronize()
    res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), res


def _multi(H, P, B, X0, ldb, ldx, shift=0, **kw):
    n, nvec = B.shape
    hb, hx = np.full((n, ldb), np.nan, dtype=H.dtype), np.full((n, ldx), np.nan, dtype=H.dtype)
    hb[:, :nvec], hx[:, :nvec] = B, X0
    bt, xt = G.put(hb.reshape(-1), H.dtype, shift), G.put(hx.reshape(-1), H.dtype, shift)
    torch.cuda.synchronize()
    res = H.pcg_multi(P, bt.data_ptr(), ldb, xt.data_ptr(), ldx, nvec, **kw)
    torch.cuda.synchronize()
    assert _bits(bt.cpu().numpy()) == _bits(hb), "B was written"
    X = xt.cpu().numpy().reshape(n, ldx)
    assert _bits(X[:, nvec:]) == _bits(hx[:, nvec:]), "the padding columns of X were written"
    return np.ascontiguousarray(X[:, :nvec]), res


def _products_per_apply(P, setup):
    if setup != "plain":
        return P.amg_smoothed_info().products_per_apply
    i = P.amg_info()
    return 2 * i.sweeps * (i.levels - 1) + (0 if i.coarse_direct else 2 * i.sweeps - 1)


@pytest.mark.parametrize("setup, prec", [("plain", "fp64"), ("smoothed", "fp64"), ("mis2", "fp64"), ("plain", "fp32")])
def test_block_pcg_is_three_single_solves_bit_for_bit(setup, prec):
    dtype, K, nvec, m = G.dtype_of(prec), 4, 3, 24
    n, _, rp, ci, va = synth.laplacian_2d(m, dtype)
    A = _matrix_handle(n, rp, ci, va, K)
    P = capi.Precond.amg_block(A, rp, ci, va, K, setup=setup)
    try:
        per_apply = _products_per_apply(P, setup)
        g = np.arange(n) % m / (m - 1.0)
        smooth = np.sin(np.pi * g) * np.sin(np.pi * (np.arange(n) // m) / (m - 1.0))
        Asmooth = AM.csr_product(n, rp, ci, va, dtype)(smooth.astype(dtype))
        B = np.stack([KM.inputs(n, dtype)[0], np.zeros(n, dtype=dtype), Asmooth], axis=1).astype(dtype)
        rtol = 1e-8 if dtype == np.float64 else 1e-4
        X0 = np.random.default_rng(11).standard_normal((n, nvec)).astype(dtype)
        X0[:, 2] = smooth * (1.0 + 10 * rtol)          # a start whose residual is 10 rtol |b|: a few steps
        for kw in [dict(rtol=0.0, max_iters=k) for k in range(5)] + [dict(rtol=rtol, max_iters=100)]:
            singles = [_single(A, P, B[:, j], X0[:, j], check_every=1, **kw) for j in range(nvec)]
            if kw["max_iters"] == 100:
                its = [r.iterations for _, r in singles]
                assert all(r.status == capi.CG_CONVERGED for _, r in singles) and its[1] == 0 and its[2] < its[0], its          # stops at once; stops early
            for every in (1, 3, 0):
                for ldb, ldx in ((nvec, nvec), (nvec + 2, nvec + 2)):
                    for shift in (0, 1) if every == 1 else (0,):
                        X, res = _multi(A, P, B, X0, ldb, ldx, shift, check_every=every, **kw)
                        for j in range(nvec):
                            x, r = singles[j]
                            ctx = (setup, prec, kw, every, ldb, ldx, shift, j)
                            assert _bits(X[:, j]) == _bits(x), (ctx, int(np.sum(X[:, j] != x)))          # (a stopped column: untouched behind its stop)
                            assert (res[j].iterations, res[j].status) == (r.iterations, r.status), ctx
                            assert _bits(np.array([res[j].residual_norm, res[j].b_norm])) == _bits(np.array([r.residual_norm, r.b_norm])), ctx
                        step = every or 8
                        most = max(r.iterations for _, r in singles)
                        enqueued = kw["max_iters"] if kw["rtol"] == 0.0 else min(-(-most // step) * step, kw["max_iters"])
                        assert all(res[j].spmv_count == 1 + per_apply + (1 + per_apply) * enqueued for j in range(nvec)), (kw, every, res[0].spmv_count, enqueued)
        Xh, resh = A.pcg_multi_host(P, B, X0=X0, rtol=rtol, max_iters=100)          # the host twin
        for j in range(nvec):
            assert _bits(Xh[:, j]) == _bits(singles[j][0]) and resh[j].iterations == singles[j][1].iterations
    finally:
        P.close()
        A.close()


# ---- errors and declines ----
def test_errors_declines_and_an_object_still_usable_behind_them():
    L = capi.lib()
    n, _, rp, ci, va = synth.laplacian_2d(24)
    A = _matrix_handle(n, rp, ci, va, 8)
    D = cvr_amd.CvrMatrix(n, n, rp, ci, va)          # the default layout
    P = capi.Precond.amg_block(A, rp, ci, va, 2, setup="smoothed")
    O = capi.Precond.amg(A, rp, ci, va)
    try:
        r = KM.inputs(n, np.float64)[0]
        want = _apply(P, r, np.float64)
        R = np.stack([r, r, r], axis=1)
        rt, zt = G.put(R.reshape(-1), np.float64), G.put(np.zeros(3 * n), np.float64)
        opt, res = capi.CgOptions(), (capi.CgResult * 3)()
        L.cvr_cg_default_options(C.byref(opt))
        # nvec > K: both numbers, nothing written
        assert L.cvr_precond_apply_multi_device(P._p, rt.data_ptr(), 3, zt.data_ptr(), 3, 3, None) == capi.ERR_INVALID
        assert "nvec = 3" in capi.last_error() and "2 columns" in capi.last_error(), capi.last_error()
        assert L.cvr_pcg_multi_device(A._h, P._p, rt.data_ptr(), 3, zt.data_ptr(), 3, 3, C.byref(opt), res, None) == capi.ERR_INVALID
        assert "nvec = 3" in capi.last_error() and "2 columns" in capi.last_error(), capi.last_error()
        hb, hx = R.copy(), np.zeros((n, 3))
        assert L.cvr_pcg_multi(A._h, P._p, hb.ctypes.data, hx.ctypes.data, 3, C.byref(opt), res) == capi.ERR_INVALID
        torch.cuda.synchronize()
        assert not zt.cpu().numpy().any() and not hx.any()
        # ... behind the existing checks in their order
        assert L.cvr_precond_apply_multi_device(P._p, rt.data_ptr(), 3, zt.data_ptr(), 3, 9, None) == capi.ERR_INVALID and "1 to 8" in capi.last_error()
        assert L.cvr_precond_apply_multi_device(P._p, rt.data_ptr(), 2, zt.data_ptr(), 3, 3, None) == capi.ERR_INVALID and "ldr" in capi.last_error()
        # K = 2 on a handle without the plain layout
        nw, _, prp, pci, _ = synth.web_google_like(0.5)
        nw, _, rpw, ciw, vaw = synth.spd_from_pattern(nw, prp, pci)
        W = cvr_amd.CvrMatrix(nw, nw, rpw, ciw, vaw)          # default options: the rules pick a layout that is not the plain one
        assert not W.spmm_supported
        with pytest.raises(capi.CvrError) as e:
            capi.Precond.amg_block(W, rpw, ciw, vaw, 2)
        W.close()
        assert e.value.code == capi.ERR_STATE and "cvr_options.nvec >= 2" in str(e.value) and str(e.value).count("cvr_precond_amg_block") >= 1
        one = capi.Precond.amg_block(D, rp, ci, va, 1)          # K = 1 takes any handle
        z1 = _apply_multi(one, r.reshape(n, 1), 1, 1)
        assert _bits(z1[:, 0]) == _bits(_apply(one, r, np.float64))
        X1, r1 = D.pcg_multi_host(one, r.reshape(n, 1), rtol=1e-8, max_iters=100)          # nvec = 1, ld = 1 on a default handle
        xs, rs = D.pcg_host(one, r, rtol=1e-8, max_iters=100)
        assert _bits(X1[:, 0]) == _bits(xs) and r1[0].iterations == rs.iterations and rs.status == capi.CG_CONVERGED
        one.close()
        # the entry points that decline kind 4 decline the block object in the same words
        bt, xt = G.put(r, np.float64), G.put(np.zeros(n), np.float64)
        out, hb1, hx1 = np.zeros(len(va)), r.copy(), np.zeros(n)
        one_res = capi.CgResult()

        def declined(rc, name):
            assert rc == capi.ERR_STATE and "kind 4 (AMG)" in capi.last_error(), (name, rc, capi.last_error())

        declined(L.cvr_precond_export(P._p, out.ctypes.data), "export")
        declined(L.cvr_pbicgstab_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), C.byref(opt), C.byref(one_res), None), "pbicgstab_device")
        declined(L.cvr_pbicgstab(A._h, P._p, hb1.ctypes.data, hx1.ctypes.data, C.byref(opt), C.byref(one_res)), "pbicgstab")
        declined(L.cvr_pgmres_device(A._h, P._p, bt.data_ptr(), xt.data_ptr(), 30, C.byref(opt), C.byref(one_res), None), "pgmres_device")
        declined(L.cvr_pgmres(A._h, P._p, hb1.ctypes.data, hx1.ctypes.data, 30, C.byref(opt), C.byref(one_res)), "pgmres")
        # an ordinary object is declined by the multi entry points in the pinned words
        words = "the preconditioner is of kind 4 (AMG): this entry point takes block-Jacobi objects (kind 0) only"
        assert L.cvr_precond_apply_multi_device(O._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, None) == capi.ERR_STATE
        assert capi.last_error() == "cvr_precond_apply_multi_device: " + words
        assert L.cvr_pcg_multi_device(A._h, O._p, bt.data_ptr(), 1, xt.data_ptr(), 1, 1, C.byref(opt), C.byref(one_res), None) == capi.ERR_STATE
        assert capi.last_error() == "cvr_pcg_multi: " + words
        assert L.cvr_pcg_multi(A._h, O._p, hb1.ctypes.data, hx1.ctypes.data, 1, C.byref(opt), C.byref(one_res)) == capi.ERR_STATE
        assert capi.last_error() == "cvr_pcg_multi: " + words
        torch.cuda.synchronize()
        assert not xt.cpu().numpy().any() and not hx1.any() and not out.any()
        # the info call on other objects
        J = capi.Precond.block_jacobi(rp, ci, va, 4)
        assert L.cvr_precond_amg_block_info(J._p, C.byref(capi.AmgBlockInfo())) == capi.ERR_INVALID and "is of kind 0, not" in capi.last_error()
        J.close()
        assert L.cvr_precond_amg_block_info(O._p, C.byref(capi.AmgBlockInfo())) == capi.ERR_INVALID and "was not built by cvr_precond_amg_block" in capi.last_error()
        assert L.cvr_precond_amg_block_info(P._p, None) == capi.ERR_INVALID
        # behind all of it the object applies as before, alone and in a block
        assert _bits(_apply(P, r, np.float64)) == _bits(want)
        Z = _apply_multi(P, R[:, :2], 2, 2)
        assert _bits(Z[:, 0]) == _bits(want) and _bits(Z[:, 1]) == _bits(want)
    finally:
        P.close()
        O.close()
        A.close()
        D.close()


def test_n_zero():
    rp, ci, va = np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)
    A = cvr_amd.CvrMatrix(0, 0, rp, ci, va)
    P = capi.Precond.amg_block(A, rp, ci, va, 1, setup="smoothed")
    try:
        bi = P.amg_block_info()
        assert (bi.nvec, bi.setup) == (1, 1) and P.amg_info().levels == 1
        t = torch.zeros(8, dtype=torch.float64, device="cuda")
        assert capi.lib().cvr_precond_apply_multi_device(P._p, t.data_ptr(), 1, t[4:].data_ptr(), 1, 1, None) == 0
        assert capi.lib().cvr_precond_apply_device(P._p, t.data_ptr(), t[4:].data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert not t.cpu().numpy().any()
    finally:
        P.close()
        A.close()
