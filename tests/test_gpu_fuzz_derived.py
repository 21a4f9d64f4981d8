"""GPU (MI355X): the operations built on the plain product -- cvr_options.transpose, mutable_values / cvr_update_values, cvr_spmv_scaled_device and
cvr_spmm_device -- over random matrices and random option combinations, where test_gpu_fuzz.py holds the plain product alone.

The cases are fuzz_checks.derived_cases / spmm_cases: cases.random_case (1 .. 3999 rows, 1 .. 5999 columns, empty and giant rows, power-law lengths,
unsorted rows, duplicates, empty columns; at most 100 000 entries), fp32 one case in four, the small value set one in three, and for the first test
cases.random_options (the two option families of test_gpu_fuzz.py).  Each parameter is a block of cases with its own seed (base seed + block);
CVR_FUZZ_CASES multiplies the cases of a block, CVR_FUZZ_SEED replaces the base seed.  The expectations are fuzz_checks.py's, which
tests/test_fuzz_checks_host.py shows to reject wrong results; the coverage the default cases reach is asserted there too.

A case whose options the library refuses for its matrix -- with the same code on the handle and on its twin -- is skipped; at most one case in
eight of a block may be.  Every block prints one line of counts: the cases skipped and the layouts its handles formed (cvr_info)."""
import json

import numpy as np
import pytest

import cvr_amd
import fuzz_checks as FC
from cvr_amd import capi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _try(fn):
    try:
        return fn(), None
    except capi.CvrError as e:
        return None, e.code


def _tdt(H):
    return torch.float64 if H.dtype == np.float64 else torch.float32


def _tally(t, info):
    i = info
    for name, on in (("phases", i.col_phases > 1), ("window", i.x_window > 0), ("hub", i.hub_entries > 0), ("panels", i.col_panels > 1), ("interleave", i.interleave > 0),
                     ("gang", i.gang > 0), ("narrow", i.narrow_cols > 0), ("tags16", i.row_tags16 > 0), ("cut_rows", i.nshared > 0), ("dict", i.value_dict > 0)):
        t[name] = t.get(name, 0) + int(on)
    t["handles"] = t.get("handles", 0) + 1


class Buffers:
    """x_ext and y_ext of one handle on the device, for cvr_spmv_device and cvr_spmv_scaled_device"""

    def __init__(self, H):
        self.H = H
        self.x = torch.zeros(H.info.x_elems, dtype=_tdt(H), device="cuda")
        self.y = torch.zeros(max(H.info.yext_elems, 1), dtype=_tdt(H), device="cuda")

    def plain(self, x):
        H = self.H
        self.x.zero_()
        self.x[: H.ncols] = torch.from_numpy(x)
        self.y.fill_(float("nan"))
        torch.cuda.synchronize()
        H.spmv_device(self.x.data_ptr(), self.y.data_ptr())
        torch.cuda.synchronize()
        return self.y[: H.nrows].cpu().numpy()

    def scaled(self, x, y0, alpha, beta, x_null=False):
        H = self.H
        self.x.zero_()
        if x is not None:
            self.x[: H.ncols] = torch.from_numpy(x)
        self.y.fill_(float("nan"))
        self.y[: H.nrows] = torch.from_numpy(y0)
        torch.cuda.synchronize()
        H.spmv_scaled_device(None if x_null else self.x.data_ptr(), self.y.data_ptr(), alpha, beta)
        torch.cuda.synchronize()
        return self.y[: H.nrows].cpu().numpy()          # (the scratch tail beyond nrows is the library's)


def _check_transpose(c, tally):
    """H = the handle of A^T built on the device, R = the handle of numpy's stable transposition given as device arrays, same options"""
    nrows, ncols, rp, ci, va = c.A
    tn, tm, trp, tci, tva, _ = FC.stable_transpose(nrows, ncols, rp, ci, va)
    R, rcode = _try(lambda: FC._from_device(tn, tm, trp, tci, tva, c.opts))
    H, hcode = _try(lambda: cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, **c.opts))
    assert rcode == hcode, (c.ctx, rcode, hcode, capi.last_error())
    if R is None:
        return False
    try:
        assert (H.nrows, H.ncols) == (ncols, nrows), c.ctx
        FC.assert_same_handle(H, R, lambda: FC._from_device(tn, tm, trp, tci, tva, c.opts))
        y, _ = H.spmv(c.xt)
        yr, _ = R.spmv(c.xt)
        assert FC._bits_equal(y, yr), c.ctx
        FC.assert_transposed_product(y, nrows, ncols, rp, ci, va, c.xt)
        _tally(tally, H.info)
    finally:
        H.close()
        R.close()
    return True


def _check_product(M, c, vals, x, tr):
    y, _ = M.spmv(x)
    if tr:
        FC.assert_transposed_product(y, c.nrows, c.ncols, c.rp, c.ci, vals, x)
    else:
        FC.assert_oracle(y, c.rp, c.ci, vals, x, c.ctx)
    return y


def _check_update_and_scaled(c, tally):
    nrows, ncols, rp, ci, v1 = c.A
    tr = int(c.transposed_update)
    x = c.xt if tr else c.x

    def make(vals, **kw):
        return cvr_amd.CvrMatrix(nrows, ncols, rp, ci, vals, transpose=tr, **kw, **c.opts)

    M, code = _try(lambda: make(v1, mutable_values=1))
    if M is None:          # (a layout the options cannot build for this matrix: refused without the option as well)
        twin, tcode = _try(lambda: make(v1, value_dict=0))
        assert twin is None and tcode == code, (c.ctx, code, tcode)
        return False
    try:
        assert M.info.value_dict == 0 and M.update_values_supported(), c.ctx
        _check_product(M, c, v1, x, tr)
        for vals in (c.v2, c.v3):
            M.update_values(vals)
            y = _check_product(M, c, vals, x, tr)
            B = make(vals, mutable_values=1)
            try:
                assert FC._bits_equal(y, B.spmv(x)[0]), c.ctx
                FC.assert_same_handle(M, B, lambda: make(vals, mutable_values=1))
            finally:
                B.close()
        _tally(tally, M.info)
        _check_scaled(M, c, x)
    finally:
        M.close()
    return True


def _check_scaled(M, c, x):
    """four (alpha, beta) on the updated handle: bit for bit the contract applied to the same handle's plain product"""
    dtype, n = c.dtype, M.nrows
    buf = Buffers(M)
    s = buf.plain(x)
    null_done = False
    for alpha, beta in c.pairs:
        y0 = (c.sub.random(n) * 4 - 2).astype(dtype)
        if n > 0:
            y0[int(c.sub.integers(0, n))] = -0.0          # (beta * -0 + alpha * 0 keeps its sign rules)
        if dtype(beta) == 0:
            y0 = np.full(n, np.nan, dtype=dtype)          # not read
        xin = np.full(len(x), np.nan, dtype=dtype) if dtype(alpha) == 0 else x          # not read
        y = buf.scaled(xin, y0, alpha, beta)
        FC.assert_scaled(y, s, y0, alpha, beta, dtype)
        if dtype(alpha) == 0 and not null_done:
            FC.assert_scaled(buf.scaled(None, y0, alpha, beta, x_null=True), s, y0, alpha, beta, dtype)
            null_done = True
    assert FC._bits_equal(buf.plain(x), s), (c.ctx, "a scaled call left state behind")


@pytest.mark.parametrize("block", range(FC.BLOCKS))
def test_fuzz_transpose_update_scaled(block):
    ncases = FC.cases_per_block()
    skipped, tally = dict(transpose=0, update=0, cases=0), {}
    for c in FC.derived_cases(FC.base_seed(0) + block, ncases):
        t, u = _check_transpose(c, tally), _check_update_and_scaled(c, tally)
        skipped["transpose"] += not t
        skipped["update"] += not u
        skipped["cases"] += not (t and u)
    print("fuzz_derived", json.dumps(dict(test="transpose_update_scaled", block=block, cases=ncases, skipped=skipped, formed=tally)), flush=True)
    assert skipped["cases"] * 8 <= ncases, (skipped, ncases)          # (a refusal the generator should not have drawn: cases.random_options)


def _spmv_columns(A, X):
    """cvr_spmv_device of every column of X on A: (nrows, k)"""
    buf = Buffers(A)
    return np.stack([buf.plain(np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])], axis=1) if X.shape[1] else np.zeros((A.nrows, 0), A.dtype)


def _spmm_raw(A, c):
    """cvr_spmm_device with the case's strides and offsets: X's positions beyond k are NaN, Y starts as the sentinel; the whole Y buffer"""
    info, k = A.info, c.k
    dt = _tdt(A)
    xb = torch.full((c.xoff + info.x_elems * c.ldx + 8,), float("nan"), dtype=dt, device="cuda")
    xv = xb[c.xoff: c.xoff + info.x_elems * c.ldx].view(info.x_elems, c.ldx)
    xv[: A.ncols, :k] = torch.from_numpy(np.ascontiguousarray(c.X))
    xv[A.ncols, :k] = 0          # the pad row
    rows = max(info.yext_elems, 1)
    yb = torch.full((c.yoff + rows * c.ldy + 8,), FC.SENTINEL, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    A.spmm_device(xb.data_ptr() + c.xoff * xb.element_size(), c.ldx, yb.data_ptr() + c.yoff * yb.element_size(), c.ldy, k)
    torch.cuda.synchronize()
    whole = yb.cpu().numpy()
    assert np.all(whole[: c.yoff] == FC.SENTINEL) and np.all(whole[c.yoff + rows * c.ldy:] == FC.SENTINEL), (c.ctx, "written outside the Y block")
    return whole[c.yoff: c.yoff + rows * c.ldy].reshape(rows, c.ldy)


def _check_spmm(A, c, vals):
    cols = _spmv_columns(A, c.X)
    FC.assert_spmm_block(_spmm_raw(A, c), A.nrows, c.k, cols)
    for j in range(c.k):
        FC.assert_oracle(cols[:, j], c.rp, c.ci, vals, c.X[:, j], (c.ctx, "vector", j))


@pytest.mark.parametrize("block", range(FC.BLOCKS))
def test_fuzz_spmm(block):
    ncases = FC.cases_per_block()
    tally = {}
    for c in FC.spmm_cases(FC.base_seed(1) + block, ncases):
        nrows, ncols, rp, ci, va = c.A
        A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=int(c.mutable), **c.opts)
        try:
            assert A.spmm_supported, c.ctx
            _check_spmm(A, c, va)
            if c.mutable:
                A.update_values(c.v2)
                _check_spmm(A, c, c.v2)
            _tally(tally, A.info)
        finally:
            A.close()
    print("fuzz_derived", json.dumps(dict(test="spmm", block=block, cases=ncases, formed=tally)), flush=True)
