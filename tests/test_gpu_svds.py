"""GPU (MI355X): cvr_svds_device / cvr_svds against the numpy model of include/cvr_amd.h (tests/svds_model.py; tests/test_svds_model_host.py shows on
the CPU that the model finds the leading triplets within its bounds and that the comparison used here rejects twelve wrong recurrences).

The model's products are the two handles' own cvr_spmv_device and its small decomposition the library's own cvr_svd_host (held to LAPACK on the
CPU); everything else -- the Gram-Schmidt passes of both halves, the fixed-tree sums, the projected matrix, the estimates, the restart products -- is
the model's own arithmetic.  The device is held to it bit for bit: svals, U, V, nconv, status, restarts, spmv_count and max_estimate, for
max_restarts = 0, 1, 2 at tol = 0 and for a solve to tol.

The shapes are those where the kernels can go wrong: packet tails (3 x 5, 5 x 3, 4 x 4), one workgroup's edge (255 .. 257 on either side), several
workgroups (1023 .. 1025, 4097 x 1025, 40 001 x 4097), every size of the column groups (ncv 3, 8, 20, 64: remainders 3, 0, 4, 0 of the input
streams; left halves of 0 .. 63 and right halves of 1 .. 64 columns), and a square nonsymmetric matrix whose second handle is the same CSR with
transpose = 1.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch

import cvr_amd
import svds_model as SM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-8, np.float32: 1e-4}
SENTINEL = 777.0


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


class Side:
    """one handle with the buffers of its product"""

    def __init__(self, H):
        self.H = H
        self.tdt = torch.float64 if H.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(H.info.x_elems, H.ncols + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, H.nrows, 1), dtype=self.tdt, device="cuda")

    def product(self, p):
        self.xbuf[: self.H.ncols].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.H.nrows].cpu().numpy()


class Pair:
    """the handles of A and A^T and the solver call in the model's terms"""

    def __init__(self, nr, nc, rp, ci, va, explicit=False, opts_a=None, opts_at=None):
        self.nr, self.nc, self.dtype = nr, nc, va.dtype.type
        self.A = cvr_amd.CvrMatrix(nr, nc, rp, ci, va, **(opts_a or {}))
        if explicit:
            self.AT = cvr_amd.CvrMatrix(*SM.transpose_csr(nr, nc, rp, ci, va), **(opts_at or {}))
        else:
            self.AT = cvr_amd.CvrMatrix(nr, nc, rp, ci, va, transpose=1, **(opts_at or {}))
        assert (self.AT.nrows, self.AT.ncols) == (nc, nr)
        self.a, self.at = Side(self.A), Side(self.AT)
        self.tdt = self.a.tdt

    def close(self):
        self.A.close()
        self.AT.close()

    def model(self):
        return SM.SvdsModel(self.a.product, self.at.product, self.dtype)

    def put(self, a, off=0):
        a = np.ascontiguousarray(a, dtype=self.dtype).reshape(-1)
        t = torch.empty(a.size + off, dtype=self.tdt, device="cuda")[off:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, v0, nev, ncv=0, tol=0.0, max_restarts=0, offs=(0, 0, 0), ldu=None, ldv=None, want="UV", stream=None):
        """cvr_svds_device on a start vector of exactly ncols values and nev columns of ldu / ldv values, `offs` values off the allocation's grid (v0,
        U, V), everything filled with a sentinel first; returns (SvdEntry, SvdResult) and checks that nothing outside the returned triplets was
        written and that v0 is unchanged"""
        nr, nc = self.nr, self.nc
        ldu, ldv = nr if ldu is None else ldu, nc if ldv is None else ldv
        vt = self.put(v0, offs[0])
        ut = torch.full((nev * ldu + offs[1],), SENTINEL, dtype=self.tdt, device="cuda")[offs[1]:]
        wt = torch.full((nev * ldv + offs[2],), SENTINEL, dtype=self.tdt, device="cuda")[offs[2]:]
        svals = np.full(nev, SENTINEL)
        opt, res = self.A._svd_options(nev, ncv, tol, max_restarts), capi.SvdResult()
        torch.cuda.synchronize()
        rc = capi.lib().cvr_svds_device(self.A._h, self.AT._h, vt.data_ptr(), svals.ctypes.data, ut.data_ptr() if "U" in want else None, ldu,
                                        wt.data_ptr() if "V" in want else None, ldv, C.byref(opt), C.byref(res), stream)
        torch.cuda.synchronize()
        assert rc == 0, (rc, cvr_amd.last_error())
        assert vt.cpu().numpy().tobytes() == np.ascontiguousarray(v0, dtype=self.dtype).tobytes(), "v0 was written"
        count = 0 if res.status == SM.BREAKDOWN else res.nconv if res.status == SM.INVARIANT else nev
        Ub, Vb = ut.cpu().numpy().reshape(nev, ldu), wt.cpu().numpy().reshape(nev, ldv)
        assert (Ub[:, nr:] == SENTINEL).all() and (Vb[:, nc:] == SENTINEL).all(), "values beyond a column's length were written"
        assert (Ub[count:] == SENTINEL).all() and (Vb[count:] == SENTINEL).all() and (svals[count:] == SENTINEL).all(), "more than the returned triplets was written"
        if "U" not in want:
            assert (Ub == SENTINEL).all()
        if "V" not in want:
            assert (Vb == SENTINEL).all()
        return SM.SvdEntry(svals[:count], np.ascontiguousarray(Ub[:count, :nr].T), np.ascontiguousarray(Vb[:count, :nc].T), res.nconv, res.status, res.restarts,
                           res.spmv_count, res.max_estimate), res


def _same(got, want, ctx, vectors=True):
    msg = SM.compare(got, want, vectors)
    assert msg == "", (ctx, msg)


def _against_the_model(S, v0, nev, ncv, ctx, offs=((0, 0, 0),), lds=((None, None),), cap=8):
    """the bitwise tier for one pair and one (nev, ncv): max_restarts = 0, 1, 2 at tol = 0, then the solve to tol (at most `cap` restarts)"""
    M = S.model()
    M.run(v0, S.nr, nev, ncv, 0.0, 2)
    for r, entry in enumerate(M.history):
        for o in offs:
            for ldu, ldv in lds:
                got, _ = S.solve(v0, nev, ncv, 0.0, r, offs=o, ldu=ldu, ldv=ldv)
                _same(got, entry, (ctx, "max_restarts", r, o, ldu, ldv))
    want = S.model().run(v0, S.nr, nev, ncv, TOL[S.dtype], cap)
    got, _ = S.solve(v0, nev, ncv, TOL[S.dtype], cap, offs=offs[-1], ldu=lds[-1][0], ldv=lds[-1][1])
    _same(got, want, (ctx, "tol"))


# (nrows, ncols) -> the (nev, ncv) pairs run there
SHAPES = {(3, 5): [(1, 3)], (5, 3): [(1, 3)], (4, 4): [(1, 3)], (64, 70): [(8, 64)], (255, 257): [(6, 20)], (257, 255): [(3, 8)], (256, 256): [(1, 3), (3, 8)],
          (1023, 1025): [(3, 8)], (1025, 1023): [(6, 20)], (1024, 1024): [(1, 3)], (4097, 1025): [(3, 8)], (40001, 4097): [(3, 8)]}


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=[f"{r}x{c}" for r, c in sorted(SHAPES)])
def test_shapes_against_the_model(shape, prec):
    """a random rectangular band; v0, U and V on the 16-byte grid and 1 .. 3 values off it, ldu / ldv equal to the column and beyond it"""
    dtype = _dtype(prec)
    nr, nc = shape
    S = Pair(*SM.band_rect(nr, nc, dtype), explicit=nr % 2 == 1)
    try:
        v0 = SM.start_vector(nc, dtype)
        small = max(nr, nc) <= 1025
        for nev, ncv in SHAPES[shape]:
            _against_the_model(S, v0, nev, ncv, ("shape", shape, prec, nev, ncv), offs=((0, 0, 0), (1, 2, 3)) if small else ((3, 1, 2),),
                               lds=((None, None), (nr + 3, nc + 1)) if small else ((nr + 1, nc + 3),), cap=4 if ncv == 64 else 8)
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_square_nonsymmetric_with_the_transposed_handle(prec):
    """at is the same CSR with transpose = 1; U only, V only, neither; two calls and a caller's stream give the same bits; cvr_svds and the Python methods"""
    dtype = _dtype(prec)
    n = 301
    nr, nc, rp, ci, va = SM.random_sparse(n, n, dtype, per_row=5)
    assert not np.array_equal(SM.dense_of(nr, nc, rp, ci, va), SM.dense_of(nr, nc, rp, ci, va).T)
    S = Pair(nr, nc, rp, ci, va)
    try:
        v0, tol = SM.start_vector(n, dtype), TOL[dtype]
        want = S.model().run(v0, n, 3, 16, tol, 40)
        assert want.status == SM.CONVERGED and want.restarts >= 1, want
        got, res = S.solve(v0, 3, 16, tol, 40, stream=torch.cuda.Stream().cuda_stream)
        _same(got, want, ("stream", prec))
        again, _ = S.solve(v0, 3, 16, tol, 40, offs=(1, 3, 2), ldu=n + 5, ldv=n + 2)
        _same(again, want, ("again", prec))
        for only in ("U", "V", ""):
            got, _ = S.solve(v0, 3, 16, tol, 40, want=only)
            _same(got, want, ("blocks", only, prec), vectors=only if only else False)
        # the true residuals of what came back, in fp64: each triplet's returned estimate and the allowance of tests/test_svds_model_host.py
        A = SM.dense_of(nr, nc, rp, ci, va)
        U, V = want.U.astype(np.float64), want.V.astype(np.float64)
        bound = want.scalars["est"] + SM.residual_allowance(dtype, want.svals[0])          # the returned estimates (max_estimate is their largest, scaled)
        assert res.max_estimate == (want.scalars["est"] / np.maximum(SM.EPS23, want.svals)).max()
        assert (np.linalg.norm(A @ V - U * want.svals, axis=0) <= bound).all() and (np.linalg.norm(A.T @ U - V * want.svals, axis=0) <= bound).all()
        assert (np.abs(want.svals - np.linalg.svd(A, compute_uv=False)[:3]) <= bound).all()
        # the host entry point and the Python methods
        sv, U, V, hres = S.A.svds_host(S.AT, v0, 3, 16, tol, 40)
        assert sv.tobytes() == want.svals.tobytes() and np.ascontiguousarray(U).tobytes() == np.ascontiguousarray(want.U).tobytes()
        assert np.ascontiguousarray(V).tobytes() == np.ascontiguousarray(want.V).tobytes()
        assert (hres.nconv, hres.status, hres.restarts, hres.spmv_count, hres.max_estimate) == (res.nconv, res.status, res.restarts, res.spmv_count, res.max_estimate)
        sv, U, V, _ = S.A.svds(S.AT, S.put(v0), 3, 16, tol, 40)
        assert sv.tobytes() == want.svals.tobytes() and U.cpu().numpy().tobytes() == np.ascontiguousarray(want.U.T).tobytes()
        assert V.cpu().numpy().tobytes() == np.ascontiguousarray(want.V.T).tobytes()
        sv, U, V, r = S.A.svds(S.AT, nev=2, tol=tol, vectors=False)
        assert U is None and V is None and r.status == SM.CONVERGED and len(sv) == 2
        sv, U, V, _ = S.A.svds_host(S.AT, v0, 3, 16, tol, 40, vectors=False)
        assert U is None and V is None and sv.tobytes() == want.svals.tobytes()
    finally:
        S.close()


def _diag_case(dtype):
    """A (96 x 97) with A[i, i] = d_i, 1 <= d_i <= 8 distinct, and an empty last column"""
    d = 1.0 + 7.0 * ((np.arange(96) * 37) % 96) / 96.0
    return 96, 97, np.arange(97, dtype=np.int64), np.arange(96, dtype=np.int32), d.astype(dtype), d.astype(dtype).astype(np.float64)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_closed_halves_and_breakdowns(prec):
    dtype = _dtype(prec)
    nr, nc, rp, ci, va, d = _diag_case(dtype)
    S = Pair(nr, nc, rp, ci, va)
    rtol = 1e-6 if dtype == np.float32 else 1e-13
    try:
        # v0 = e_i: the right half closes at step 0 with the exact triplet
        e = np.zeros(nc, dtype=dtype)
        e[11] = 1
        got, _ = S.solve(e, 1, 3, 1e-8, 5)
        assert (got.status, got.nconv, got.restarts, got.max_estimate, got.spmv_count) == (SM.CONVERGED, 1, 0, 0.0, 6) and got.svals[0] == d[11], (got, d[11])
        assert got.V[:, 0].tolist() == e.tolist() and got.U[:, 0].tolist() == e[:nr].tolist()
        _same(got, S.model().run(e, nr, 1, 3, 1e-8, 5), ("e_i", prec))
        # three entries: the right half closes at step 2; nev = 4: fewer triplets than wanted
        v = np.zeros(nc, dtype=dtype)
        v[[0, 40, 95]] = (1.0, 2.0, -1.5)
        want = S.model().run(v, nr, 4, 6, 1e-8, 5)
        got, _ = S.solve(v, 4, 6, 1e-8, 5, offs=(1, 1, 1), ldu=nr + 2, ldv=nc + 2)
        assert (got.status, got.nconv, got.restarts) == (SM.INVARIANT, 3, 0) and np.allclose(got.svals, np.sort(d[[0, 40, 95]])[::-1], rtol=rtol, atol=0), got
        _same(got, want, ("three entries", prec))
        # two entries and a component in the null space: the left half closes at step 2 with a 2 x 3 projected matrix
        v = np.zeros(nc, dtype=dtype)
        v[[7, 50, 96]] = (1.0, -2.0, 0.7)
        for nev, status in ((2, SM.CONVERGED), (3, SM.INVARIANT)):
            want = S.model().run(v, nr, nev, 6, 1e-8, 5)
            assert (want.scalars["p"], want.scalars["q"]) == (2, 3)
            got, _ = S.solve(v, nev, 6, 1e-8, 5)
            assert (got.status, got.nconv, got.max_estimate) == (status, 2, 0.0) and np.allclose(got.svals, np.sort(d[[7, 50]])[::-1], rtol=rtol, atol=0), got
            _same(got, want, ("left half", nev, prec))
        # v0 in the null space: the left half closes at step 0 and nothing is returned (solve() checks the sentinels)
        e = np.zeros(nc, dtype=dtype)
        e[96] = 1
        got, _ = S.solve(e, 2, 6, 1e-8, 5)
        assert (got.status, got.nconv, len(got.svals), got.U.shape, got.V.shape, got.max_estimate) == (SM.INVARIANT, 0, 0, (nr, 0), (nc, 0), 0.0), got
        _same(got, S.model().run(e, nr, 2, 6, 1e-8, 5), ("null space", prec))
        # v0 = 0 and a NaN in v0: breakdown, nothing written
        for bad in (np.zeros(nc, dtype=dtype), np.where(np.arange(nc) == 5, np.nan, 1.0).astype(dtype)):
            got, _ = S.solve(bad, 2, 6, 1e-8, 5)
            assert (got.status, got.nconv, len(got.svals), got.U.shape, got.V.shape) == (SM.BREAKDOWN, 0, 0, (nr, 0), (nc, 0)), got
            _same(got, S.model().run(bad, nr, 2, 6, 1e-8, 5), ("breakdown", prec))
    finally:
        S.close()
    # a NaN among A's values
    vn = va.copy()
    vn[40] = np.nan
    S = Pair(nr, nc, rp, ci, vn)
    try:
        got, _ = S.solve(np.ones(nc, dtype=dtype), 2, 6, 1e-8, 5)
        assert (got.status, got.nconv, len(got.svals)) == (SM.BREAKDOWN, 0, 0), got
    finally:
        S.close()


def test_errors_with_real_handles():
    dtype = np.float64
    nr, nc, rp, ci, va = SM.band_rect(44, 30, dtype)
    L = capi.lib()
    opt, res = capi.SvdOptions(), capi.SvdResult()
    L.cvr_svd_default_options(C.byref(opt))
    vt = torch.ones(nr + nc + 8, dtype=torch.float64, device="cuda")
    ut = torch.zeros(4 * (nr + nc) + 8, dtype=torch.float64, device="cuda")
    sv = np.zeros(8)
    torch.cuda.synchronize()
    S = Pair(nr, nc, rp, ci, va)
    A32 = cvr_amd.CvrMatrix(nr, nc, rp, ci, va.astype(np.float32), transpose=1)
    try:
        def call(a, at, ldu=nr, ldv=nc, U=True, V=True):
            return L.cvr_svds_device(a, at, vt.data_ptr(), sv.ctypes.data, ut.data_ptr() if U else None, ldu, ut.data_ptr() if V else None, ldv, C.byref(opt), C.byref(res), None)
        # either handle before cvr_preprocess
        view = capi.CsrView(nr, nc, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
        h = C.c_void_p()
        assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
        for a, at in ((h, S.AT._h), (S.AT._h, h)):
            assert call(a, at) == capi.ERR_STATE and "cvr_preprocess" in cvr_amd.last_error()
        hv = np.ones(nr + nc)
        assert L.cvr_svds(h, S.AT._h, hv.ctypes.data, sv.ctypes.data, None, 0, None, 0, C.byref(opt), C.byref(res)) == capi.ERR_STATE
        L.cvr_destroy(h)
        # at is not ncols x nrows of a: swapped handles of a non-square pair, A beside itself
        for a, at in ((S.AT._h, S.AT._h), (S.A._h, S.A._h)):
            assert call(a, at) == capi.ERR_INVALID and "transpose" in cvr_amd.last_error()
        # mixed value types
        assert call(S.A._h, A32._h) == capi.ERR_INVALID and "type" in cvr_amd.last_error()
        # another device, where there is one
        if capi.device_count() > 1:
            far = cvr_amd.CvrMatrix(nr, nc, rp, ci, va, transpose=1, device=1)
            try:
                assert call(S.A._h, far._h) == capi.ERR_INVALID and "devices" in cvr_amd.last_error()
            finally:
                far.close()
        # ncv beyond the smaller side; the leading dimensions
        opt.ncv = 31
        assert call(S.A._h, S.AT._h) == capi.ERR_INVALID and "ncv" in cvr_amd.last_error()
        opt.ncv = 0
        assert call(S.A._h, S.AT._h, ldu=nr - 1) == capi.ERR_INVALID and "ldu" in cvr_amd.last_error()
        assert call(S.A._h, S.AT._h, ldv=nc - 1) == capi.ERR_INVALID and "ldv" in cvr_amd.last_error()
        assert call(S.A._h, S.AT._h, ldu=nr - 1, U=False, V=False) == 0, cvr_amd.last_error()          # a null block's leading dimension is not looked at
        torch.cuda.synchronize()
    finally:
        A32.close()
        S.close()
    assert not ut.cpu().numpy().any()
