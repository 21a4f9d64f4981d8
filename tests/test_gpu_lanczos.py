"""GPU (MI355X): cvr_eigsh_device / cvr_eigsh against the numpy model of include/cvr_amd.h (tests/lanczos_model.py; tests/test_lanczos_model_host.py
shows on the CPU that the model finds the extreme eigenpairs within its bounds and that the comparison used here rejects nine wrong recurrences).

The model's product is the handle's own cvr_spmv_device and its small eigensolver the library's own cvr_sym_eig_host (held to LAPACK on the CPU);
everything else -- the Gram-Schmidt passes, the fixed-tree sums, the projected matrix, the estimates, the restart product -- is the model's own
arithmetic.  The device is held to it bit for bit: evals, evecs, nconv, status, restarts, spmv_count and max_estimate, for max_restarts = 0, 1, 2 at
tol = 0 and for a solve to tol.

The shapes are those where the kernels can go wrong: packet tails (n = 3, 4, 5), one workgroup's edge (255 .. 257), several workgroups (1023 .. 1025,
4097, 40 001), every size of the column groups (ncv 3, 8, 20, 64: remainders 3, 0, 4, 0 of the input streams; 1 .. 8 output columns and more), and one
size per type just above one trip of the packet loop that ends in a partial packet.  Nothing here reads the reference tree."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
import lanczos_model as LM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-8, np.float32: 1e-4}
SENTINEL = 777.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


class System:
    """one handle with the buffers of its product, and the eigensolver call in the model's terms"""

    def __init__(self, n, rp, ci, va, **options):
        self.n, self.dtype = n, va.dtype.type
        self.H = cvr_amd.CvrMatrix(n, n, rp, ci, va, **options)
        self.tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(self.H.info.x_elems, n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(self.H.info.yext_elems, n, 1), dtype=self.tdt, device="cuda")

    def close(self):
        self.H.close()

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def model(self):
        return LM.LanczosModel(self.product, self.dtype)

    def put(self, a, off=0):
        a = np.ascontiguousarray(a, dtype=self.dtype).reshape(-1)
        t = torch.empty(a.size + off, dtype=self.tdt, device="cuda")[off:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, v0, nev, which, ncv=0, tol=0.0, max_restarts=0, offs=(0, 0), ldv=None, vectors=True, stream=None):
        """cvr_eigsh_device on a start vector of exactly n values and nev columns of ldv values, `offs` values off the allocation's grid, everything
        filled with a sentinel first; returns (EigEntry, EigResult) and checks that nothing outside the returned pairs was written"""
        n = self.n
        ldv = n if ldv is None else ldv
        vt = self.put(v0, offs[0])
        et = torch.full((nev * ldv + offs[1],), SENTINEL, dtype=self.tdt, device="cuda")[offs[1]:]
        evals = np.full(nev, SENTINEL)
        opt, res = self.H._eig_options(nev, "LA" if which == LM.LARGEST else "SA", ncv, tol, max_restarts), capi.EigResult()
        torch.cuda.synchronize()
        rc = capi.lib().cvr_eigsh_device(self.H._h, vt.data_ptr(), evals.ctypes.data, et.data_ptr() if vectors else None, ldv, C.byref(opt), C.byref(res), stream)
        torch.cuda.synchronize()
        assert rc == 0, (rc, cvr_amd.last_error())
        assert vt.cpu().numpy().tobytes() == np.ascontiguousarray(v0, dtype=self.dtype).tobytes(), "v0 was written"
        count = 0 if res.status == LM.BREAKDOWN else res.nconv if res.status == LM.INVARIANT else nev
        E = et.cpu().numpy().reshape(nev, ldv)
        assert (E[:, n:] == SENTINEL).all(), "values beyond n of a column were written"
        assert (E[count:] == SENTINEL).all() and (evals[count:] == SENTINEL).all(), "more than the returned pairs was written"
        if not vectors:
            assert (E == SENTINEL).all()
        return LM.EigEntry(evals[:count], np.ascontiguousarray(E[:count, :n].T), res.nconv, res.status, res.restarts, res.spmv_count, res.max_estimate), res


def _same(got, want, ctx, vectors=True):
    msg = LM.compare(got, want, vectors)
    assert msg == "", (ctx, msg)


def _against_the_model(S, v0, nev, ncv, ctx, ends=(LM.LARGEST, LM.SMALLEST), offs=((0, 0),), ldvs=(None,), cap=8):
    """the bitwise tier for one system and one (nev, ncv): max_restarts = 0, 1, 2 at tol = 0, then the solve to tol (at most `cap` restarts)"""
    for which in ends:
        M = S.model()
        M.run(v0, nev, which, ncv, 0.0, 2)
        for r, entry in enumerate(M.history):
            for o in offs:
                for ldv in ldvs:
                    got, _ = S.solve(v0, nev, which, ncv, 0.0, r, offs=o, ldv=ldv)
                    _same(got, entry, (ctx, which, "max_restarts", r, o, ldv))
        want = S.model().run(v0, nev, which, ncv, TOL[S.dtype], cap)
        got, _ = S.solve(v0, nev, which, ncv, TOL[S.dtype], cap, offs=offs[-1], ldv=ldvs[-1])
        _same(got, want, (ctx, which, "tol"))


PAIRS = {3: [(1, 3)], 4: [(1, 3)], 5: [(1, 3)], 63: [(3, 8), (6, 20)], 64: [(8, 64)], 65: [(3, 8)], 255: [(6, 20)], 256: [(1, 3), (3, 8)], 257: [(8, 64)],
         1023: [(3, 8)], 1024: [(6, 20)], 1025: [(1, 3)], 4097: [(6, 20)], 40001: [(3, 8)]}


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n", sorted(PAIRS))
def test_sizes_against_the_model(n, prec):
    """an indefinite symmetric band; v0 and evecs on and off the 16-byte grid, ldv = n and n + 3"""
    dtype = _dtype(prec)
    _, _, rp, ci, va = LM.band_indefinite(n, dtype)
    S = System(n, rp, ci, va)
    try:
        v0 = LM.start_vector(n, dtype)
        small = n <= 1025
        for nev, ncv in PAIRS[n]:
            _against_the_model(S, v0, nev, ncv, ("size", n, prec, nev, ncv), offs=((0, 0), (1, 1)) if small else ((1, 1),), ldvs=(None, n + 3) if small else (n + 3,),
                               cap=4 if ncv == 64 else 8)
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_second_trip_of_the_packet_loop(prec):
    """ncv = 4, nev = 1, one restart: the restart product's second trip, ending in a partial packet"""
    dtype = _dtype(prec)
    pack = KM.pack_of(dtype)
    n = KM.GRID * pack + pack + 1
    assert KM.trips_of(n, pack) == 2 and n % pack == 1
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    S = System(n, rp, ci, va)
    try:
        v0 = LM.start_vector(n, dtype)
        M = S.model()
        want = M.run(v0, 1, LM.LARGEST, 4, 0.0, 1)
        assert want.restarts == 1 and want.status == LM.MAX_RESTARTS
        got, _ = S.solve(v0, 1, LM.LARGEST, 4, 0.0, 1, offs=(1, 1), ldv=n + 3)
        _same(got, want, ("two trips", prec))
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", ["default", "panels", "gang", "nvec"])
def test_layouts_against_the_model(layout, prec):
    """the vector kernels are the same across layouts; info.x_elems, info.yext_elems and the library's buffers are not"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = LM.band_indefinite(2500, dtype)
    S = System(n, rp, ci, va, **K.ALL_LAYOUTS[layout])
    try:
        _against_the_model(S, LM.start_vector(n, dtype), 3, 8, ("layout", layout, prec), ends=(LM.LARGEST,))
    finally:
        S.close()


def test_stream_mutable_transposed_and_host():
    for dtype in (np.float64, np.float32):
        n, _, rp, ci, va = LM.band_indefinite(301, dtype)
        v0 = LM.start_vector(n, dtype)
        tol = TOL[dtype]
        # a caller's stream; evecs = NULL gives the same evals; two calls give the same bits, another handle used in between
        S = System(n, rp, ci, va)
        other = System(*[LM.laplacian_1d(64, dtype)[i] for i in (0, 2, 3, 4)])
        try:
            want = S.model().run(v0, 3, LM.SMALLEST, 16, tol, 40)
            assert want.status == LM.CONVERGED
            st = torch.cuda.Stream()
            got, res = S.solve(v0, 3, LM.SMALLEST, 16, tol, 40, stream=st.cuda_stream)
            _same(got, want, ("stream", dtype))
            other.solve(LM.start_vector(64, dtype), 2, LM.LARGEST, 6, tol, 3)
            again, _ = S.solve(v0, 3, LM.SMALLEST, 16, tol, 40)
            _same(again, want, ("again", dtype))
            only, _ = S.solve(v0, 3, LM.SMALLEST, 16, tol, 40, vectors=False)
            _same(only, want, ("values only", dtype), vectors=False)
            # the host entry point and the Python methods
            ev, vec, hres = S.H.eigsh_host(3, "SA", 16, tol, v0, 40)
            assert ev.tobytes() == want.evals.tobytes() and np.ascontiguousarray(vec).tobytes() == np.ascontiguousarray(want.evecs).tobytes()
            assert (hres.nconv, hres.status, hres.restarts, hres.spmv_count, hres.max_estimate) == (res.nconv, res.status, res.restarts, res.spmv_count, res.max_estimate)
            ev, vec, _ = S.H.eigsh(3, "SA", 16, tol, S.put(v0), 40)
            assert ev.tobytes() == want.evals.tobytes() and vec.cpu().numpy().tobytes() == np.ascontiguousarray(want.evecs.T).tobytes()
            ev, vec, r = S.H.eigsh(2, "LA", tol=tol, vectors=False)
            assert vec is None and r.status == LM.CONVERGED and len(ev) == 2
        finally:
            S.close()
            other.close()
        # a mutable handle: A, then 2 A -- each solve is the model's on the handle as it is then
        S = System(n, rp, ci, va, mutable_values=1)
        try:
            got, _ = S.solve(v0, 3, LM.LARGEST, 16, tol, 40)
            _same(got, S.model().run(v0, 3, LM.LARGEST, 16, tol, 40), ("mutable", dtype))
            S.H.update_values((2 * va).astype(dtype))
            got2, _ = S.solve(v0, 3, LM.LARGEST, 16, tol, 40)
            _same(got2, S.model().run(v0, 3, LM.LARGEST, 16, tol, 40), ("mutable, updated", dtype))
            assert got2.status == LM.CONVERGED and np.allclose(got2.evals, 2 * got.evals, rtol=1e-3)
        finally:
            S.close()
        # a transpose = 1 handle of the same symmetric matrix
        S = System(n, rp, ci, va, transpose=1)
        try:
            got, _ = S.solve(v0, 3, LM.LARGEST, 16, tol, 40)
            _same(got, S.model().run(v0, 3, LM.LARGEST, 16, tol, 40), ("transposed", dtype))
        finally:
            S.close()


def _diag96(dtype):
    """golden/diag96 as the loader's arrays say, read literally (97 rows, the first one empty): a diagonal with a few entries above it; `alone` are the
    columns that hold their diagonal entry only, so A acts on their span as a diagonal matrix"""
    n, rp, ci, va = LM.diag96(dtype)
    A = LM.dense_of(n, rp, ci, va)
    alone = [j for j in range(n) if np.count_nonzero(A[:, j]) == 1 and A[j, j] != 0]
    return n, rp, ci, va, A.diagonal().copy(), alone


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_closed_spaces_and_breakdowns(prec):
    dtype = _dtype(prec)
    n, rp, ci, va, diag, alone = _diag96(dtype)
    S = System(n, rp, ci, va)
    try:
        # v0 = e_i: the space closes after one step with the exact diagonal entry
        i = alone[11]
        e = np.zeros(n, dtype=dtype)
        e[i] = 1
        got, res = S.solve(e, 1, LM.LARGEST, 3, 1e-8, 5)
        assert (got.status, got.nconv, got.restarts, got.max_estimate) == (LM.CONVERGED, 1, 0, 0.0) and got.evals[0] == diag[i], (got, diag[i])
        assert got.evecs[:, 0].tolist() == e.tolist()
        _same(got, S.model().run(e, 1, LM.LARGEST, 3, 1e-8, 5), ("e_i", prec))
        # v0 supported on 3 entries with distinct diagonal values, nev = 4: the space closes with 3 columns
        idx = [alone[0], alone[len(alone) // 2], alone[-1]]
        assert len({diag[k] for k in idx}) == 3
        v = np.zeros(n, dtype=dtype)
        v[idx] = (1.0, 2.0, -1.5)
        want = S.model().run(v, 4, LM.SMALLEST, 6, 1e-8, 5)
        got, res = S.solve(v, 4, LM.SMALLEST, 6, 1e-8, 5)
        assert (got.status, got.nconv, got.restarts) == (LM.INVARIANT, 3, 0) and np.allclose(got.evals, np.sort(diag[idx]), rtol=1e-6 if dtype == np.float32 else 1e-13, atol=0), got
        _same(got, want, ("three entries", prec))
        # v0 = 0 and a NaN in v0: breakdown, nothing written (solve() checks the sentinels)
        for bad in (np.zeros(n, dtype=dtype), np.where(np.arange(n) == 5, np.nan, 1.0).astype(dtype)):
            got, res = S.solve(bad, 2, LM.LARGEST, 6, 1e-8, 5)
            assert (got.status, got.nconv, len(got.evals), got.evecs.shape) == (LM.BREAKDOWN, 0, 0, (n, 0)), got
            want = S.model().run(bad, 2, LM.LARGEST, 6, 1e-8, 5)
            assert (want.status, want.spmv_count, want.restarts) == (got.status, got.spmv_count, got.restarts)
    finally:
        S.close()
    # a NaN among A's values
    vn = va.copy()
    vn[rp[40]] = np.nan
    S = System(n, rp, ci, vn)
    try:
        got, res = S.solve(np.ones(n, dtype=dtype), 2, LM.LARGEST, 6, 1e-8, 5)
        assert (got.status, got.nconv, len(got.evals)) == (LM.BREAKDOWN, 0, 0), got
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_laplacian_end_to_end(prec):
    """n = 1025, both ends, nev = 4: the closed form within the bound of tests/test_lanczos_model_host.py (residual_allowance)"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = LM.laplacian_1d(1025, dtype)
    exact = LM.laplacian_eigs(n)
    S = System(n, rp, ci, va)
    try:
        for which, ref in ((LM.LARGEST, exact[-4:]), (LM.SMALLEST, exact[:4])):
            ev, vec, res = S.H.eigsh(4, "LA" if which == LM.LARGEST else "SA", ncv=32, tol=TOL[dtype], v0=S.put(LM.start_vector(n, dtype)), max_restarts=400)
            assert res.status == LM.CONVERGED and res.nconv == 4, (res.status, res.nconv, res.restarts)
            bound = TOL[dtype] * np.maximum(LM.EPS23, np.abs(ev)) + LM.residual_allowance(dtype, 4.0)
            print(f"laplacian 1025 {prec} which={which}: restarts {res.restarts}, steps {res.spmv_count}, max error {np.abs(ev - ref).max():.3g}, bound {bound.min():.3g}")
            assert (np.abs(ev - ref) <= bound).all(), (ev, ref, bound)
    finally:
        S.close()


def test_errors_with_a_real_handle():
    dtype = np.float64
    n, _, rp, ci, va = LM.band_indefinite(44, dtype)
    L = capi.lib()
    opt, res = capi.EigOptions(), capi.EigResult()
    L.cvr_eig_default_options(C.byref(opt))
    vt = torch.ones(n + 8, dtype=torch.float64, device="cuda")
    et = torch.zeros(4 * n + 8, dtype=torch.float64, device="cuda")
    ev = np.zeros(8)
    torch.cuda.synchronize()
    # before cvr_preprocess
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    assert L.cvr_eigsh_device(h, vt.data_ptr(), ev.ctypes.data, None, 0, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hv = np.ones(n)
    assert L.cvr_eigsh(h, hv.ctypes.data, ev.ctypes.data, None, 0, C.byref(opt), C.byref(res)) == capi.ERR_STATE
    L.cvr_destroy(h)
    # a matrix that is not square
    R = cvr_amd.CvrMatrix(n - 1, n, rp[:n], ci[: rp[n - 1]], va[: rp[n - 1]])
    try:
        assert L.cvr_eigsh_device(R._h, vt.data_ptr(), ev.ctypes.data, None, 0, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "square" in cvr_amd.last_error()
    finally:
        R.close()
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        opt.ncv = 50          # > n
        assert L.cvr_eigsh_device(A._h, vt.data_ptr(), ev.ctypes.data, None, 0, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "ncv" in cvr_amd.last_error()
        opt.ncv = 0
        assert L.cvr_eigsh_device(A._h, vt.data_ptr(), ev.ctypes.data, et.data_ptr(), n - 1, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "ldv" in cvr_amd.last_error()
    finally:
        A.close()
    assert not et.cpu().numpy().any()
