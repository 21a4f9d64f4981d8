"""GPU (MI355X): cvr_lobpcg_device / cvr_lobpcg against numpy.linalg.eigvalsh and against the numpy model of include/cvr_amd.h (tests/lobpcg_model.py;
tests/test_lobpcg_model_host.py shows on the CPU that the model finds the lowest pairs within its bounds and that its checks reject three wrong
recurrences).  The model's product is the handle's own cvr_spmv_device and its apply the object's own cvr_precond_apply_device; everything else --
the residuals, the two Gram-Schmidt passes, the fixed-tree sums of G and H, the Cholesky and Rayleigh-Ritz loops, the combination -- is the model's
own arithmetic, in the kernels' summation order.

The shapes are those where the kernels can go wrong: n = 3k exactly, packet tails and one workgroup's edge (63, 64, 65, 257), several workgroups
(1025, 4097), one size past one grid pass of packets (524 291 values in fp64, 1 048 581 in fp32), k = 1, 3, 4, 8 (the compile-time block extents 1, 4,
4, 8; k = 2 rides in the layout test), and the two Laplacians of the issue.
The fp32 tolerance of a case is the smallest power of ten the model reaches in fp32 on it on the CPU with every one of three products, the fused
multiply-add row sums of an fp32 SpMV among them (lobpcg_model.fp32_tolerance, recorded in lobpcg_model.FP32_TOL and held on the CPU by
tests/test_lobpcg_model_host.py), not a figure taken from a device run.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch

import cvr_amd
import krylov_model as KM
import lobpcg_model as LM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
UNIT = {np.float64: 1e-12, np.float32: 1e-5}          # the parity tests' allowance of one product (TOL64, TOL32 of test_gpu_parity.py)
MAX_ITERS = 1500

FP32_TOL = LM.FP32_TOL          # (matrix, k): fp32 tolerance


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _matrix(name, dtype):
    if name == "lap24":
        return LM.laplacian_grid(24, 24, dtype)
    if name == "lap40x12":
        return LM.laplacian_grid(40, 12, dtype)
    if name == "lap40":
        return LM.laplacian_grid(40, 40, dtype)
    return LM.banded(int(name[4:]), dtype)


_REF = {}


def _reference(name, dtype):
    """(dense A of the matrix rounded to T, |A|, eigvalsh of it), computed once per case"""
    key = (name, np.dtype(dtype).name)
    if key not in _REF:
        n, _, rp, ci, va = _matrix(name, dtype)
        A = LM.dense_of(n, rp, ci, va)
        _REF[key] = (A, np.abs(A), np.linalg.eigvalsh(A))
    return _REF[key]


class System:
    """one handle with the buffers of its product, and the solver call in the model's terms"""

    def __init__(self, name, dtype, **options):
        self.name, self.dtype = name, dtype
        self.n, _, self.rp, self.ci, self.va = _matrix(name, dtype)
        self.H = cvr_amd.CvrMatrix(self.n, self.n, self.rp, self.ci, self.va, **options)
        self.tdt = torch.float64 if dtype == np.float64 else torch.float32
        n = self.n
        self.xbuf = torch.zeros(max(self.H.info.x_elems, n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(self.H.info.yext_elems, n, 1), dtype=self.tdt, device="cuda")
        self.rbuf = torch.zeros(n, dtype=self.tdt, device="cuda")
        self.zbuf = torch.zeros(n, dtype=self.tdt, device="cuda")
        self.pc = {}

    def close(self):
        for p in self.pc.values():
            p.close()
        self.H.close()

    def precond(self, kind):
        if kind not in self.pc:
            P, a = capi.Precond, (self.rp, self.ci, self.va)
            if kind == "chebyshev":
                lo, hi = self.H.chebyshev_bounds()
                self.pc[kind] = P.chebyshev(self.H, 4, lo, hi)
            else:
                make = {"jacobi1": lambda: P.block_jacobi(*a, 1), "jacobi8": lambda: P.block_jacobi(*a, 8), "ilu0": lambda: P.ilu0(*a), "fsai": lambda: P.fsai(*a),
                        "amg": lambda: P.amg(self.H, *a), "amg_smoothed": lambda: P.amg_smoothed(self.H, *a), "amg_mis2": lambda: P.amg_mis2(self.H, *a),
                        "mcsgs": lambda: P.mcsgs(*a)}
                self.pc[kind] = make[kind]()
        return self.pc[kind]

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def apply_of(self, kind):
        if kind is None:
            return None
        pc = self.precond(kind)

        def apply(r):
            self.rbuf.copy_(torch.from_numpy(np.ascontiguousarray(r, dtype=self.dtype)))
            torch.cuda.synchronize()
            pc.apply(self.rbuf.data_ptr(), self.zbuf.data_ptr())
            torch.cuda.synchronize()
            return self.zbuf.cpu().numpy()
        return apply

    def model(self, kind=None):
        return LM.LobpcgModel(self.product, self.dtype, self.apply_of(kind))

    def solve(self, X0, kind=None, which=LM.SMALLEST, tol=1e-8, max_iters=MAX_ITERS, off=0, ldx=None, expect=0):
        """cvr_lobpcg_device on a block of k columns of ldx values, `off` values off the allocation's grid, the padding filled with a sentinel; returns
        (BlockEntry, LobpcgResult) and checks that nothing but the n values of each column was written"""
        n, k = X0.shape
        ldx = n if ldx is None else ldx
        host = np.full((k, ldx), SENTINEL, dtype=self.dtype)
        host[:, :n] = X0.T
        xt = torch.empty(k * ldx + off, dtype=self.tdt, device="cuda")[off:]
        xt.copy_(torch.from_numpy(host.reshape(-1)))
        evals, resn = np.full(k, SENTINEL), np.full(k, SENTINEL)
        opt, res = self.H._lobpcg_options(k, "LA" if which == LM.LARGEST else "SA", tol, max_iters), capi.LobpcgResult()
        torch.cuda.synchronize()
        rc = capi.lib().cvr_lobpcg_device(self.H._h, None if kind is None else self.precond(kind)._p, xt.data_ptr(), ldx, evals.ctypes.data, resn.ctypes.data,
                                          C.byref(opt), C.byref(res), None)
        torch.cuda.synchronize()
        assert rc == expect, (rc, cvr_amd.last_error())
        out = xt.cpu().numpy().reshape(k, ldx)
        assert (out[:, n:] == SENTINEL).all(), "values beyond n of a column were written"
        if rc or res.status == LM.BREAKDOWN:
            assert out.tobytes() == host.tobytes() and (evals == SENTINEL).all() and (resn == SENTINEL).all(), "written behind a breakdown or an error"
            return LM.BlockEntry([], [], X0, 0, res.status, res.iterations, res.spmv_count, res.precond_applies, res.restarts_without_p, 0.0), res
        return LM.BlockEntry(evals, resn, np.ascontiguousarray(out[:, :n].T), res.nconv, res.status, res.iterations, res.spmv_count, res.precond_applies,
                             res.restarts_without_p, res.max_rel_residual), res


def _check_pairs(S, e, k, which=LM.SMALLEST):
    """the eigenvalues against eigvalsh within the reported residual plus one product's allowance, and the residual recomputed in fp64"""
    A, absA, lam = _reference(S.name, S.dtype)
    ref = lam[:k] if which == LM.SMALLEST else lam[-k:]
    X = e.X.astype(np.float64)
    allow = LM.residual_allowance(absA, X, UNIT[S.dtype])
    err, true = np.abs(e.evals - ref), np.linalg.norm(A @ X - X * e.evals, axis=0)
    print(f"{S.name} k={k} {np.dtype(S.dtype).name}: {e.iterations} iterations, {e.restarts_without_p} without P; max (|theta - lambda| - resnorm) / allowance "
          f"{((err - e.resnorms) / allow).max():.3g}; max (recomputed - resnorm) / allowance {((true - e.resnorms) / allow).max():.3g}")
    assert (err <= e.resnorms + allow).all(), (S.name, k, err, e.resnorms, allow)
    assert (true <= e.resnorms + allow).all(), (S.name, k, true, e.resnorms, allow)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name,k", sorted(FP32_TOL))
def test_eigenvalues_and_residuals(name, k, prec):
    dtype = _dtype(prec)
    S = System(name, dtype)
    try:
        e, res = S.solve(LM.start_block(S.n, k, dtype), tol=1e-8 if dtype == np.float64 else FP32_TOL[(name, k)])
        assert e.status == LM.CONVERGED and e.nconv == k, e
        assert res.spmv_count == k * (2 + res.iterations) and res.precond_applies == 0
        _check_pairs(S, e, k)
    finally:
        S.close()


def _against_the_model(S, X0, kind, ctx, which=LM.SMALLEST, tol=None, max_iters=MAX_ITERS):
    """bit for bit: the model forms every sum in the kernels' order (krylov_model.tree_sum) and the Rayleigh-Ritz step in the header's order, so the
    issue's fallback (iterations within 1, theta within 4 eps |theta| iterations) is tightened to equality of X, evals, resnorms and every count"""
    tol = (1e-8 if S.dtype == np.float64 else 1e-5) if tol is None else tol
    want = S.model(kind).run(X0, which, tol, max_iters)
    got, _ = S.solve(X0, kind, which, tol, max_iters)
    diff = LM.compare(got, want)
    print(f"{ctx}: device {got.iterations} iterations, model {want.iterations}; bit for bit: {'yes' if diff == '' else 'NO: ' + diff[:200]}")
    assert diff == "", (ctx, diff)
    return got, want, diff


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name,k,kind", [("lap24", 4, None), ("lap24", 4, "jacobi8"), ("lap40x12", 3, "fsai"), ("band65", 4, None), ("band257", 8, None),
                                         ("band1025", 1, None), ("band4097", 1, "jacobi1")])
def test_against_the_model(name, k, kind, prec):
    dtype = _dtype(prec)
    S = System(name, dtype)
    try:
        X0 = LM.start_block(S.n, k, dtype)
        # a few iterations (the state at MAX_ITERS is the sharpest comparison: nothing has converged away), then the solve to tol
        _against_the_model(S, X0, kind, (name, k, kind, prec, "5 iterations"), max_iters=5)
        got, _, _ = _against_the_model(S, X0, kind, (name, k, kind, prec, "to tol"))
        assert got.status == LM.CONVERGED
    finally:
        S.close()


SHAPES = ("lap24", "lap40x12", "band63", "band64", "band65", "band257", "band1025", "band4097")


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SHAPES)
def test_every_shape_with_every_k_against_the_model(name, prec):
    """k = 1, 3, 4, 8 on every shape for 5 iterations, bit for bit: this needs no convergence, so it also holds the pairs that
    test_eigenvalues_and_residuals leaves out because the band's dense lower end takes the model thousands of iterations there"""
    dtype = _dtype(prec)
    S = System(name, dtype)
    try:
        for k in (1, 3, 4, 8):
            _against_the_model(S, LM.start_block(S.n, k, dtype), None, (name, k, prec, "5 iterations"), max_iters=5)
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("k", [1, 3])
def test_second_trip_of_the_packet_loop(k, prec):
    """n = one grid pass of packets, one packet and one value more: every kernel's packet loop goes round twice for the first threads and ends in a
    partial packet; the sums of the residual, update, Gram and combine kernels span the trips.  2 iterations (m = k, 2k, 3k), X on the
    16-byte grid and one value off it with ldx > n, bit for bit against the model"""
    dtype = _dtype(prec)
    pack = KM.pack_of(dtype)
    n = KM.GRID * pack + pack + 1
    assert KM.trips_of(n, pack) == 2 and n % pack == 1
    S = System(f"band{n}", dtype)
    try:
        X0 = LM.start_block(n, k, dtype)
        want = S.model().run(X0, LM.SMALLEST, 0.0, 2)
        assert (want.status, want.iterations, want.spmv_count, want.restarts_without_p) == (LM.MAX_ITERS, 2, 3 * k, 0)
        for off, ldx in ((0, None), (1, n + 3)):
            got, _ = S.solve(X0, tol=0.0, max_iters=2, off=off, ldx=ldx)
            diff = LM.compare(got, want)
            assert diff == "", (k, prec, off, ldx, diff)
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_n_equal_3k_and_too_small(prec):
    dtype = _dtype(prec)
    for k in (1, 3, 8):
        n = 3 * k
        S = System(f"band{n}", dtype)
        try:
            X0 = LM.start_block(n, k, dtype)
            got, want, _ = _against_the_model(S, X0, None, ("n = 3k", k, prec), max_iters=60)
            if got.status == LM.CONVERGED:
                _check_pairs(S, got, k)
            if k < 8:          # one column more: n < 3 nev
                S.solve(LM.start_block(n, k + 1, dtype), expect=capi.ERR_INVALID)
                assert "3 * nev" in cvr_amd.last_error()
        finally:
            S.close()
    # n = 1 with k = 1
    A = cvr_amd.CvrMatrix(1, 1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([2.0], dtype=dtype))
    try:
        x = torch.ones(4, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        ev, rn = np.zeros(1), np.zeros(1)
        opt, res = A._lobpcg_options(1, "SA", 1e-8, 10), capi.LobpcgResult()
        torch.cuda.synchronize()
        assert capi.lib().cvr_lobpcg_device(A._h, None, x.data_ptr(), 1, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "3 * nev" in cvr_amd.last_error()
    finally:
        A.close()


@pytest.mark.parametrize("kind", ["jacobi1", "jacobi8", "chebyshev", "ilu0", "fsai", "amg", "amg_smoothed", "amg_mis2", "mcsgs"])
def test_every_kind_is_taken(kind):
    S = System("lap24", np.float64)
    try:
        e, res = S.solve(LM.start_block(S.n, 4, np.float64), kind)
        print(f"{kind}: {e.iterations} iterations, {res.precond_applies} applies")
        assert e.status == LM.CONVERGED and res.precond_applies == 4 * (1 + res.iterations), e
        _check_pairs(S, e, 4)
    finally:
        S.close()


def test_the_preconditioner_pays():
    """the 40 x 40 Laplacian, k = 4: fewer iterations with amg_mis2 than without an object.  The model, run here with the device's product and apply
    as callables, says which assertion holds: twice fewer where it shows a threefold gap, strictly fewer otherwise."""
    S = System("lap40", np.float64)
    try:
        X0 = LM.start_block(S.n, 4, np.float64)
        m_amg, m_none = S.model("amg_mis2").run(X0, LM.SMALLEST, 1e-8, MAX_ITERS), S.model(None).run(X0, LM.SMALLEST, 1e-8, MAX_ITERS)
        d_amg, _ = S.solve(X0, "amg_mis2")
        d_none, _ = S.solve(X0, None)
        print(f"40 x 40 Laplacian, k = 4: model {m_amg.iterations} with amg_mis2, {m_none.iterations} without; device {d_amg.iterations}, {d_none.iterations}")
        assert m_amg.status == m_none.status == d_amg.status == d_none.status == LM.CONVERGED
        if m_none.iterations >= 3 * m_amg.iterations:
            assert d_amg.iterations * 2 <= d_none.iterations
        else:
            assert d_amg.iterations < d_none.iterations
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_determinism_and_layout(prec):
    dtype = _dtype(prec)
    S = System("band257", dtype)
    try:
        X0 = LM.start_block(S.n, 2, dtype)
        tol = 1e-8 if dtype == np.float64 else 1e-5
        a, _ = S.solve(X0, tol=tol)
        assert a.status == LM.CONVERGED
        for off, ldx in ((0, None), (1, None), (0, S.n + 3), (1, S.n + 5)):          # again; an unaligned base; ldx > n (solve checks the padding)
            b, _ = S.solve(X0, tol=tol, off=off, ldx=ldx)
            assert LM.compare(b, a) == "", (off, ldx)
        # max_iters = 0: the Rayleigh-Ritz of the start block
        z, res = S.solve(X0, tol=tol, max_iters=0)
        assert (z.status, z.iterations, res.spmv_count) == (LM.MAX_ITERS, 0, 2)
        A, _, _ = _reference("band257", dtype)
        Q, _ = np.linalg.qr(X0.astype(np.float64))
        assert np.allclose(z.evals, np.linalg.eigvalsh(Q.T @ A @ Q), rtol=1e-5 if dtype == np.float32 else 1e-12, atol=0)
        assert LM.compare(z, S.model().run(X0, LM.SMALLEST, tol, 0)) == ""
        # the host entry point and the Python methods
        ev, X, rn, hres = S.H.lobpcg_host(X0, tol=tol, max_iters=MAX_ITERS)
        assert ev.tobytes() == a.evals.tobytes() and rn.tobytes() == a.resnorms.tobytes() and np.ascontiguousarray(X).tobytes() == np.ascontiguousarray(a.X).tobytes()
        xt = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda()
        ev, rn, _ = S.H.lobpcg(xt, tol=tol, max_iters=MAX_ITERS)
        assert ev.tobytes() == a.evals.tobytes() and xt.cpu().numpy().tobytes() == np.ascontiguousarray(a.X.T).tobytes()
    finally:
        S.close()


def test_the_largest_end():
    S = System("lap24", np.float64)
    try:
        X0 = LM.start_block(S.n, 4, np.float64)
        e, _ = S.solve(X0, which=LM.LARGEST)
        assert e.status == LM.CONVERGED and (np.diff(e.evals) >= 0).all()
        _check_pairs(S, e, 4, LM.LARGEST)
        S.solve(X0, "jacobi1", which=LM.LARGEST, expect=capi.ERR_INVALID)
        assert "CVR_EIG_LARGEST" in cvr_amd.last_error()
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_a_nan_in_the_start_block(prec):
    """a status code, nothing written (solve checks X, evals and resnorms against their sentinels)"""
    dtype = _dtype(prec)
    S = System("band65", dtype)
    try:
        X0 = LM.start_block(S.n, 3, dtype)
        X0[7, 1] = np.nan
        for kind in (None, "jacobi8"):
            e, res = S.solve(X0, kind)
            assert (e.status, res.nconv, res.iterations) == (LM.BREAKDOWN, 0, 0), (kind, e)
    finally:
        S.close()


def test_errors_with_a_real_handle():
    dtype = np.float64
    n, _, rp, ci, va = LM.banded(44, dtype)
    L = capi.lib()
    opt, res = capi.LobpcgOptions(), capi.LobpcgResult()
    L.cvr_lobpcg_default_options(C.byref(opt))
    opt.nev = 2
    xt = torch.ones(2 * n + 8, dtype=torch.float64, device="cuda")
    ev, rn, hx = np.zeros(8), np.zeros(8), np.ones(2 * n)
    torch.cuda.synchronize()
    # before cvr_preprocess
    view = capi.CsrView(n, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0)
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    assert L.cvr_lobpcg_device(h, None, xt.data_ptr(), n, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    assert L.cvr_lobpcg(h, None, hx.ctypes.data, n, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res)) == capi.ERR_STATE
    L.cvr_destroy(h)
    # a matrix that is not square
    R = cvr_amd.CvrMatrix(n - 1, n, rp[:n], ci[: rp[n - 1]], va[: rp[n - 1]])
    try:
        assert L.cvr_lobpcg_device(R._h, None, xt.data_ptr(), n, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "square" in cvr_amd.last_error()
    finally:
        R.close()
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    m2, _, rp2, ci2, va2 = LM.banded(45, dtype)
    other = capi.Precond.block_jacobi(rp2, ci2, va2, 1)
    f32 = capi.Precond.block_jacobi(rp, ci, va.astype(np.float32), 1)
    try:
        assert L.cvr_lobpcg_device(A._h, None, xt.data_ptr(), n - 1, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "ldx" in cvr_amd.last_error()
        assert L.cvr_lobpcg_device(A._h, other._p, xt.data_ptr(), n, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "the preconditioner has n = 45" in cvr_amd.last_error()
        assert L.cvr_lobpcg_device(A._h, f32._p, xt.data_ptr(), n, ev.ctypes.data, rn.ctypes.data, C.byref(opt), C.byref(res), None) == capi.ERR_INVALID
        assert "fp32" in cvr_amd.last_error()
    finally:
        other.close()
        f32.close()
        A.close()
    assert (xt.cpu().numpy() == 1).all() and not ev.any() and not rn.any()
