"""GPU (MI355X): the block-Jacobi object with several right-hand sides -- cvr_precond_apply_multi_device, cvr_pcg_multi_device, cvr_pcg_multi, all
through the ABI.

The reference is the code that was there before, run column by column on the same handle and object: cvr_precond_apply_device for the apply,
cvr_pcg_device for the solver (and cvr_cg_multi_device with the exported diagonal for block_size = 1).  Everything is compared bit for bit.  The
handles are made with nvec = 8 (the plain layout, which the k-wide product needs); the padding columns of every block hold a sentinel that must come
back with the same bits, and R and B must come back unwritten.

  * the apply: n = 1, 3, 5, 515 x block sizes 1, 3, 8, 32 x nvec 1, 2, 3, 5, 8, both leading-dimension pairs, both offsets, fp64 and fp32 (a partial
    packet alone; a block across packets, threads and workgroups; short last blocks; n < bs), and the second trip ending in a partial packet with a
    -0.0 and a NaN that stays in its block and its column
  * the solver: every nvec, leading dimension, offset and check_every, fp64 and fp32, the host twin, spmv_count; block_size = 1
  * columns that stop at different steps, in two orders; a NaN and an Inf in b; -A
  * what it is for: a block-diagonal system with 8 right-hand sides within 2 steps
  * the neighbours: the single-vector path on a default handle, the error returns with real objects, one object for two handles, no state left"""
import numpy as np
import pytest

import cvr_amd
import krylov_model as KM
import oraclelib as O
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 60
SENTINEL = -777.25          # (exact in fp32 and fp64) what stands in the padding columns
LDS = (lambda k: (k, k), lambda k: (k + 3, k + 1))


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _dev(a, dtype, shift=0):
    """a device copy of `a` (any shape) of exactly its size, `shift` elements off the allocation's start"""
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.empty(a.size + shift, dtype=_tdt(dtype), device="cuda")[shift:]
    t.copy_(torch.from_numpy(a.reshape(-1)))
    return t


def _padded(A, ld, dtype):
    n, k = A.shape
    h = np.full((n, ld), SENTINEL, dtype=dtype)
    h[:, :k] = A
    return h


# ---- the apply ----
def _apply_single(P, r):
    rt, zt = _dev(r, P.dtype), _dev(np.full(len(r), SENTINEL), P.dtype)
    torch.cuda.synchronize()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    return zt.cpu().numpy()


def _apply_multi(P, R, ldr, ldz, shift=0):
    """cvr_precond_apply_multi_device on blocks of exactly n rows whose padding columns (and all of Z) hold SENTINEL; checks R and the padding of Z"""
    n, nvec = R.shape
    hr, hz = _padded(R, ldr, P.dtype), np.full((n, ldz), SENTINEL, dtype=P.dtype)
    rt, zt = _dev(hr, P.dtype, shift), _dev(hz, P.dtype, shift)
    torch.cuda.synchronize()
    P.apply_multi(rt.data_ptr(), ldr, zt.data_ptr(), ldz, nvec)
    torch.cuda.synchronize()
    assert _bits_equal(rt.cpu().numpy().reshape(n, ldr), hr), "R was written"
    Z = zt.cpu().numpy().reshape(n, ldz)
    assert _bits_equal(Z[:, nvec:], hz[:, nvec:]), "the padding columns of Z were written"
    return np.ascontiguousarray(Z[:, :nvec])


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("bs", [1, 3, 8, 32])
def test_apply_is_the_single_apply_column_by_column(bs, prec):
    dtype = _dtype(prec)
    for n in (1, 3, 5, 515):
        _, _, rp, ci, va = KM.banded("spd", n, dtype)
        P = capi.Precond.block_jacobi(rp, ci, va, bs)
        try:
            R = np.random.default_rng(n * 100 + bs).standard_normal((n, 8)).astype(dtype)
            R[n // 2, 1] = -0.0
            refs = [_apply_single(P, R[:, c]) for c in range(8)]
            for nvec in (1, 2, 3, 5, 8):
                for ld in LDS:
                    ldr, ldz = ld(nvec)
                    for shift in (0, 1):
                        Z = _apply_multi(P, R[:, :nvec], ldr, ldz, shift)
                        for c in range(nvec):
                            assert _bits_equal(Z[:, c], refs[c]), (prec, n, bs, nvec, ldr, ldz, shift, c, int(np.sum(Z[:, c] != refs[c])))
        finally:
            P.close()


def _banded_spd(n, dtype, half_band=2):
    n, _, rp, ci, _ = synth.banded_sym(n, half_band=half_band)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


def test_apply_second_trip_ending_in_a_partial_packet():
    """every thread's first trip, then the second trip ending in a partial packet; a -0.0, and a NaN that stays in its own block and column"""
    n, bs, nvec, dtype = 1024 * 256 * 2 + 3, 8, 2, np.float64
    _, _, rp, ci, va = _banded_spd(n, dtype)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        R = np.random.default_rng(5).standard_normal((n, nvec))
        R[7, 0] = -0.0
        at = n - 2          # in the short last block (rows n - 3 .. n - 1)
        R[at, 1] = np.nan
        refs = [_apply_single(P, R[:, c]) for c in range(nvec)]
        for ld, shift in ((LDS[0], 0), (LDS[1], 1)):
            ldr, ldz = ld(nvec)
            Z = _apply_multi(P, R, ldr, ldz, shift)
            for c in range(nvec):
                assert _bits_equal(Z[:, c], refs[c]), (ldr, ldz, shift, c)
            assert not np.isnan(Z[:, 0]).any()
            bad = np.flatnonzero(np.isnan(Z[:, 1]))
            assert len(bad) and (bad // bs == at // bs).all(), bad
    finally:
        P.close()


# ---- the solver ----
def _single(H, P, b, x0=None, **kw):
    """cvr_pcg_device on arrays of exactly nrows values; (x, result)"""
    bt, xt = _dev(b, H.dtype), _dev(np.zeros(H.nrows) if x0 is None else x0, H.dtype)
    torch.cuda.synchronize()
    res = H.pcg(P, bt.data_ptr(), xt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), res


def _multi(H, P, B, X0=None, ldb=None, ldx=None, shift=0, minv=None, **kw):
    """cvr_pcg_multi_device (P a Precond) or cvr_cg_multi_device (P None, minv an array) on blocks of exactly nrows rows whose padding columns hold
    SENTINEL; checks that B and the padding of X come back with the same bits; (X, results)"""
    n, nvec = B.shape
    ldb, ldx = ldb or nvec, ldx or nvec
    hb, hx = _padded(B, ldb, H.dtype), _padded(np.zeros((n, nvec)) if X0 is None else X0, ldx, H.dtype)
    bt, xt = _dev(hb, H.dtype, shift), _dev(hx, H.dtype, shift)
    mt = None if minv is None else _dev(minv, H.dtype)
    torch.cuda.synchronize()
    if P is not None:
        res = H.pcg_multi(P, bt.data_ptr(), ldb, xt.data_ptr(), ldx, nvec, **kw)
    else:
        res = H.cg_multi(bt.data_ptr(), ldb, xt.data_ptr(), ldx, nvec, minv_ptr=mt.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert len(res) == nvec
    assert _bits_equal(bt.cpu().numpy().reshape(n, ldb), hb), "B was written"
    X = xt.cpu().numpy().reshape(n, ldx)
    assert _bits_equal(X[:, nvec:], hx[:, nvec:]), "the padding columns of X were written"
    return np.ascontiguousarray(X[:, :nvec]), res


def _same_result(r, ref, ctx):
    assert (r.iterations, r.status) == (ref.iterations, ref.status), (ctx, r.iterations, r.status, ref.iterations, ref.status)
    assert np.float64(r.residual_norm).tobytes() == np.float64(ref.residual_norm).tobytes(), (ctx, r.residual_norm, ref.residual_norm)
    assert np.float64(r.b_norm).tobytes() == np.float64(ref.b_norm).tobytes(), (ctx, r.b_norm, ref.b_norm)


def _assert_columns(X, res, refs, ctx):
    """column j of the block solve against the single solve refs[j] = (x, result)"""
    for j, (xr, rr) in enumerate(refs):
        _same_result(res[j], rr, (ctx, j))
        assert _bits_equal(X[:, j], xr), (ctx, j, "x differs", int(np.sum(X[:, j] != xr)))
    assert len({r.spmv_count for r in res}) == 1 and len({r.seconds for r in res}) == 1


def _block(n, dtype, k=8, seed=11):
    """k right-hand sides and start vectors: x_rand and seeded normals from a zero start, every third from a random start"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    B[:, 0] = synth.x_rand(n)
    X0 = np.zeros((n, k))
    X0[:, 2::3] = rng.random((n, len(range(2, k, 3)))) * 2 - 1
    return B.astype(dtype), X0.astype(dtype)


class System:
    """a banded SPD matrix, its nvec = 8 handle and its block-Jacobi object"""

    def __init__(self, n, bs, dtype, options=None):
        self.n, self.bs, self.dtype = n, bs, dtype
        _, _, self.rp, self.ci, self.va = KM.banded("spd", n, dtype)
        self.H = cvr_amd.CvrMatrix(n, n, self.rp, self.ci, self.va, **(dict(nvec=8) if options is None else options))
        self.P = capi.Precond.block_jacobi(self.rp, self.ci, self.va, bs)

    def close(self):
        self.P.close()
        self.H.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", [(250, 3), (1000, 8), (4099, 32)])
def test_bit_for_bit_against_the_single_solver(n, bs, prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    S = System(n, bs, dtype)
    try:
        H, P = S.H, S.P
        assert H.spmm_supported
        B, X0 = _block(n, dtype)
        refs = [_single(H, P, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(8)]
        assert all(r.status == capi.CG_CONVERGED and r.iterations > 0 for _, r in refs)
        for nvec in (1, 2, 3, 5, 8):
            for ld in LDS:
                ldb, ldx = ld(nvec)
                for shift in (0, 1):
                    counts = []
                    for every in (1, 3, MAX_ITERS):
                        X, res = _multi(H, P, B[:, :nvec], X0[:, :nvec], ldb=ldb, ldx=ldx, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                        _assert_columns(X, res, refs[:nvec], (n, bs, prec, nvec, ldb, ldx, shift, every))
                        counts.append(res[0].spmv_count)
                    # read back after every step, nothing is enqueued behind the last column's stop; with one read-back, everything is
                    assert counts[0] == max(r.iterations for _, r in refs[:nvec]) + 1 and counts == sorted(counts) and counts[-1] == MAX_ITERS + 1
            Xh, rh = H.pcg_multi_host(P, B[:, :nvec], X0[:, :nvec], rtol=rtol, max_iters=MAX_ITERS)          # the host twin
            _assert_columns(Xh, rh, refs[:nvec], (n, bs, prec, nvec, "host"))
        # below the stop: max_iters steps in every column
        refs2 = [_single(H, P, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=2) for j in range(5)]
        X, res = _multi(H, P, B[:, :5], X0[:, :5], ldb=6, ldx=8, rtol=rtol, max_iters=2)
        _assert_columns(X, res, refs2, "max_iters 2")
        X, res = _multi(H, P, B[:, :5], X0[:, :5], rtol=rtol, max_iters=0)
        assert _bits_equal(X, X0[:, :5]) and all((r.spmv_count, r.iterations, r.status) == (1, 0, capi.CG_MAX_ITERS) for r in res)
    finally:
        S.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_block_size_one_is_cg_multi_with_the_exported_diagonal(prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    S = System(1000, 1, dtype)
    try:
        W = S.P.export()
        assert W.shape == (S.n, 1, 1) and S.P.info.identity_blocks == 0
        B, X0 = _block(S.n, dtype)
        for nvec, ldb, ldx, shift, every in ((8, 8, 8, 0, 0), (5, 8, 6, 1, 1), (1, 1, 1, 0, 3)):
            kw = dict(ldb=ldb, ldx=ldx, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            Xr, rr = _multi(S.H, None, B[:, :nvec], X0[:, :nvec], minv=W.reshape(-1), **kw)
            X, res = _multi(S.H, S.P, B[:, :nvec], X0[:, :nvec], **kw)
            assert _bits_equal(X, Xr), (prec, nvec)
            for j in range(nvec):
                _same_result(res[j], rr[j], (prec, nvec, j))
            assert all(r.status == capi.CG_CONVERGED and r.iterations > 0 for r in res)
    finally:
        S.close()


def test_columns_that_stop_at_different_steps_and_isolation():
    """a late column must not freeze with an early one, an early or a bad column must not leak into the others"""
    dtype, rtol = np.float64, 1e-10
    S = System(1000, 8, dtype)
    try:
        H, P, n = S.H, S.P, S.n
        b = synth.x_rand(n)
        sol = {t: _single(H, P, b, rtol=t, max_iters=MAX_ITERS)[0] for t in (1e-4, 1e-7, 1e-10)}
        rng = np.random.default_rng(3)
        start = rng.random(n) * 2 - 1
        bnan, binf = rng.standard_normal(n), rng.standard_normal(n)
        bnan[n // 3] = np.nan
        binf[n - 1] = np.inf
        B = np.stack([np.zeros(n), b, b, b, bnan, binf, b, rng.standard_normal(n)], axis=1)
        X0 = np.stack([start, sol[1e-10], sol[1e-4], sol[1e-7], start, start, np.zeros(n), start], axis=1)
        refs = [_single(H, P, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(8)]
        steps = [r.iterations for _, r in refs]
        print("steps per column:", steps, "status:", [r.status for _, r in refs])
        assert not refs[0][0].any() and refs[0][1].b_norm == 0          # b = 0: x = 0 whatever the start
        assert (refs[1][1].iterations, refs[1][1].status) == (0, capi.CG_CONVERGED) and _bits_equal(refs[1][0], X0[:, 1])
        for j in (4, 5):          # the NaN and the Inf: breakdown at step 0, x untouched
            assert (refs[j][1].iterations, refs[j][1].status) == (0, capi.CG_BREAKDOWN) and _bits_equal(refs[j][0], X0[:, j])
        assert all(refs[j][1].status == capi.CG_CONVERGED for j in (2, 3, 6, 7)) and 0 < steps[3] <= steps[2] <= steps[6] and steps[3] < steps[6], steps
        for order in (list(range(8)), [6, 4, 0, 7, 1, 2, 5, 3]):
            for ldb, ldx, shift in ((8, 8, 0), (11, 9, 1)):
                for every in (1, 3, MAX_ITERS):
                    X, res = _multi(H, P, B[:, order], X0[:, order], ldb=ldb, ldx=ldx, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                    _assert_columns(X, res, [refs[j] for j in order], (order, ldb, ldx, shift, every))
                    for at, j in enumerate(order):
                        if j in (4, 5):
                            assert _bits_equal(X[:, at], X0[:, j]), (order, j)
        Xh, rh = H.pcg_multi_host(P, B, X0, rtol=rtol, max_iters=MAX_ITERS)
        _assert_columns(Xh, rh, refs, "host")
        order = [3, 0, 4, 7, 2]          # (an odd number of columns: the early stops share sub-blocks with other neighbours)
        X, res = _multi(H, P, B[:, order], X0[:, order], ldb=6, ldx=5, rtol=rtol, max_iters=MAX_ITERS, check_every=3)
        _assert_columns(X, res, [refs[j] for j in order], order)
        # -A (the object is still A's): p . A p < 0 in every column at step 0, X untouched
        N = cvr_amd.CvrMatrix(n, n, S.rp, S.ci, -S.va, nvec=8)
        try:
            B2, X2 = _block(n, dtype, seed=12)
            X, res = _multi(N, P, B2, X2, rtol=rtol, max_iters=MAX_ITERS)
            for j in range(8):
                assert (res[j].status, res[j].iterations) == (capi.CG_BREAKDOWN, 0), j
                _same_result(res[j], _single(N, P, B2[:, j], x0=X2[:, j], rtol=rtol, max_iters=MAX_ITERS)[1], ("-A", j))
            assert _bits_equal(X, X2)
        finally:
            N.close()
    finally:
        S.close()


# ---- what it is for ----
def test_block_diagonal_system_with_eight_right_hand_sides_within_two_steps():
    n, bs, rtol = 4096, 8, 1e-10
    _, _, rp, ci, va = synth.block_diag_spd(n, bs, cond=1e3)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
    P = capi.Precond.block_jacobi(rp, ci, va, bs)
    try:
        assert P.info.identity_blocks == 0
        B, _ = _block(n, np.float64)
        X, res = _multi(A, P, B, rtol=rtol, max_iters=MAX_ITERS)
        for j in range(8):
            y, _ = O.csr_spmv64(rp, ci, va, X[:, j])
            true = float(np.linalg.norm(B[:, j] - y) / np.linalg.norm(B[:, j]))
            print(f"column {j}: {res[j].iterations} steps, true residual / rtol = {true / rtol:.3g}")
            assert res[j].status == capi.CG_CONVERGED and res[j].iterations <= 2, (j, res[j].status, res[j].iterations)
            assert true <= 2 * rtol, (j, true)
    finally:
        P.close()
        A.close()


# ---- the neighbours ----
def test_single_vector_path_and_errors_with_real_objects():
    dtype, rtol = np.float64, 1e-10
    n, bs = 250, 3
    M = System(n, bs, dtype)
    nrows, _, prp, pci, _ = synth.web_google_like(0.5)
    na, _, rpa, cia, vaa = synth.spd_from_pattern(nrows, prp, pci)
    A = cvr_amd.CvrMatrix(na, na, rpa, cia, vaa)          # default options: the rules pick a layout that is not the plain one
    PA = P = capi.Precond.block_jacobi(rpa, cia, vaa, bs)
    try:
        assert not A.spmm_supported
        B, X0 = _block(na, dtype, k=2)
        # one vector of stride 1 runs on any handle and is cvr_pcg_device
        ref = _single(A, P, B[:, 0], x0=X0[:, 0], rtol=rtol, max_iters=MAX_ITERS)
        assert ref[1].iterations > 0
        for shift in (0, 1):
            X, res = _multi(A, P, B[:, :1], X0[:, :1], shift=shift, rtol=rtol, max_iters=MAX_ITERS)
            _assert_columns(X, res, [ref], ("default handle", shift))
        Xh, rh = A.pcg_multi_host(P, B[:, :1], X0[:, :1], rtol=rtol, max_iters=MAX_ITERS)
        _assert_columns(Xh, rh, [ref], "default handle, host")
        with pytest.raises(capi.CvrError) as e:
            _multi(A, P, B, X0, rtol=rtol, max_iters=MAX_ITERS)
        assert e.value.code == capi.ERR_STATE and "nvec" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            A.pcg_multi_host(P, B, X0, rtol=rtol, max_iters=MAX_ITERS)
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.CvrError) as e:          # one vector, but not of stride 1
            _multi(A, P, B[:, :1], X0[:, :1], ldb=2, ldx=1, rtol=rtol, max_iters=MAX_ITERS)
        assert e.value.code == capi.ERR_STATE
        # the pair: n, type, device
        S, P = M, M.P
        B, X0 = _block(n, dtype, k=2)
        _, _, rp2, ci2, va2 = KM.banded("spd", n + 1, dtype)
        Q = capi.Precond.block_jacobi(rp2, ci2, va2, bs)
        with pytest.raises(capi.CvrError) as e:
            _multi(M.H, Q, B, X0, rtol=rtol, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "nrows" in str(e.value) and "cvr_pcg_multi" in str(e.value)
        Q.close()
        F = capi.Precond.block_jacobi(S.rp, S.ci, S.va.astype(np.float32), bs)
        with pytest.raises(capi.CvrError) as e:
            _multi(M.H, F, B, X0, rtol=rtol, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "type" in str(e.value)
        with pytest.raises(capi.CvrError) as e:
            M.H.pcg_multi_host(F, B, X0, rtol=rtol, max_iters=3)
        assert e.value.code == capi.ERR_INVALID
        F.close()
        if cvr_amd.device_count() >= 2:
            D = capi.Precond.block_jacobi(S.rp, S.ci, S.va, bs, device=1)
            with pytest.raises(capi.CvrError) as e:
                _multi(M.H, D, B, X0, rtol=rtol, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "device" in str(e.value)
            D.close()
            torch.cuda.set_device(0)
        # a rectangular handle; R == Z
        R = cvr_amd.CvrMatrix(n, n + 7, S.rp, S.ci, S.va, nvec=8)
        with pytest.raises(capi.CvrError) as e:
            _multi(R, P, B, X0, rtol=rtol, max_iters=3)
        assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
        R.close()
        t = _dev(B, dtype)
        with pytest.raises(capi.CvrError) as e:
            P.apply_multi(t.data_ptr(), 2, t.data_ptr(), 2, 2)
        assert e.value.code == capi.ERR_INVALID and "same block" in str(e.value)
    finally:
        PA.close()
        A.close()
        M.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_one_object_two_handles_and_no_state_left_behind(prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    S = System(1000, 8, dtype)
    H2 = cvr_amd.CvrMatrix(S.n, S.n, S.rp, S.ci, S.va, nvec=8, mutable_values=1)
    try:
        H, P = S.H, S.P
        B, X0 = _block(S.n, dtype, k=4)
        D = capi.Precond.block_jacobi(S.rp, S.ci, S.va, 1)
        minv = D.export().reshape(-1)
        D.close()
        before_cg = _multi(H, None, B, X0, minv=minv, rtol=rtol, max_iters=MAX_ITERS)
        before_pcg = [_single(H, P, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(4)]
        first = None
        for A in (H, H2, H):          # the object belongs to no handle: two handles use it in turn, with the same bits
            X, res = _multi(A, P, B, X0, ldb=5, ldx=4, rtol=rtol, max_iters=MAX_ITERS)
            _assert_columns(X, res, before_pcg, "two handles")
            first = X if first is None else first
            assert _bits_equal(X, first)
        # cvr_cg_multi_device and cvr_pcg_device give their old bits on the same handle afterwards
        after_cg = _multi(H, None, B, X0, minv=minv, rtol=rtol, max_iters=MAX_ITERS)
        assert _bits_equal(after_cg[0], before_cg[0])
        for a, b in zip(after_cg[1], before_cg[1]):
            _same_result(a, b, "cg_multi afterwards")
        for j in range(4):
            x, r = _single(H, P, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS)
            assert _bits_equal(x, before_pcg[j][0])
            _same_result(r, before_pcg[j][1], ("pcg afterwards", j))
    finally:
        H2.close()
        S.close()
