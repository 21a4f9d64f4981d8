"""GPU (MI355X): batched conjugate gradients -- cvr_cg_multi_device / cvr_cg_multi, all through the ABI.

The reference is the single solver on the same handle: column j of X and its (iterations, status, residual_norm, b_norm) must be bit for bit
what cvr_cg_device returns for b = B[:, j] and x0 = X[:, j] with the same options.  The matrices are test_gpu_cg's (synth.spd_from_pattern over
an R-MAT, a web-Google-like and a banded pattern: kappa <= 3, at most 19 steps to 1e-10 in fp64 and 8 to 1e-4 in fp32), the handles are made
with nvec = 8 (the plain layout, which the k-wide product needs).

  * every nvec, leading dimension, alignment and check_every, fp64 and fp32, and the host twin; the padding columns keep their sentinel bits
  * columns that stop at different steps; columns with a NaN or an Inf in b, -A; the Jacobi preconditioner shared by the columns
  * the packet loop's edges: a partial packet alone, a whole trip and one value, the second trip ending in a partial packet
  * the stop states, the error returns with a real handle, and the neighbours: mutable handles, streams, no state left behind
"""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import cases as K
import cvr_amd
import oraclelib as O
from cvr_amd import capi, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 40
SENTINEL = -777.25          # (exact in fp32 and fp64) what stands in the padding columns of B and X


@functools.lru_cache(maxsize=None)
def _pattern(name):
    if name == "web":
        n, _, rp, ci, _ = synth.web_google_like(scale=0.05)
    elif name == "banded":
        n, _, rp, ci, _ = synth.banded_sym(40000)
    else:
        n, _, rp, ci, _ = synth.rmat(14, dedupe=True)
    return n, rp, ci


@functools.lru_cache(maxsize=None)
def _spd(name, dtype):
    n, rp, ci = _pattern(name)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


@pytest.fixture(scope="module")
def handle():
    """handle(name, dtype): the nvec = 8 handle of a test matrix, made once"""
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            n, _, rp, ci, va = _spd(name, dtype)
            made[name, dtype] = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
            assert made[name, dtype].spmm_supported
        return made[name, dtype]
    yield get
    for A in made.values():
        A.close()


def _tdt(H):
    return torch.float64 if H.dtype == np.float64 else torch.float32


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _dbits(v):
    return struct.pack("<d", v)


def _dev(H, a, shift=0):
    """a device copy of `a` (any shape) of exactly its size, `shift` elements off the allocation's start"""
    a = np.ascontiguousarray(a, dtype=H.dtype)
    t = torch.empty(a.size + shift, dtype=_tdt(H), device="cuda")[shift:]
    t.copy_(torch.from_numpy(a.reshape(-1)))
    return t


def _single(H, b, x0=None, minv=None, **kw):
    """cvr_cg_device on arrays of exactly nrows values; (x, result)"""
    n = H.nrows
    bt, xt = _dev(H, b), _dev(H, np.zeros(n) if x0 is None else x0)
    mt = None if minv is None else _dev(H, minv)
    torch.cuda.synchronize()
    res = H.cg(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), res


def _multi(H, B, X0=None, ldb=None, ldx=None, shift=0, minv=None, stream=None, **kw):
    """cvr_cg_multi_device on blocks of exactly nrows rows of ldb / ldx values whose padding columns hold SENTINEL; checks that B and the padding of
    X come back with the same bits; (X, results)"""
    n, nvec = B.shape
    ldb, ldx = ldb or nvec, ldx or nvec
    hb = np.full((n, ldb), SENTINEL, dtype=H.dtype)
    hb[:, :nvec] = B
    hx = np.full((n, ldx), SENTINEL, dtype=H.dtype)
    hx[:, :nvec] = 0 if X0 is None else X0
    bt, xt = _dev(H, hb, shift), _dev(H, hx, shift)
    mt = None if minv is None else _dev(H, minv, shift)
    torch.cuda.synchronize()
    res = H.cg_multi(bt.data_ptr(), ldb, xt.data_ptr(), ldx, nvec, minv_ptr=None if mt is None else mt.data_ptr(), stream=stream, **kw)
    torch.cuda.synchronize()
    assert len(res) == nvec
    assert _bits_equal(bt.cpu().numpy().reshape(n, ldb), hb), "B was written"
    X = xt.cpu().numpy().reshape(n, ldx)
    assert _bits_equal(X[:, nvec:], hx[:, nvec:]), "the padding columns of X were written"
    return np.ascontiguousarray(X[:, :nvec]), res


def _same_result(r, ref, ctx):
    assert (r.iterations, r.status) == (ref.iterations, ref.status), (ctx, r.iterations, r.status, ref.iterations, ref.status)
    assert _dbits(r.residual_norm) == _dbits(ref.residual_norm) and _dbits(r.b_norm) == _dbits(ref.b_norm), (ctx, r.residual_norm, ref.residual_norm, r.b_norm, ref.b_norm)


def _assert_columns(X, res, refs, ctx):
    """column j of the block solve against the single solve refs[j] = (x, result)"""
    for j, (xr, rr) in enumerate(refs):
        _same_result(res[j], rr, (ctx, j))
        assert _bits_equal(X[:, j], xr), (ctx, j, "x differs", int(np.sum(X[:, j] != xr)))
    assert len({r.spmv_count for r in res}) == 1 and len({r.seconds for r in res}) == 1


def _true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, x)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))


def _block(n, dtype, k=8, seed=11):
    """k right-hand sides and start vectors: x_rand and seeded normals from a zero start, the later ones from a random start"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    B[:, 0] = synth.x_rand(n)
    X0 = np.zeros((n, k))
    X0[:, 2::3] = rng.random((n, len(range(2, k, 3)))) * 2 - 1
    return B.astype(dtype), X0.astype(dtype)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["rmat", "web", "banded"])
def test_bit_for_bit_against_the_single_solver(handle, name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    H, rtol = handle(name, dtype), RTOL[dtype]
    n = H.nrows
    B, X0 = _block(n, dtype)
    refs = [_single(H, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(8)]
    assert all(r.status == capi.CG_CONVERGED and r.iterations > 0 for _, r in refs)
    for nvec in (1, 2, 3, 5, 8):
        for ldb, ldx in ((nvec, nvec), (nvec + 3, nvec + 1)):
            for shift in (0, 1):
                counts = []
                for every in (1, 3, MAX_ITERS):
                    X, res = _multi(H, B[:, :nvec], X0[:, :nvec], ldb=ldb, ldx=ldx, shift=shift, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
                    _assert_columns(X, res, refs[:nvec], (name, prec, nvec, ldb, ldx, shift, every))
                    counts.append(res[0].spmv_count)
                # read back after every step, nothing is enqueued behind the last column's stop; with one read-back, everything is
                assert counts[0] == max(r.iterations for _, r in refs[:nvec]) + 1 and counts == sorted(counts) and counts[-1] == MAX_ITERS + 1
        Xh, rh = H.cg_multi_host(B[:, :nvec], X0[:, :nvec], rtol=rtol, max_iters=MAX_ITERS)          # the host twin
        _assert_columns(Xh, rh, refs[:nvec], (name, prec, nvec, "host"))


def test_columns_that_stop_at_different_steps(handle):
    """a late column must not freeze with an early one, and an early column must not leak into the others"""
    dtype = np.float64
    H = handle("rmat", dtype)
    n = H.nrows
    b = synth.x_rand(n)
    sol = {t: _single(H, b, rtol=t, max_iters=MAX_ITERS)[0] for t in (1e-4, 1e-7, 1e-10)}
    rng = np.random.default_rng(3)
    e5 = np.zeros(n)
    e5[5] = 1
    B = np.stack([b, b, b, b, np.zeros(n), e5, np.ones(n), rng.standard_normal(n)], axis=1)
    X0 = np.stack([np.zeros(n), sol[1e-4], sol[1e-7], sol[1e-10], rng.random(n) * 2 - 1, np.zeros(n), np.zeros(n), np.zeros(n)], axis=1)
    refs = [_single(H, B[:, j], x0=X0[:, j], rtol=1e-10, max_iters=MAX_ITERS) for j in range(8)]
    steps = [r.iterations for _, r in refs]
    print("steps per column:", steps)
    assert all(r.status == capi.CG_CONVERGED for _, r in refs)
    assert len(set(steps)) >= 4, steps
    assert not refs[4][0].any() and refs[4][1].b_norm == 0          # b = 0: x = 0 whatever the start
    for ldb, ldx, shift in ((8, 8, 0), (11, 9, 1)):
        for every in (1, 3, MAX_ITERS):
            X, res = _multi(H, B, X0, ldb=ldb, ldx=ldx, shift=shift, rtol=1e-10, max_iters=MAX_ITERS, check_every=every)
            _assert_columns(X, res, refs, (ldb, ldx, shift, every))
    Xh, rh = H.cg_multi_host(B, X0, rtol=1e-10, max_iters=MAX_ITERS)
    _assert_columns(Xh, rh, refs, "host")
    # (an odd number of columns in another order: the early stops share sub-blocks with other neighbours)
    order = [3, 0, 4, 7, 2]
    X, res = _multi(H, B[:, order], X0[:, order], ldb=6, ldx=5, rtol=1e-10, max_iters=MAX_ITERS, check_every=3)
    _assert_columns(X, res, [refs[j] for j in order], order)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_isolation_of_bad_columns(handle, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    H, rtol = handle("rmat", dtype), RTOL[dtype]
    n = H.nrows
    B, X0 = _block(n, dtype, k=5)
    X0[:, 1] = np.random.default_rng(8).random(n) * 2 - 1
    X0[:, 3] = X0[:, 1]
    B[n // 3, 1] = np.nan
    B[n - 1, 3] = np.inf
    refs = [_single(H, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(5)]
    for ldb, ldx, every in ((5, 5, 0), (8, 6, 1)):
        X, res = _multi(H, B, X0, ldb=ldb, ldx=ldx, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
        for j in (1, 3):          # the NaN and the Inf: breakdown at step 0, x untouched
            assert res[j].status == capi.CG_BREAKDOWN and res[j].iterations == 0, (j, res[j].status, res[j].iterations)
            assert _bits_equal(X[:, j], X0[:, j]), j
            assert (refs[j][1].status, refs[j][1].iterations) == (capi.CG_BREAKDOWN, 0)
        for j in (0, 2, 4):       # the finite columns: their single solves
            _same_result(res[j], refs[j][1], (ldb, every, j))
            assert refs[j][1].status == capi.CG_CONVERGED and _bits_equal(X[:, j], refs[j][0]), (ldb, every, j)
    # -A: p . A p < 0 in every column at step 0
    _, _, rp, ci, va = _spd("rmat", dtype)
    N = cvr_amd.CvrMatrix(n, n, rp, ci, -va, nvec=8)
    B, X0 = _block(n, dtype, k=8, seed=12)
    X, res = _multi(N, B, X0, rtol=rtol, max_iters=MAX_ITERS)
    for j in range(8):
        assert res[j].status == capi.CG_BREAKDOWN and res[j].iterations == 0, j
        ref = _single(N, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS)[1]
        _same_result(res[j], ref, ("-A", j))
    assert _bits_equal(X, X0)
    N.close()


def test_jacobi_preconditioner_shared_by_the_columns():
    dtype, rtol = np.float64, 1e-10
    for name in ("rmat", "web", "banded"):
        n, rp, ci = _pattern(name)
        s = 10.0 ** (2 * np.random.default_rng(20261016).random(n))
        _, _, rp2, ci2, va = synth.spd_from_pattern(n, rp, ci, dscale=s, dtype=dtype)
        A = cvr_amd.CvrMatrix(n, n, rp2, ci2, va, nvec=8)
        B, X0 = _block(n, dtype, k=4)
        minv = 1.0 / (s * s)
        refs = [_single(A, B[:, j], x0=X0[:, j], minv=minv, rtol=rtol, max_iters=MAX_ITERS) for j in range(4)]
        for ldb, ldx, shift, every in ((4, 4, 0, 0), (7, 5, 1, 1)):
            X, res = _multi(A, B, X0, ldb=ldb, ldx=ldx, shift=shift, minv=minv, rtol=rtol, max_iters=MAX_ITERS, check_every=every)
            _assert_columns(X, res, refs, (name, ldb, ldx, shift, every))
        for j in range(4):
            true = _true_residual(rp2, ci2, va, X[:, j], B[:, j])
            print(f"S A S/{name} column {j}: {res[j].iterations} steps, true / rtol = {true / rtol:.3f}")
            assert res[j].status == capi.CG_CONVERGED and true <= 2 * rtol, (name, j, true)
        A.close()


def _banded_spd(n, dtype, half_band=2):
    n, _, rp, ci, _ = synth.banded_sym(n, half_band=half_band)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


@pytest.mark.parametrize("prec,n,nvec", [(p, n, k) for p in ("fp64", "fp32") for n in (1, 3, 5, 257 * 2 + 1) for k in (3, 8)] + [("fp64", 1024 * 256 * 2 + 3, 2)])
def test_packet_loop_edges(prec, n, nvec):
    """n = 1, 3, 5: a partial packet only (fp32: 5 is a whole packet and one value); 515: some threads with a whole packet, one with a partial one,
    the rest with none; 1024 * 256 * 2 + 3 in fp64: every thread's first trip, then the second trip ending in a partial packet"""
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    _, _, rp, ci, va = _banded_spd(n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
    B, X0 = _block(n, dtype, k=nvec, seed=n % 1000)
    refs = [_single(A, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(nvec)]
    assert all(r.status == capi.CG_CONVERGED for _, r in refs)
    for ldb, ldx, shift in ((nvec, nvec, 0), (nvec + 1, nvec + 2, 1)):
        X, res = _multi(A, B, X0, ldb=ldb, ldx=ldx, shift=shift, rtol=rtol, max_iters=MAX_ITERS)
        _assert_columns(X, res, refs, (n, nvec, ldb, ldx, shift))
    A.close()


def test_stop_states(handle):
    dtype, rtol = np.float64, 1e-10
    H = handle("rmat", dtype)
    n = H.nrows
    B, X0 = _block(n, dtype, k=3)
    X0[:, 0] = np.random.default_rng(5).random(n) * 2 - 1
    # max_iters = 0: the initial residual alone
    X, res = _multi(H, B, X0, rtol=rtol, max_iters=0)
    assert _bits_equal(X, X0)
    for j in range(3):
        assert res[j].spmv_count == 1 and res[j].iterations == 0 and res[j].status == capi.CG_MAX_ITERS
        _same_result(res[j], _single(H, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=0)[1], ("max_iters 0", j))
    # max_iters = 2 with nothing converged
    X, res = _multi(H, B, X0, ldb=4, ldx=6, rtol=rtol, max_iters=2)
    refs = [_single(H, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=2) for j in range(3)]
    _assert_columns(X, res, refs, "max_iters 2")
    assert all(r.spmv_count == 3 and r.iterations == 2 and r.status == capi.CG_MAX_ITERS for r in res)


def test_errors_and_the_single_vector_path_with_real_handles():
    nrows, _, prp, pci, _ = synth.web_google_like(0.5)
    n, _, rp, ci, va = synth.spd_from_pattern(nrows, prp, pci)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)          # default options: the rules pick a layout that is not the plain one
    assert not A.spmm_supported
    B, X0 = _block(n, np.float64, k=2)
    with pytest.raises(capi.CvrError) as e:
        _multi(A, B, X0, rtol=1e-10, max_iters=MAX_ITERS)
    assert e.value.code == capi.ERR_STATE and "nvec" in str(e.value)
    with pytest.raises(capi.CvrError) as e:
        A.cg_multi_host(B, X0, rtol=1e-10, max_iters=MAX_ITERS)
    assert e.value.code == capi.ERR_STATE and "nvec" in str(e.value)
    with pytest.raises(capi.CvrError) as e:          # one vector, but not of stride 1
        _multi(A, B[:, :1], X0[:, :1], ldb=2, ldx=1, rtol=1e-10, max_iters=MAX_ITERS)
    assert e.value.code == capi.ERR_STATE
    # one vector of stride 1 runs on any layout
    ref = _single(A, B[:, 0], x0=X0[:, 0], rtol=1e-10, max_iters=MAX_ITERS)
    assert ref[1].status == capi.CG_CONVERGED
    for shift in (0, 1):
        X, res = _multi(A, B[:, :1], X0[:, :1], shift=shift, rtol=1e-10, max_iters=MAX_ITERS)
        _assert_columns(X, res, [ref], ("default handle", shift))
    Xh, rh = A.cg_multi_host(B[:, :1], X0[:, :1], rtol=1e-10, max_iters=MAX_ITERS)
    _assert_columns(Xh, rh, [ref], "default handle, host")
    A.close()
    # rectangular
    n, rp, ci = _pattern("rmat")
    R = cvr_amd.CvrMatrix(n, n + 7, rp, ci, np.ones(len(ci)), nvec=8)
    with pytest.raises(capi.CvrError) as e:
        _multi(R, np.ones((n, 2)), rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID and "square" in str(e.value)
    with pytest.raises(capi.CvrError) as e:
        R.cg_multi_host(np.ones((n, 2)), rtol=1e-6, max_iters=3)
    assert e.value.code == capi.ERR_INVALID
    R.close()
    # before cvr_preprocess
    L = capi.lib()
    nrows, ncols, crp, cci, cva = K.cases()["uniform_2000"]
    view = capi.CsrView(nrows, ncols, crp.ctypes.data, cci.ctypes.data, cva.ctypes.data, 0)
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), None) == 0, cvr_amd.last_error()
    bt = torch.ones(nrows * 2, dtype=torch.float64, device="cuda")
    xt = torch.zeros(nrows * 2, dtype=torch.float64, device="cuda")
    opt, res = capi.CgOptions(), (capi.CgResult * 2)()
    L.cvr_cg_default_options(C.byref(opt))
    assert L.cvr_cg_multi_device(h, bt.data_ptr(), 2, xt.data_ptr(), 2, 2, C.byref(opt), res, None) == capi.ERR_STATE
    assert "cvr_preprocess" in cvr_amd.last_error()
    hb = np.ones(nrows * 2)
    assert L.cvr_cg_multi(h, hb.ctypes.data, hb.ctypes.data, 2, C.byref(opt), res) == capi.ERR_STATE
    assert L.cvr_destroy(h) == 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_neighbours(handle, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    n, _, rp, ci, va = _spd("web", dtype)
    H = handle("web", dtype)
    B, X0 = _block(n, dtype, k=4)
    # no state left behind: a plain k-wide product gives the same bits before and after a solve
    xt = torch.zeros((H.info.x_elems, 4), dtype=_tdt(H), device="cuda")
    xt[:n] = torch.from_numpy(B)

    def plain():
        yt = torch.full((H.info.yext_elems, 4), float("nan"), dtype=_tdt(H), device="cuda")
        torch.cuda.synchronize()
        H.spmm_device(xt.data_ptr(), 4, yt.data_ptr(), 4, 4)
        torch.cuda.synchronize()
        return yt[:n].cpu().numpy()
    before = plain()
    X, res = _multi(H, B, X0, rtol=rtol, max_iters=MAX_ITERS)
    assert all(r.status == capi.CG_CONVERGED for r in res)
    assert _bits_equal(plain(), before)
    # a torch side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Xs, rs = _multi(H, B, X0, rtol=rtol, max_iters=MAX_ITERS, stream=side.cuda_stream)
    assert _bits_equal(Xs, X)
    for a, b in zip(rs, res):
        _same_result(a, b, "side stream")
    # a mutable handle: A, then 2 A; each solve is the single solver's on the handle as it is then
    M = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8, mutable_values=1)
    for vals in (va, (2 * va).astype(dtype)):
        if vals is not va:
            M.update_values(vals)
        refs = [_single(M, B[:, j], x0=X0[:, j], rtol=rtol, max_iters=MAX_ITERS) for j in range(4)]
        Xm, rm = _multi(M, B, X0, ldb=5, ldx=4, rtol=rtol, max_iters=MAX_ITERS)
        _assert_columns(Xm, rm, refs, "mutable")
        assert all(r.status == capi.CG_CONVERGED for r in rm)
        assert max(_true_residual(rp, ci, vals, Xm[:, j], B[:, j]) for j in range(4)) <= 2 * rtol
    M.close()
