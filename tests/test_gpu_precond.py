"""GPU (MI355X): the block-Jacobi preconditioner object -- cvr_precond_block_jacobi, cvr_precond_export, cvr_precond_apply_device -- through the ABI.

Build: the exported W against numpy's fp64 inverse of the blocks precond_model.blocks_of gathers from the same CSR.  Both are computed inverses of the
same block B; each obeys the textbook forward bound c n kappa u, so per block
    |W - Wref|_max <= 64 * bs * kappa_inf(B) * 2^-53 * |Wref|_max        (+ 2^-24 * |Wref|_max in fp32: the one rounding of W to float)
with kappa_inf computed here; 64 covers pivot growth, which is 1 for these diagonally dominant blocks.  The matrices are krylov_model.banded("spd")
with one planted duplicate, read from host arrays and from device arrays; the identity fall-back on an empty row, a NaN and a singular block; and
a row of 70 000 entries.
Apply: cvr_precond_apply_device against precond_model.apply on the exported W, bit for bit, with a -0, a denormal and a huge value in r, r and z one
element off the 16-byte grid, twice, and canaries around z."""
import numpy as np
import pytest
import torch

import cvr_amd
import krylov_model as KM
import precond_model as PM
from cvr_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 32), (250, 3), (1000, 8), (4099, 16), (4099, 32), (96, 2)]
CANARY = -777.25


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _matrix(n, dtype):
    """krylov_model.banded("spd") with a second (0, 0) entry at the end of row 0"""
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    e = int(rp[1])
    ci = np.concatenate([ci[:e], [0], ci[e:]]).astype(np.int32)
    va = np.concatenate([va[:e], [0.25], va[e:]]).astype(dtype)
    rp = rp.copy()
    rp[1:] += 1
    return rp, ci, va


def _build(rp, ci, va, bs, where):
    if where == "host":
        return capi.Precond.block_jacobi(rp, ci, va, bs), None
    keep = (torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda())
    torch.cuda.synchronize()
    P = capi.Precond.block_jacobi_from_device(len(rp) - 1, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), bs, is_f32=va.dtype == np.float32)
    return P, keep


def _check_blocks(W, B, dtype, ctx, only=None):
    """the bound of the module docstring, block by block; returns the worst |W - Wref|_max / bound"""
    bs = B.shape[1]
    worst = 0.0
    for k in (range(len(B)) if only is None else only):
        ref = np.linalg.inv(B[k])
        kappa = np.abs(B[k]).sum(axis=1).max() * np.abs(ref).sum(axis=1).max()
        top = np.abs(ref).max()
        bound = 64 * bs * kappa * 2.0 ** -53 * top + (2.0 ** -24 * top if dtype == np.float32 else 0.0)
        err = np.abs(W[k].astype(np.float64) - ref).max()
        worst = max(worst, err / bound)
        assert err <= bound, (ctx, "block", k, err, bound, kappa)
    return worst


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", SHAPES)
def test_build_against_the_fp64_inverse(n, bs, prec, where):
    dtype = _dtype(prec)
    rp, ci, va = _matrix(n, dtype)
    P, keep = _build(rp, ci, va, bs, where)
    try:
        i = P.info
        assert (i.n, i.block_size, i.is_f32, i.nblocks, i.identity_blocks, i.device) == (n, bs, int(dtype == np.float32), PM.nblocks_of(n, bs), 0, 0)
        W = P.export()
        assert W.dtype == dtype and W.shape == (i.nblocks, bs, bs)
        B = PM.blocks_of(rp, ci, va, bs)
        assert B[0, 0, 0] == np.float64(va[np.flatnonzero(ci[: rp[1]] == 0)[0]]) + 0.25          # (the duplicate is in)
        worst = _check_blocks(W, B, dtype, (n, bs, prec, where))
        print(f"n {n} bs {bs} {prec} {where}: worst |W - Wref|_max / bound = {worst:.3g}")
        m = n - (i.nblocks - 1) * bs
        if m < bs:          # the identity completion of the short last block, exactly
            last = W[-1]
            assert np.array_equal(last[m:, m:], np.eye(bs - m, dtype=dtype)) and not last[:m, m:].any() and not last[m:, :m].any()
    finally:
        P.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_identity_blocks(prec):
    """bs = 2, five blocks: a healthy one, one with an empty row, one holding a NaN, an exactly singular one (1 2; 2 4), a healthy one"""
    dtype = _dtype(prec)
    rows = [[(0, 4.0), (1, 1.0)], [(0, 1.0), (1, 3.0)],
            [], [(2, 1.0), (3, 2.0)],
            [(4, 2.0), (5, np.nan)], [(4, 1.0), (5, 2.0)],
            [(6, 1.0), (7, 2.0)], [(6, 2.0), (7, 4.0)],
            [(8, 5.0), (9, -1.0), (0, 7.0)], [(8, -1.0), (9, 2.0)]]
    rp = np.zeros(11, dtype=np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    va = np.array([v for r in rows for _, v in r], dtype=dtype)
    for where in ("host", "device"):
        P, keep = _build(rp, ci, va, 2, where)
        try:
            assert P.info.nblocks == 5 and P.info.identity_blocks == 3
            W = P.export()
            for k in (1, 2, 3):
                assert np.array_equal(W[k], np.eye(2, dtype=dtype)), (k, W[k])
            _check_blocks(W, PM.blocks_of(rp, ci, va, 2), dtype, ("identity", prec, where), only=(0, 4))
        finally:
            P.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_duplicates_are_added_in_csr_order(prec):
    """bs = 2, two blocks (2 u; 0 2) whose u is the sum of three entries 2^60, -2^60, 1 of one (i, j): 1 in CSR order, 0 in the reverse order (and in
    four of the six orders), so W[0][1] is -0.25 exactly or 0.  Block 0 holds the three side by side (one trip of the scan: the claim word orders
    them); in block 1 eleven entries outside the block lie between each two (three trips).  Every value is a power of two times a small integer in
    fp32 as well, and the elimination is exact."""
    dtype = _dtype(prec)
    big = 2.0 ** 60          # (1 + 2^60 rounds to 2^60 in fp64; the entries are exact in fp32)
    filler = [(c, 3.0) for c in (0, 1)] * 5 + [(0, 3.0)]
    rows = [[(0, 2.0), (1, big), (1, -big), (1, 1.0)], [(1, 2.0)],
            [(2, 2.0), (3, big)] + filler + [(3, -big)] + filler + [(3, 1.0)], [(3, 2.0)]]
    rp = np.zeros(5, dtype=np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    va = np.array([v for r in rows for _, v in r], dtype=dtype)
    want = np.array([[0.5, -0.25], [0.0, 0.5]], dtype=dtype)
    assert np.array_equal(PM.blocks_of(rp, ci, va, 2), [[[2.0, 1.0], [0.0, 2.0]]] * 2)
    for where in ("host", "device"):
        P, keep = _build(rp, ci, va, 2, where)
        try:
            W = P.export()
            assert P.info.identity_blocks == 0
            for k in (0, 1):
                assert np.array_equal(W[k], want), (prec, where, k, W[k])
        finally:
            P.close()


def test_a_row_of_70000_entries():
    """n = 70 016, bs = 8: row 35 004 holds 70 000 entries of which 5 fall into its block (35 000 .. 35 007); every other row is its diagonal"""
    n, bs, long_row = 70016, 8, 35004
    cols = np.setdiff1d(np.arange(70003), [35000, 35002, 35007])
    assert len(cols) == 70000 and ((cols >= 35000) & (cols < 35008)).sum() == 5
    lens = np.ones(n, dtype=np.int64)
    lens[long_row] = len(cols)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    ci = np.arange(n, dtype=np.int32).repeat(lens)
    va = np.full(len(ci), 2.0)
    ci[rp[long_row]: rp[long_row + 1]] = cols
    va[rp[long_row]: rp[long_row + 1]] = np.where(cols == long_row, 2.0, 0.125 * (1 + cols % 7))
    P, _ = _build(rp, ci, va, bs, "host")
    try:
        assert P.info.identity_blocks == 0
        W = P.export()
        k = long_row // bs
        B = PM.blocks_of(rp, ci, va, bs)
        assert np.count_nonzero(B[k][long_row % bs]) == 5
        _check_blocks(W, B, np.float64, "long row", only=(0, k - 1, k, k + 1, len(B) - 1))
        assert np.array_equal(W[0], 0.5 * np.eye(bs))
    finally:
        P.close()


def _special_r(n, dtype, rng):
    r = rng.standard_normal(n).astype(dtype)
    fi = np.finfo(dtype)
    for pos, v in ((0, -0.0), (n // 2, fi.smallest_subnormal * 5), (n - 1, fi.max / 4), (n // 3, -0.0)):
        r[pos] = v
    return r


def _apply_case(P, W, n, bs, dtype, ctx):
    rng = np.random.default_rng(n + bs)
    r = _special_r(n, dtype, rng)
    want = PM.apply(W, r, bs, dtype)
    assert not np.isnan(want).any()
    tdt = _tdt(dtype)
    for shift in (0, 1):          # r on the 16-byte grid and one element off it; z always one element off
        rt = torch.empty(n + shift, dtype=tdt, device="cuda")[shift:]
        rt.copy_(torch.from_numpy(r))
        zbuf = torch.full((n + 9,), CANARY, dtype=tdt, device="cuda")
        zt = zbuf[1: 1 + n]
        got = []
        for _ in range(2):
            zt.fill_(CANARY)
            torch.cuda.synchronize()
            P.apply(rt.data_ptr(), zt.data_ptr())
            torch.cuda.synchronize()
            got.append(zt.cpu().numpy())
        assert got[0].tobytes() == got[1].tobytes(), (ctx, shift, "two calls differ")
        if got[0].tobytes() != want.tobytes():
            i = int(np.flatnonzero((got[0].view(np.uint8).reshape(n, -1) != want.view(np.uint8).reshape(n, -1)).any(axis=1))[0])
            raise AssertionError((ctx, shift, "first difference at", i, got[0][i], want[i]))
        whole = zbuf.cpu().numpy()
        assert whole[0] == CANARY and (whole[1 + n:] == CANARY).all(), (ctx, shift, "canary")
        assert rt.cpu().numpy().tobytes() == r.tobytes()
    # aligned z as well (the 16-byte stores)
    rt = torch.from_numpy(r).cuda()
    zt = torch.full((n + 8,), CANARY, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    P.apply(rt.data_ptr(), zt.data_ptr())
    torch.cuda.synchronize()
    out = zt.cpu().numpy()
    assert out[:n].tobytes() == want.tobytes() and (out[n:] == CANARY).all(), (ctx, "aligned")


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", SHAPES)
def test_apply_against_the_model(n, bs, prec):
    dtype = _dtype(prec)
    rp, ci, va = _matrix(n, dtype)
    P, _ = _build(rp, ci, va, bs, "host")
    try:
        _apply_case(P, P.export(), n, bs, dtype, (n, bs, prec))
    finally:
        P.close()


def test_apply_on_the_second_trip_of_the_packet_loop():
    n, bs, dtype = KM.GRID * 2 + 37, 4, np.float64
    assert KM.trips_of(n, KM.pack_of(dtype)) == 2
    rp, ci, va = _matrix(n, dtype)
    P, _ = _build(rp, ci, va, bs, "host")
    try:
        _apply_case(P, P.export(), n, bs, dtype, (n, bs))
    finally:
        P.close()


def test_apply_errors_with_a_real_object():
    rp, ci, va = _matrix(16, np.float64)
    P, _ = _build(rp, ci, va, 4, "host")
    try:
        t = torch.zeros(16, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.CvrError) as e:
            P.apply(t.data_ptr(), t.data_ptr())
        assert e.value.code == capi.ERR_INVALID
    finally:
        P.close()
    E = capi.Precond.block_jacobi(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 4)          # n = 0 is valid
    assert (E.info.n, E.info.nblocks, E.info.identity_blocks) == (0, 0, 0) and E.export().shape == (0, 4, 4)
    E.close()
    assert cvr_amd.device_count() >= 1
