"""GPU (MI355X): several vectors at once -- cvr_spmm_device over a handle created with cvr_options.nvec >= 2 (the plain layout).

  * every column j of Y is bit for bit cvr_spmv_device of X[:, j] on the same handle (the k-wide kernel keeps each vector's order of
    FMAs, ds_adds and fix-up additions), and within the parity tolerances of the CSR oracle
  * the image of such a handle is the plain layout: equal to the CPU mirror of the format
  * cut rows, strides, unaligned blocks, columns of X / Y beyond nvec, value dictionary, narrow columns, the host entry, the image
    cache, handles of other layouts, a full-size matrix on a torch stream
"""
import numpy as np
import pytest

import cases as K
import cvr_amd
from cvr_amd import capi, synth
import oraclelib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = K.cases()
CASES32 = K.cases(np.float32)
TOL64, TOL32 = 1e-12, 1e-5
NVECS = (1, 2, 3, 4, 8, 11, 16)


def _tdt(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


def _x_block(ncols, k, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((ncols, k)) * 2 - 1).astype(dtype)


def _spmv_columns(A, X):
    """cvr_spmv_device of every column of X (host, ncols x k) on A: (nrows, k)"""
    n, nc, info = A.nrows, A.ncols, A.info
    dt = _tdt(A.dtype)
    out = np.zeros((n, X.shape[1]), dtype=A.dtype)
    x = torch.zeros(info.x_elems, dtype=dt, device="cuda")
    y = torch.zeros(max(info.yext_elems, 1), dtype=dt, device="cuda")
    for j in range(X.shape[1]):
        x[:nc] = torch.from_numpy(np.ascontiguousarray(X[:, j]))
        torch.cuda.synchronize()
        A.spmv_device(x.data_ptr(), y.data_ptr())
        torch.cuda.synchronize()
        out[:, j] = y[:n].cpu().numpy()
    return out


def _spmm(A, X, ldx=None, ldy=None, xoff=0, yoff=0, fill_x=0.0, fill_y=0.0, stream=None, raw=False):
    """cvr_spmm_device of X (host, ncols x k) with the given strides / element offsets; X's positions beyond k hold fill_x (the pad
    row's too), Y starts as fill_y.  Returns Y[:nrows, :k] -- or the whole Y buffer (yext_elems x ldy) with raw=True."""
    nc, info = A.ncols, A.info
    k = X.shape[1]
    ldx, ldy = ldx or k, ldy or k
    dt = _tdt(A.dtype)
    xb = torch.full((xoff + info.x_elems * ldx + 8,), fill_x, dtype=dt, device="cuda")
    xv = xb[xoff: xoff + info.x_elems * ldx].view(info.x_elems, ldx)
    xv[:nc, :k] = torch.from_numpy(np.ascontiguousarray(X))
    xv[nc, :k] = 0
    yb = torch.full((yoff + max(info.yext_elems, 1) * ldy + 8,), fill_y, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    A.spmm_device(xb.data_ptr() + xoff * xb.element_size(), ldx, yb.data_ptr() + yoff * yb.element_size(), ldy, k,
                  None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    yv = yb[yoff: yoff + max(info.yext_elems, 1) * ldy].view(-1, ldy).cpu().numpy()
    return yv if raw else yv[: A.nrows, :k].copy()


def _check_oracle(Y, X, rp, ci, va, tol, ctx):
    for j in range(X.shape[1]):
        yref, absy = O.csr_spmv64(rp, ci, va, X[:, j])
        bad, worst = O.tol_check(Y[:, j], yref, absy + (1e-30 if tol == TOL32 else 0.0), tol=tol)
        assert len(bad) == 0, (ctx, "vector", j, "rows", bad[:8], "worst rel", worst)


def _parity(A, rp, ci, va, ctx, nvecs=NVECS, seed=1):
    tol = TOL32 if A.f32 else TOL64
    X = _x_block(A.ncols, max(nvecs), A.dtype, seed)
    ref = _spmv_columns(A, X)
    for k in nvecs:
        Y = _spmm(A, X[:, :k])
        assert np.array_equal(Y.view(np.uint8), ref[:, :k].copy().view(np.uint8)), (ctx, k, "not bitwise equal to cvr_spmv_device per column")
        _check_oracle(Y, X[:, :k], rp, ci, va, tol, (ctx, k))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("S", [4, 8, 32])
@pytest.mark.parametrize("name", sorted(CASES))
def test_spmm_parity_every_case(name, S, prec):
    nrows, ncols, rp, ci, va = (CASES if prec == "fp64" else CASES32)[name]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=S, nvec=16)
    assert A.spmm_supported
    _parity(A, rp, ci, va, (name, S, prec))
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["power_law_3000", "few_rows_lt_lanes", "leading_trailing_empty", "two_giants"])
def test_nvec_handle_is_the_plain_layout(name, prec):
    nrows, ncols, rp, ci, va = (CASES if prec == "fp64" else CASES32)[name]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=8, nvec=4)
    i = A.info
    assert (i.col_phases, i.col_panels, i.interleave, i.waves_per_block, i.x_window, i.hub_entries, i.gang) == (1, 1, 0, 1, 0, 0, 0)
    mir = O.Cvr64(nrows, ncols, rp, ci, va, 8, use_dict=i.value_dict > 0, narrow=i.narrow_cols)
    assert (i.nchunks, i.nshared, i.value_dict) == (mir.nchunks, mir.nshared, mir.ndict)
    img = A.export_image()
    for key in ("image", "desc", "target", "shared"):
        assert np.array_equal(img[key], getattr(mir, key)), key
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name,S", [("two_giants", 4), ("one_row_long", 8), ("dense_row_plus_singletons", 4), ("power_law_3000", 8)])
def test_spmm_cut_rows(name, S, prec):
    nrows, ncols, rp, ci, va = (CASES if prec == "fp64" else CASES32)[name]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=S, split_threshold=16, nvec=8)
    assert A.info.nshared > 0
    _parity(A, rp, ci, va, (name, S, prec), nvecs=(2, 3, 5, 8, 11, 16), seed=3)
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("k,ldx,ldy,xoff,yoff", [(2, 5, 3, 1, 1), (3, 3, 7, 1, 0), (4, 6, 4, 1, 1), (4, 8, 9, 0, 1), (8, 12, 9, 1, 1),
                                                 (8, 8, 8, 2, 3), (11, 13, 16, 1, 1), (16, 20, 17, 0, 0), (5, 8, 8, 4, 0)])
def test_spmm_strides_offsets_and_untouched_columns(k, ldx, ldy, xoff, yoff, prec):
    """ldx > nvec, ldy > nvec, blocks that start off the 16-byte grid (X + 1, Y + 1 values): the same bits as the packed call; X's values
    beyond nvec (NaN) do not reach Y, and Y's positions beyond nvec keep their sentinel in every row, scratch rows included"""
    name = "power_law_3000"
    nrows, ncols, rp, ci, va = (CASES if prec == "fp64" else CASES32)[name]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=8, split_threshold=32, nvec=k)
    assert A.info.nshared > 0
    X = _x_block(ncols, k, A.dtype, 11)
    packed = _spmm(A, X)
    sentinel = -7.25
    Yall = _spmm(A, X, ldx=ldx, ldy=ldy, xoff=xoff, yoff=yoff, fill_x=np.nan, fill_y=sentinel, raw=True)
    Y = Yall[:nrows, :k]
    assert np.array_equal(Y.view(np.uint8), packed.view(np.uint8)), (k, ldx, ldy, xoff, yoff)
    assert not np.isnan(Y).any()
    assert np.all(Yall[:, k:] == sentinel)
    _check_oracle(Y, X, rp, ci, va, TOL32 if A.f32 else TOL64, (k, ldx, ldy))
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_spmm_value_dictionary_and_narrow_columns(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    # a pattern matrix: its few distinct values stream as one-byte codes
    rng = np.random.default_rng(4)
    nrows, ncols, rp, ci, _ = K.csr_from_lengths(rng.integers(0, 30, size=3000), 2500, rng, dtype)
    va = np.ones(len(ci), dtype=dtype)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=8, split_threshold=24, nvec=16)
    assert A.info.value_dict > 0 and A.spmm_supported
    _parity(A, rp, ci, va, ("pattern", prec))
    A.close()
    # a banded matrix: 16-bit column offsets per chunk
    nrows, ncols, rp, ci, va = synth.banded_sym(20000, 13, dtype=dtype)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=8, nvec=16)
    assert A.info.narrow_cols == 1 and A.spmm_supported
    _parity(A, rp, ci, va, ("banded", prec))
    A.close()


def test_other_layouts_and_conflicting_options():
    nrows, ncols, rp, ci, va = synth.web_google_like(scale=0.5)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
    assert A.info.waves_per_block > 1 or A.info.col_phases > 1 or A.info.x_window > 0, "expected the resident layout"
    assert not A.spmm_supported
    X = _x_block(ncols, 2, np.float64, 5)
    with pytest.raises(capi.CvrError) as e:
        _spmm(A, X)
    assert e.value.code == capi.ERR_STATE and "nvec" in str(e.value)
    Y1 = _spmm(A, X[:, :1])
    assert np.array_equal(Y1, _spmv_columns(A, X[:, :1]))
    A.close()
    n, nc, rp, ci, va = CASES["power_law_3000"]
    for opt in (dict(col_phases=4), dict(col_panels=2), dict(x_window=1024), dict(waves_per_block=4), dict(hub_table=1024), dict(hub_reorder=1),
                dict(interleave=1), dict(gang=1)):
        with pytest.raises(capi.CvrError) as e:
            cvr_amd.CvrMatrix(n, nc, rp, ci, va, nvec=2, **opt)
        assert e.value.code == capi.ERR_INVALID, opt
    # the same options with their off values are accepted
    B = cvr_amd.CvrMatrix(n, nc, rp, ci, va, nvec=2, col_phases=1, col_panels=1, x_window=0, waves_per_block=1, hub_table=0, hub_reorder=0, interleave=0, gang=0)
    assert B.spmm_supported
    B.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_spmm_host_entry_and_image_cache(prec, tmp_path):
    nrows, ncols, rp, ci, va = (CASES if prec == "fp64" else CASES32)["uniform_2000"]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, nvec=6)
    X = _x_block(ncols, 6, A.dtype, 9)
    Yd = _spmm(A, X)
    Yh, t = A.spmm(X, iters=3)
    assert Yh.shape == (nrows, 6) and t.iters == 3 and t.mean_s > 0
    assert np.array_equal(Yh, Yd)
    path = str(tmp_path / "img.cvr")
    A.save_image(path)
    B = cvr_amd.CvrMatrix.from_image(path, nvec=6)
    assert B.spmm_supported
    assert np.array_equal(_spmm(B, X), Yd)
    for other in (0, 2, 8):
        with pytest.raises(capi.CvrError) as e:
            cvr_amd.CvrMatrix.from_image(path, nvec=other)
        assert e.value.code == capi.ERR_STATE
    B.close()
    A.close()


def test_spmm_full_size_web_google():
    nrows, ncols, rp, ci, va = synth.web_google_like()
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, nvec=8)
    assert A.spmm_supported and A.info.col_phases == 1 and A.info.waves_per_block == 1
    X = _x_block(ncols, 8, np.float64, 21)
    Y = _spmm(A, X)
    _check_oracle(Y, X, rp, ci, va, TOL64, "web-Google x 8")
    assert np.array_equal(_spmm(A, X), Y)
    s = torch.cuda.Stream()
    assert np.array_equal(_spmm(A, X, stream=s), Y)
    A.close()
