"""GPU (MI355X): the handle of A^T built on the device (cvr_options.transpose).

The contract: cvr_create(A, transpose = 1) is bit for bit cvr_create(T) with T = the CSR of A^T (numpy's stable argsort of A's columns: row j
holds A's elements of column j in ascending CSR position, column index = A's row) passed as device arrays with the same options -- the image,
the gang export, every cvr_info field but the times, every result.
  * every case of cases.py plus rectangular / offset / unsorted ones, fp64 and fp32, every layout of the scaled-product tests and the defaults;
    y also against numpy's A.T @ x
  * host and device arrays of A give the same handle; a column out of range of A in device memory is refused
  * mutable_values: one array, indexed like A's vals, updates A's and A^T's handles
  * the image cache (round trip, the flag refused both ways), SpMM, the scaled product, power iteration, cvr_tune, full-size shapes
"""
import ctypes as C

import numpy as np
import pytest

import cases as K
import cvr_amd
from cvr_amd import capi, synth
from fuzz_checks import _bits, _from_device, assert_same_handle, assert_transposed_product, stable_transpose          # (shared with test_gpu_fuzz_derived.py)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAYOUTS = K.LAYOUTS          # (the shared layout table: tests/cases.py)
ALL_LAYOUTS = K.ALL_LAYOUTS


def _cases(dtype):
    out = dict(K.cases(dtype))
    rng = np.random.default_rng(20261016)
    out["unsorted_rows"] = K.csr_from_lengths(rng.integers(0, 30, size=1500), 1200, rng, dtype, sort=False)
    out["wide_short"] = K.csr_from_lengths(rng.integers(0, 60, size=40), 5000, rng, dtype)          # 40 x 5000: A^T is tall
    # row_ptr[0] > 0: the library reads positions row_ptr[0] .. row_ptr[nrows] - 1 only
    n, m, rp, ci, va = K.csr_from_lengths(rng.integers(0, 9, size=700), 650, rng, dtype)
    off = 37
    out["offset_row_ptr"] = (n, m, rp + off, np.concatenate([rng.integers(0, m, size=off).astype(np.int32), ci]),
                             np.concatenate([np.full(off, np.nan, dtype=dtype), va]))
    return out


def _try(fn):
    try:
        return fn(), None
    except capi.CvrError as e:
        return None, e.code


def _x(n, dtype, seed):
    return (np.random.default_rng(seed).random(n) * 2 - 1).astype(dtype)


def _check_pair(name, A, opts, dtype, check_numpy=True):
    nrows, ncols, rp, ci, va = A
    tn, tm, trp, tci, tva, _ = stable_transpose(nrows, ncols, rp, ci, va)
    R, rcode = _try(lambda: _from_device(tn, tm, trp, tci, tva, opts))
    H, hcode = _try(lambda: cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, **opts))
    assert rcode == hcode, (name, rcode, hcode, capi.last_error())
    if R is None:
        return False
    assert (H.nrows, H.ncols) == (ncols, nrows)
    assert_same_handle(H, R, lambda: _from_device(tn, tm, trp, tci, tva, opts))
    x = _x(nrows, dtype, 3)
    y, _ = H.spmv(x)
    yr, _ = R.spmv(x)
    assert np.array_equal(_bits(y), _bits(yr)), name
    if check_numpy:
        assert_transposed_product(y, nrows, ncols, rp, ci, va, x)
    H.close()
    R.close()
    return True


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_transposed_handle_is_the_handle_of_t(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    built = 0
    for name, A in _cases(dtype).items():
        built += _check_pair(name, A, ALL_LAYOUTS[layout], dtype)
    assert built >= 6, built


def test_host_and_device_arrays_of_a_give_the_same_handle():
    for name, (nrows, ncols, rp, ci, va) in _cases(np.float64).items():
        for opts in ({}, LAYOUTS["phases"], LAYOUTS["gang"]):
            H, hc = _try(lambda: cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, **opts))
            D, dc = _try(lambda: _from_device(nrows, ncols, rp, ci, va, opts, transpose=1))
            assert hc == dc, (name, hc, dc)
            if H is None:
                continue
            assert_same_handle(H, D, lambda: _from_device(nrows, ncols, rp, ci, va, opts, transpose=1))
            x = _x(nrows, np.float64, 5)
            assert np.array_equal(H.spmv(x)[0], D.spmv(x)[0])
            H.close()
            D.close()


def test_device_arrays_of_a_are_checked():
    nrows, ncols, rp, ci, va = K.cases()["uniform_2000"]
    bad = ci.copy()
    bad[len(bad) // 2] = ncols          # one column out of range
    with pytest.raises(capi.CvrError) as e:
        _from_device(nrows, ncols, rp, bad, va, {}, transpose=1)
    assert e.value.code == capi.ERR_INVALID
    bad[len(bad) // 2] = -3
    with pytest.raises(capi.CvrError) as e:
        _from_device(nrows, ncols, rp, bad, va, {}, transpose=1)
    assert e.value.code == capi.ERR_INVALID
    rpb = rp.copy()
    rpb[5] = rpb[6] + 1                 # row_ptr decreases
    with pytest.raises(capi.CvrError) as e:
        _from_device(nrows, ncols, rpb, ci, va, {}, transpose=1)
    assert e.value.code == capi.ERR_INVALID
    # ... and a good handle still builds afterwards (no sticky device error)
    H = _from_device(nrows, ncols, rp, ci, va, {}, transpose=1)
    assert H.nrows == ncols
    H.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_one_value_array_updates_both_handles(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    for name in ("power_law_3000", "offset_row_ptr", "one_row_long", "uniform_2000"):
        nrows, ncols, rp, ci, va = _cases(dtype)[name]
        v2 = (np.random.default_rng(9).random(len(va)) * 4 - 2).astype(dtype)
        for opts in ({}, LAYOUTS["panels"], LAYOUTS["gang"]):
            A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, **opts)
            T = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, transpose=1, **opts)
            assert T.update_values_supported()
            vt = torch.from_numpy(v2).to("cuda")
            torch.cuda.synchronize()
            A.update_values_device(vt.data_ptr())
            T.update_values_device(vt.data_ptr())
            torch.cuda.synchronize()
            FA = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, **opts)
            FT = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, transpose=1, **opts)
            assert_same_handle(A, FA, lambda: cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, **opts))
            assert_same_handle(T, FT, lambda: cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, transpose=1, **opts))
            x, xt = _x(ncols, dtype, 1), _x(nrows, dtype, 2)
            y, _ = T.spmv(xt)
            assert np.array_equal(_bits(y), _bits(FT.spmv(xt)[0]))
            assert_transposed_product(y, nrows, ncols, rp, ci, v2, xt)
            assert np.array_equal(_bits(A.spmv(x)[0]), _bits(FA.spmv(x)[0]))
            T.update_values(va)          # (host form, the creation values back)
            assert np.array_equal(_bits(T.spmv(xt)[0]), _bits(cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, mutable_values=1, **opts).spmv(xt)[0]))
            for H in (A, T, FA, FT):
                H.close()


def test_image_cache_round_trip_and_the_flag(tmp_path):
    nrows, ncols, rp, ci, va = _cases(np.float64)["two_giants"]
    x = _x(nrows, np.float64, 4)
    for mv in (0, 1):
        T = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, mutable_values=mv)
        A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=mv)
        pt, pa = str(tmp_path / f"t{mv}.cvrimg"), str(tmp_path / f"a{mv}.cvrimg")
        T.save_image(pt)
        A.save_image(pa)
        L = cvr_amd.CvrMatrix.from_image(pt, transpose=1, mutable_values=mv)
        assert (L.nrows, L.ncols) == (ncols, nrows)
        assert_same_handle(L, T)          # (the default layout of this shape: no interleaved chunks)
        assert np.array_equal(L.spmv(x)[0], T.spmv(x)[0])
        for path, flag in ((pt, 0), (pa, 1)):
            with pytest.raises(capi.CvrError) as e:
                cvr_amd.CvrMatrix.from_image(path, transpose=flag, mutable_values=mv)
            assert e.value.code == capi.ERR_STATE
        for H in (T, A, L):
            H.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_spmm_and_scaled_product(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = _cases(dtype)["power_law_3000"]
    tn, tm, trp, tci, tva, _ = stable_transpose(nrows, ncols, rp, ci, va)
    H = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, nvec=4)
    R = _from_device(tn, tm, trp, tci, tva, dict(nvec=4))
    assert H.spmm_supported
    X = np.random.default_rng(6).random((nrows, 4)).astype(dtype)
    Y, _ = H.spmm(X)
    assert np.array_equal(_bits(Y), _bits(R.spmm(X)[0]))
    for j in range(4):
        assert np.array_equal(_bits(Y[:, j]), _bits(H.spmv(X[:, j])[0]))
        assert_transposed_product(Y[:, j], nrows, ncols, rp, ci, va, X[:, j])
    H.close()
    R.close()
    H = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1)
    R = _from_device(tn, tm, trp, tci, tva, {})
    x, y0 = _x(nrows, dtype, 7), _x(ncols, dtype, 8)
    for a, b in ((1.0, 0.0), (2.5, -0.5), (0.0, 3.0)):
        ys = H.spmv_scaled(x, y0, a, b)
        assert np.array_equal(_bits(ys), _bits(R.spmv_scaled(x, y0, a, b)))
        s = H.spmv(x)[0]
        with np.errstate(all="ignore"):          # (the contract of cvr_spmv_scaled_device: beta = 0 reads no y, alpha = 0 no s)
            want = (dtype(b) * y0).astype(dtype) if a == 0 else (dtype(a) * s).astype(dtype) if b == 0 else (dtype(a) * s + dtype(b) * y0).astype(dtype)
        assert np.array_equal(_bits(ys), _bits(want)), (a, b)
    H.close()
    R.close()


def test_power_iteration_on_a_transposed_square_matrix():
    n, _, rp, ci, va = synth.web_google_like(scale=0.05)
    va = np.abs(va) + 0.01
    tn, tm, trp, tci, tva, _ = stable_transpose(n, n, rp, ci, va)
    iters = 30

    def run(H):
        xt = torch.ones(H.info.x_elems, dtype=torch.float64, device="cuda")
        xt[n:] = 0
        torch.cuda.synchronize()
        lam, _ = H.power_iteration(xt.data_ptr(), iters)
        torch.cuda.synchronize()
        return lam, xt[:n].cpu().numpy()

    H = cvr_amd.CvrMatrix(n, n, rp, ci, va, transpose=1)
    R = _from_device(tn, tm, trp, tci, tva, {})
    l1, x1 = run(H)
    l2, x2 = run(H)
    l3, x3 = run(R)
    assert l1 == l2 and np.array_equal(x1, x2)          # bitwise rerun
    assert l1 == l3 and np.array_equal(x1, x3)          # the handle of T
    # numpy on A.T: the same iteration in fp64
    rows = np.searchsorted(rp, np.arange(rp[-1]), side="right") - 1
    x = np.ones(n)
    for _ in range(iters):
        y = np.bincount(ci, weights=va * x[rows], minlength=n)
        lam = float(x @ y / (x @ x))
        x = y / np.linalg.norm(y)
    assert abs(l1 - lam) <= 1e-9 * abs(lam)
    assert np.allclose(x1, x, rtol=1e-8, atol=1e-12)
    H.close()
    R.close()


def test_tune_returns_the_option_and_a_correct_product():
    nrows, ncols, rp, ci, va = _cases(np.float64)["uniform_2000"]
    rp_, ci_, va_ = (np.ascontiguousarray(a) for a in (rp, ci, va))
    view = capi.CsrView(nrows, ncols, rp_.ctypes.data, ci_.ctypes.data, va_.ctypes.data, 0, 0)
    o, best = capi.Options(), capi.Options()
    capi.lib().cvr_default_options(C.byref(o))
    o.transpose = 1
    t, tun = C.c_double(), C.c_double()
    assert capi.lib().cvr_tune(C.byref(view), C.byref(o), C.byref(best), C.byref(t), C.byref(tun)) == 0, capi.last_error()
    assert best.transpose == 1 and t.value > 0
    H = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, transpose=1, tune_steps=True)
    assert (H.nrows, H.ncols) == (ncols, nrows)
    x = _x(nrows, np.float64, 12)
    assert_transposed_product(H.spmv(x)[0], nrows, ncols, rp, ci, va, x)
    H.close()


@pytest.mark.parametrize("shape", ["web_google", "livejournal"])
def test_full_size_shapes_match_the_handle_of_t(shape):
    nrows, ncols, rp, ci, va = synth.web_google_like() if shape == "web_google" else synth.livejournal_like()
    assert _check_pair(shape, (nrows, ncols, rp, ci, va), {}, np.float64, check_numpy=(shape == "web_google"))
