"""GPU (MI355X): new values for a converted handle -- cvr_options.mutable_values, cvr_update_values / cvr_update_values_device.

  * for every layout (plain, narrow columns, window + several waves, column phases with wide row tags and bounded pieces, hub table,
    re-ordered x, column panels, interleaved and gang chunks -- the 16-bit-tag second conversion included --, nvec >= 2, the fused
    one-submission path, device arrays) in fp64 and fp32: a handle created with v1 and updated to v2 has the image, bit for bit, of a
    fresh mutable handle created with v2 (and of a handle without dictionary), the same y, and y within the CSR oracle's tolerances
  * no dictionary for mutable handles; refusals; SpMM and the power iteration after an update; the image cache; streams and graphs;
    full-size shapes; device memory given back
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

LAYOUTS = K.LAYOUTS          # (the shared layout table: tests/cases.py)


def _cases(dtype):
    return CASES if dtype == np.float64 else CASES32


def _fresh_vals(n, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(n) * 4 - 2).astype(dtype)


def _tol(dtype):
    return TOL64 if dtype == np.float64 else TOL32


def _oracle_ok(y, rp, ci, va, x, dtype):
    yref, absy = O.csr_spmv64(rp, ci, va.astype(np.float64), x.astype(np.float64))
    bad, worst = O.tol_check(y, yref, absy, tol=_tol(dtype))
    return len(bad) == 0, worst


def _diff_keys(A, B):
    """the parts of the exported images (stream, chunk tables, gang tables) that differ; column panels export nothing (empty)"""
    if A.info.col_panels > 1:
        return set()
    a, b = A.export_image(), B.export_image()
    assert a.keys() == b.keys()
    return {k for k in a if not np.array_equal(a[k], b[k])}


def _same_image(A, B):
    return not _diff_keys(A, B)


def _check_update(nrows, ncols, rp, ci, v1, opts, seed=1, vd0=True):
    """create mutable with v1, SpMV, update to v2; compare with a fresh mutable handle of v2 (and a value_dict = 0 handle)"""
    dtype = v1.dtype
    v2 = _fresh_vals(len(v1), dtype, seed)
    x = synth.x_rand(ncols).astype(dtype)
    try:
        A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v1, mutable_values=1, **opts)
    except capi.CvrError:          # (a layout the options cannot build for this matrix: refused without the option as well)
        with pytest.raises(capi.CvrError):
            cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v1, value_dict=0, **opts)
        return None
    assert A.info.value_dict == 0 and A.update_values_supported()
    y1, _ = A.spmv(x)
    ok, worst = _oracle_ok(y1, rp, ci, v1, x, dtype)
    assert ok, ("creation values", worst)
    A.update_values(v2)
    y, _ = A.spmv(x)
    B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, **opts)
    yb, _ = B.spmv(x)
    assert np.array_equal(y.view(np.uint8), yb.view(np.uint8))
    ok, worst = _oracle_ok(y, rp, ci, v2, x, dtype)
    assert ok, ("updated values", worst)
    # The images, bit for bit, in every table the layout writes the same twice without the option: interleaved images have no steal
    # targets (`target` is left unwritten, nothing reads it), two handles of value_dict = 0 differ there as well.  The stream is always compared.
    C0 = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, value_dict=0, **opts)
    C1 = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, value_dict=0, **opts)
    loose = _diff_keys(C0, C1) | ({"target"} if A.info.interleave else set())
    assert loose <= ({"target", "gbase"} if A.info.interleave else set()), loose
    assert not (_diff_keys(A, B) - loose)
    assert not (_diff_keys(A, C0) - loose)          # the position trick leaves the image of a handle without dictionary
    C0.close()
    C1.close()
    info = A.info
    A.close()
    B.close()
    return info


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_update_matches_a_fresh_handle(layout, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    opts = LAYOUTS[layout]
    seen = []
    for name, (nrows, ncols, rp, ci, va) in _cases(dtype).items():
        info = _check_update(nrows, ncols, rp, ci, va, opts, seed=len(name))
        if info is not None:
            seen.append((name, info))
    i = dict(seen)["power_law_3000"]
    want = dict(narrow=("narrow_cols", 1), window=("x_window", None), phases=("col_phases", None), phases_tags_pieces=("row_tags16", 1), hub=("hub_entries", None),
                hub_reorder=("hub_reorder", 1), panels=("col_panels", 3), interleaved=("interleave", 1), interleaved_panels=("col_panels", 8), gang=("gang", 4),
                gang_tags=("row_tags16", 1)).get(layout)
    if want:
        field, val = want
        assert (getattr(i, field) == val) if val is not None else (getattr(i, field) > 1 if field == "col_phases" else getattr(i, field) > 0), (layout, field, getattr(i, field))
    assert any(inf.nshared > 0 for _, inf in seen), "no case with rows cut over chunks"


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_gang_second_conversion_with_16_bit_tags(prec):
    """columns further than 2^17 from their group's first: cvr_preprocess converts again with 16-bit tags -- the map is made after it"""
    dtype = np.float64 if prec == "fp64" else np.float32
    rng = np.random.default_rng(5)
    nrows, ncols = 3000, 1 << 24
    nrows, ncols, rp, ci, va = K.csr_from_lengths(rng.integers(0, 6, size=nrows), ncols, rng, dtype)
    info = _check_update(nrows, ncols, rp, ci, va, dict(col_panels=1, interleave=1, steps_per_chunk=32, waves_per_block=4, gang=1))
    assert info.gang == 4 and info.row_tags16 == 1


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_fused_path_and_device_arrays(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = synth.web_google_like(0.5 if dtype == np.float64 else 1.0)          # (x of more than 2.5 MB: the resident layout with column phases)
    va = (va * (1.0 + np.arange(len(va)) % 7)).astype(dtype)
    info = _check_update(nrows, ncols, rp, ci, va, {})
    assert info.preprocess_fused == 1, "the automatic layout did not take the one-submission path"
    # CSR arrays on the device (arrays_on_device = 1), values given back through update_values_device
    dev = torch.device("cuda", 0)
    trp, tci, tva = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp.astype(np.int64), ci.astype(np.int32), va))
    A = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr(), is_f32=dtype == np.float32, mutable_values=1)
    v2 = _fresh_vals(len(va), dtype, 3)
    tv2 = torch.from_numpy(v2).to(dev)
    torch.cuda.synchronize()
    A.update_values_device(tv2.data_ptr())
    torch.cuda.synchronize()
    x = synth.x_rand(ncols).astype(dtype)
    y, _ = A.spmv(x)
    B = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tv2.data_ptr(), is_f32=dtype == np.float32, mutable_values=1)
    yb, _ = B.spmv(x)
    assert np.array_equal(y, yb) and _same_image(A, B)
    ok, worst = _oracle_ok(y, rp, ci, v2, x, dtype)
    assert ok, worst
    A.close()
    B.close()


def test_no_dictionary_for_mutable_handles():
    nrows, ncols, rp, ci, va = CASES["dense_row_plus_singletons"]
    pat = np.ones(len(va))
    D = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, pat)
    assert D.info.value_dict > 0          # nothing existing changed: the pattern matrix keeps its dictionary
    D.close()
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, pat, mutable_values=1)
    assert A.info.value_dict == 0
    v2 = np.arange(len(va)) % 10000 * 1e-3 - 4.0
    assert len(np.unique(v2)) == 10000
    A.update_values(v2)
    x = synth.x_rand(ncols)
    y, _ = A.spmv(x)
    ok, worst = _oracle_ok(y, rp, ci, v2, x, np.float64)
    assert ok, worst
    A.close()
    with pytest.raises(capi.CvrError) as e:
        cvr_amd.CvrMatrix(nrows, ncols, rp, ci, pat, mutable_values=1, value_dict=1)
    assert e.value.code == capi.ERR_INVALID


def test_refusals_and_supported():
    import ctypes as C
    nrows, ncols, rp, ci, va = CASES["uniform_2000"]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
    assert not A.update_values_supported()
    with pytest.raises(capi.CvrError) as e:
        A.update_values(va)
    assert e.value.code == capi.ERR_STATE
    A.close()
    K_ = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, keep_csr=True)
    assert not K_.update_values_supported()
    with pytest.raises(capi.CvrError) as e:
        K_.update_values(va)
    assert e.value.code == capi.ERR_STATE
    K_.close()
    # before cvr_preprocess (the C ABI directly: CvrMatrix preprocesses in its constructor)
    L = capi.lib()
    view = capi.CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0, 0)
    o = capi.Options()
    L.cvr_default_options(C.byref(o))
    o.mutable_values = 1
    h = C.c_void_p()
    assert L.cvr_create(C.byref(h), C.byref(view), C.byref(o)) == 0
    assert L.cvr_update_values_supported(h) == 0
    assert L.cvr_update_values(h, va.ctypes.data) == capi.ERR_STATE
    assert L.cvr_preprocess(h, 0, None) == 0
    assert L.cvr_update_values_supported(h) == 1
    assert L.cvr_update_values(h, va.ctypes.data) == 0
    L.cvr_destroy(h)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_spmm_and_power_iteration_after_an_update(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = _cases(dtype)["power_law_3000"]
    v2 = _fresh_vals(len(va), dtype, 11)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, nvec=4, mutable_values=1)
    A.update_values(v2)
    B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, nvec=4, mutable_values=1)
    X = np.random.default_rng(2).random((ncols, 4)).astype(dtype)
    Ya, _ = A.spmm(X)
    Yb, _ = B.spmm(X)
    assert np.array_equal(Ya, Yb)
    A.close()
    B.close()
    # power iteration (the square matrices of the web-Google shape take the one-launch step with column phases)
    n, _, rp, ci, va = synth.web_google_like(scale=0.05)
    va = va.astype(dtype)
    v2 = np.abs(_fresh_vals(len(va), dtype, 12))
    out = []
    for H in (cvr_amd.CvrMatrix(n, n, rp, ci, va, mutable_values=1), cvr_amd.CvrMatrix(n, n, rp, ci, v2, mutable_values=1)):
        if not out:
            H.update_values(v2)
        xt = torch.ones(H.info.x_elems, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        xt[n:] = 0
        torch.cuda.synchronize()
        lam, _ = H.power_iteration(xt.data_ptr(), 12)
        torch.cuda.synchronize()
        out.append((lam, xt.cpu().numpy()))
        H.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_image_cache_keeps_the_map(prec, tmp_path):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = _cases(dtype)["two_giants"]
    v2 = _fresh_vals(len(va), dtype, 4)
    x = synth.x_rand(ncols).astype(dtype)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, steps_per_chunk=16)
    path = str(tmp_path / "mut.cvr")
    A.save_image(path)
    Lh = cvr_amd.CvrMatrix.from_image(path, mutable_values=1, steps_per_chunk=16)
    assert Lh.update_values_supported()
    Lh.update_values(v2)
    B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, steps_per_chunk=16)
    assert _same_image(Lh, B)
    assert np.array_equal(Lh.spmv(x)[0], B.spmv(x)[0])
    with pytest.raises(capi.CvrError) as e:
        cvr_amd.CvrMatrix.from_image(path, steps_per_chunk=16)          # (a mutable file under a plain key)
    assert e.value.code == capi.ERR_STATE
    P = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=16)
    path2 = str(tmp_path / "plain.cvr")
    P.save_image(path2)
    with pytest.raises(capi.CvrError) as e:
        cvr_amd.CvrMatrix.from_image(path2, mutable_values=1, steps_per_chunk=16)
    assert e.value.code == capi.ERR_STATE
    for H in (A, Lh, B, P):
        H.close()


def _dev_y(H, x, stream=None):
    dt = torch.float64 if H.dtype == np.float64 else torch.float32
    xt = torch.zeros(H.info.x_elems, dtype=dt, device="cuda")
    xt[: H.ncols] = torch.from_numpy(x)
    yt = torch.zeros(max(H.info.yext_elems, 1), dtype=dt, device="cuda")
    return xt, yt


@pytest.mark.parametrize("layout", ["plain", "panels"])
def test_update_on_another_stream_is_ordered(layout):
    nrows, ncols, rp, ci, va = synth.web_google_like(scale=0.2)
    opts = dict(col_panels=1 if layout == "plain" else 4)
    v2 = _fresh_vals(len(va), np.float64, 21)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, **opts)
    B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, **opts)
    x = synth.x_rand(ncols)
    yb, _ = B.spmv(x)
    xt, yt = _dev_y(A, x)
    t2 = torch.from_numpy(v2).cuda()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    A.spmv_device(xt.data_ptr(), yt.data_ptr(), stream=s1.cuda_stream, repeat=20)
    A.update_values_device(t2.data_ptr(), stream=s2.cuda_stream)
    A.spmv_device(xt.data_ptr(), yt.data_ptr(), stream=s3.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(yt[:nrows].cpu().numpy(), yb)
    A.close()
    B.close()


def test_graph_replays_update_and_spmv():
    nrows, ncols, rp, ci, va = CASES["power_law_3000"]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1)
    x = synth.x_rand(ncols)
    xt, yt = _dev_y(A, x)
    src = torch.from_numpy(va.copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up outside the capture
        A.update_values_device(src.data_ptr(), stream=side.cuda_stream)
        A.spmv_device(xt.data_ptr(), yt.data_ptr(), stream=side.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        A.update_values_device(src.data_ptr(), stream=st)
        A.spmv_device(xt.data_ptr(), yt.data_ptr(), stream=st)
    for seed in (31, 32, 33):
        v = _fresh_vals(len(va), np.float64, seed)
        src.copy_(torch.from_numpy(v))
        g.replay()
        torch.cuda.synchronize()
        B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v, mutable_values=1)
        assert np.array_equal(yt[:nrows].cpu().numpy(), B.spmv(x)[0]), seed
        B.close()
    del g
    A.close()


@pytest.mark.parametrize("shape", ["web_google", "livejournal"])
def test_full_size_update_matches_a_fresh_handle(shape):
    nrows, ncols, rp, ci, va = synth.web_google_like() if shape == "web_google" else synth.livejournal_like()
    v2 = _fresh_vals(len(va), np.float64, 41)
    x = synth.x_rand(ncols)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1)
    if shape == "livejournal":
        assert A.info.col_panels > 1 and A.info.gang > 0, (A.info.col_panels, A.info.gang)
    A.update_values(v2)
    y, _ = A.spmv(x)
    A.close()
    B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1)
    yb, _ = B.spmv(x)
    B.close()
    assert np.array_equal(y, yb)
    ok, worst = _oracle_ok(y, rp, ci, v2, x, np.float64)
    assert ok, worst


def test_mutable_handles_release_their_device_memory():
    nrows, ncols, rp, ci, va = CASES["power_law_3000"]
    dev = torch.device("cuda", 0)
    trp, tci, tva = (torch.from_numpy(a).to(dev) for a in (np.ascontiguousarray(rp, dtype=np.int64), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va)))
    x = O.x_vec_fast(ncols)
    v2 = _fresh_vals(len(va), np.float64, 51)

    def cycle():
        for kw in (dict(), dict(col_panels=3), dict(keep_csr=True), dict(interleave=1, gang=1, col_panels=1, steps_per_chunk=32, waves_per_block=4)):
            A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, **kw)
            if A.update_values_supported():
                A.update_values(v2)
            A.spmv(x)
            A.close()
        B = cvr_amd.CvrMatrix.from_device(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr(), mutable_values=1)
        B.update_values_device(tva.data_ptr())
        B.spmv(x)
        B.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(dev)
    for _ in range(5):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(dev)
    assert free0 - free1 < (8 << 20), (free0, free1)
