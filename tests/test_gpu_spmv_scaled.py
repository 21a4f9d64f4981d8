"""GPU (MI355X): the scaled product y = alpha A x + beta y -- cvr_spmv_scaled_device / cvr_spmv_scaled.

  * every layout (plain, narrow columns, window + several waves, column phases with wide row tags and bounded pieces, hub table, re-ordered x,
    column panels, interleaved and gang chunks, nvec >= 2, the default options) in fp64 and fp32 over the seeded cases: the first nrows values of
    y are alpha * s + beta * y0 in the handle's type, bit for bit, s = cvr_spmv_device's y of the same handle; the fused write-out is bit for bit
    the two-pass form (CVR_DEBUG=scaled_two_pass); beta = 0 does not read y, alpha = 0 reads neither x nor the matrix; no state is left behind
  * rows cut over chunks on single images and on panels, both forms of the combine pass and the cut-row fold
  * the fused one-submission handle, torch streams and a captured graph, the image cache, a mutable handle after an update, full-size shapes
"""
import numpy as np
import pytest

import cases as K
import cvr_amd
from cvr_amd import capi, synth
from fuzz_checks import _bits_equal, _expect          # (shared with test_gpu_fuzz_derived.py)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = K.cases()
CASES32 = K.cases(np.float32)

LAYOUTS = K.LAYOUTS          # (the shared layout table: tests/cases.py)
ALL_LAYOUTS = K.ALL_LAYOUTS

PAIRS = [(1.0, 0.0), (2.5, 0.0), (1.0, 1.0), (-1.0, 1.0), (-0.75, 0.5), (0.0, 3.0), (0.0, 0.0)]


def _cases(dtype):
    return CASES if dtype == np.float64 else CASES32


def _tdt(H):
    return torch.float64 if H.dtype == np.float64 else torch.float32


def _plain(H, x, stream=None):
    """s = cvr_spmv_device's y"""
    xt = torch.zeros(H.info.x_elems, dtype=_tdt(H), device="cuda")
    xt[: H.ncols] = torch.from_numpy(x)
    yt = torch.full((max(H.info.yext_elems, 1),), float("nan"), dtype=_tdt(H), device="cuda")
    torch.cuda.synchronize()
    H.spmv_device(xt.data_ptr(), yt.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return yt[: H.nrows].cpu().numpy()


def _scaled(H, x, y0, alpha, beta, x_null=False, stream=None):
    xt = torch.zeros(H.info.x_elems, dtype=_tdt(H), device="cuda")
    if x is not None:
        xt[: H.ncols] = torch.from_numpy(x)
    yt = torch.full((max(H.info.yext_elems, 1),), float("nan"), dtype=_tdt(H), device="cuda")
    yt[: H.nrows] = torch.from_numpy(y0)
    torch.cuda.synchronize()
    H.spmv_scaled_device(None if x_null else xt.data_ptr(), yt.data_ptr(), alpha, beta, stream=stream)
    torch.cuda.synchronize()
    return yt[: H.nrows].cpu().numpy()


def _y0(n, dtype, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) * 4 - 2).astype(dtype)
    if n > 3:
        y[1] = -0.0          # (beta * -0 + alpha * 0 keeps its sign rules)
    return y


def _check_pairs(H, x, seed=0):
    """every (alpha, beta) of PAIRS against the formula; beta = 0 with NaN in y, alpha = 0 with NaN in x and with x = NULL; plain SpMV unchanged after"""
    dtype = H.dtype
    s = _plain(H, x)
    n = H.nrows
    out = {}
    for i, (a, b) in enumerate(PAIRS):
        y0 = _y0(n, dtype, seed + i)
        if b == 0:
            y0 = np.full(n, np.nan, dtype=dtype)          # not read
        xin = x
        if a == 0:
            xin = np.full(len(x), np.nan, dtype=dtype)      # not read
        y = _scaled(H, xin, y0, a, b)
        want = _expect(s, y0, a, b, dtype)
        assert _bits_equal(y, want), (a, b, np.flatnonzero(y.view(np.uint8) != want.view(np.uint8))[:8])
        if b == 0:
            assert not np.isnan(y).any() or np.isnan(s).any()
        if a == 0:
            assert _bits_equal(_scaled(H, None, y0, a, b, x_null=True), want)
        out[(a, b)] = y
    assert _bits_equal(_plain(H, x), s), "a scaled call left state behind"
    return out


def _make(nrows, ncols, rp, ci, va, opts):
    try:
        return cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, **opts)
    except capi.CvrError:          # (a layout the options cannot build for this matrix)
        return None


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_scaled_matches_the_formula_and_the_two_pass_form(layout, prec, monkeypatch):
    dtype = np.float64 if prec == "fp64" else np.float32
    opts = ALL_LAYOUTS[layout]
    cut = built = 0
    for name, (nrows, ncols, rp, ci, va) in _cases(dtype).items():
        monkeypatch.delenv("CVR_DEBUG", raising=False)
        A = _make(nrows, ncols, rp, ci, va, opts)
        if A is None:
            continue
        built += 1
        cut += A.info.nshared > 0
        x = synth.x_rand(ncols).astype(dtype)
        fused = _check_pairs(A, x, seed=len(name))
        A.close()
        monkeypatch.setenv("CVR_DEBUG", "scaled_two_pass")
        B = _make(nrows, ncols, rp, ci, va, opts)
        two = _check_pairs(B, x, seed=len(name))
        for k in fused:
            assert _bits_equal(fused[k], two[k]), (name, k)
        B.close()
    assert built > 0
    assert cut > 0, "no case with rows cut over chunks"


def test_fused_one_submission_handle():
    for dtype, scale in ((np.float64, 0.5), (np.float32, 1.0)):
        nrows, ncols, rp, ci, va = synth.web_google_like(scale)
        va = va.astype(dtype)
        A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
        assert A.info.preprocess_fused == 1
        _check_pairs(A, synth.x_rand(ncols).astype(dtype))
        A.close()


def _cut_matrix(f32):
    """the matrix of test_cut_rows_folded_into_the_bitmap_combine: three long rows inside one panel each"""
    rng = np.random.default_rng(99)
    n = 40_000
    deg = np.full(n, 12, dtype=np.int64)
    long_rows = {123: (4500, 0), 20_001: (4000, 20_000), 39_990: (3000, 35_000)}
    for r, (d, _) in long_rows.items():
        deg[r] = d
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ci = np.empty(rp[-1], dtype=np.int32)
    for r in range(n):
        if r in long_rows:
            ci[rp[r]:rp[r + 1]] = long_rows[r][1] + np.sort(rng.choice(5000, size=deg[r], replace=False))
        else:
            ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(n, size=deg[r], replace=False))
    va = (rng.random(rp[-1]) * 2 - 1).astype(np.float32 if f32 else np.float64)
    return n, n, rp, ci, va


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("which", ["cut_fold", "livejournal"])
def test_combine_pass_forms(which, f32, monkeypatch):
    dtype = np.float32 if f32 else np.float64
    if which == "cut_fold":
        n, nc, rp, ci, va = _cut_matrix(f32)
        kws = [{"col_panels": 8, "steps_per_chunk": 32}, {"col_panels": 8, "interleave": 1, "gang": 1, "steps_per_chunk": 32, "waves_per_block": 4}]
        debugs = ["", "no_cut_fold", "combine_bits=0", "combine_bits=1"]
    else:
        n, nc, rp, ci, va = synth.livejournal_like(scale=0.021)
        va = va.astype(dtype)
        kws = [{"col_panels": 16, "steps_per_chunk": 4}, {"col_panels": 16, "interleave": 1, "gang": 1}]
        debugs = ["combine_bits=0", "combine_bits=1"]
    x = synth.x_rand(nc).astype(dtype)
    for kw in kws:
        ref = None
        for dbg in debugs + ["scaled_two_pass"]:
            monkeypatch.setenv("CVR_DEBUG", dbg)
            A = cvr_amd.CvrMatrix(n, nc, rp, ci, va, **kw)
            assert A.info.col_panels == kw["col_panels"]
            if kw.get("steps_per_chunk") in (4, 32) and not kw.get("interleave"):
                assert A.info.nshared > 0
            got = _check_pairs(A, x)
            if ref is None:
                ref = got
            for k in got:
                assert _bits_equal(got[k], ref[k]), (kw, dbg, k)
            A.close()


def test_streams_and_graph_replay():
    nrows, ncols, rp, ci, va = synth.web_google_like(scale=0.05)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
    x = synth.x_rand(ncols)
    s = _plain(A, x)
    y0 = _y0(nrows, np.float64, 5)
    side = torch.cuda.Stream()
    y = _scaled(A, x, y0, -1.0, 1.0, stream=side.cuda_stream)
    assert _bits_equal(y, _expect(s, y0, -1.0, 1.0, np.float64))
    # a captured graph replayed k times with beta != 0: the numpy recurrence y <- alpha s + beta y
    xt = torch.zeros(A.info.x_elems, dtype=torch.float64, device="cuda")
    xt[:ncols] = torch.from_numpy(x)
    yt = torch.zeros(A.info.yext_elems, dtype=torch.float64, device="cuda")
    yt[:nrows] = torch.from_numpy(y0)
    alpha, beta = 0.25, -0.5
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm-up outside the capture
        A.spmv_scaled_device(xt.data_ptr(), yt.data_ptr(), alpha, beta, stream=side.cuda_stream)
    torch.cuda.synchronize()
    want = _expect(s, y0, alpha, beta, np.float64)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.spmv_scaled_device(xt.data_ptr(), yt.data_ptr(), alpha, beta, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        g.replay()
        want = _expect(s, want, alpha, beta, np.float64)
    torch.cuda.synchronize()
    assert _bits_equal(yt[:nrows].cpu().numpy(), want)
    del g
    A.close()


def test_host_entry_point():
    nrows, ncols, rp, ci, va = CASES["power_law_3000"]
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
    x = synth.x_rand(ncols)
    s = _plain(A, x)
    y0 = _y0(nrows, np.float64, 9)
    assert _bits_equal(A.spmv_scaled(x, y0, -1.0, 1.0), _expect(s, y0, -1.0, 1.0, np.float64))
    assert _bits_equal(A.spmv_scaled(x, None), s)
    assert _bits_equal(A.spmv_scaled(None, y0, 0.0, 2.0), _expect(s, y0, 0.0, 2.0, np.float64))
    A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_image_cache_and_mutable_handles(prec, tmp_path):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = _cases(dtype)["two_giants"]
    x = synth.x_rand(ncols).astype(dtype)
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, steps_per_chunk=16)
    path = str(tmp_path / "h.cvr")
    A.save_image(path)
    Lh = cvr_amd.CvrMatrix.from_image(path, steps_per_chunk=16)
    assert _bits_equal(_plain(Lh, x), _plain(A, x))
    _check_pairs(Lh, x)
    M = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, mutable_values=1, steps_per_chunk=16)
    M.update_values((np.random.default_rng(4).random(len(va)) * 4 - 2).astype(dtype))
    _check_pairs(M, x)
    for H in (A, Lh, M):
        H.close()


@pytest.mark.parametrize("shape", ["web_google", "livejournal"])
def test_full_size_shapes(shape):
    nrows, ncols, rp, ci, va = synth.web_google_like() if shape == "web_google" else synth.livejournal_like()
    A = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va)
    x = synth.x_rand(ncols)
    s = _plain(A, x)
    for a, b in ((-1.0, 1.0), (2.5, 0.0), (-0.75, 0.5)):
        y0 = _y0(nrows, np.float64, 11)
        assert _bits_equal(_scaled(A, x, y0, a, b), _expect(s, y0, a, b, np.float64)), (shape, a, b)
    A.close()
