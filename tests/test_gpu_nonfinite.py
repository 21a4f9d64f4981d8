"""GPU (MI355X): Inf and NaN in x, in the matrix values and in y -- data that shows a slot reading the wrong element.

The format rests on two rules: a pad slot has column ncols, value +0.0 and x_ext[ncols] == 0, and rows without non-zeros are written as +0.0.
With finite x a pad slot, a tail slot or a masked lane that gathers a wrong element of x contributes 0 * finite = 0 and nothing sees it; with
Inf or NaN in x the same mistake turns a clean row into NaN.  So: the class of every row of y (finite, +Inf, -Inf, NaN) is the one its own terms
a_k * x[c_k] give (cases.expected_class -- independent of the order of the additions), and every row whose terms are all finite is BIT FOR BIT
the row of the same handle for the same vector with the poisoned entries set to 0: the terms of such a row are identical in both runs, so no
tolerance is involved.  y starts as NaN over all of y_ext: a row nobody stores is caught as well.

  * every layout of cases.ALL_LAYOUTS in fp64 and fp32 over the seeded cases: containment in x for the patterns of cases.poison_patterns (the
    neighbour of the pad element, column 0, hub columns, columns read once, the edges of the x window, 2 % at random); x = Inf / NaN everywhere;
    non-finite matrix values with and without the value dictionary (image against the CPU mirror bit for bit); cvr_update_values copies bits
  * SpMM (one poisoned vector among nvec), the scaled product (poisoned y and poisoned x, fused and two-pass), transposed and cached handles
  * conjugate gradients stop with CVR_CG_BREAKDOWN on a NaN / Inf in b or in A, at step 0, x untouched
"""
import numpy as np
import pytest

import cases as K
import cvr_amd
import oraclelib as O
from cvr_amd import capi, synth
from test_gpu_spmv_scaled import _bits_equal, _plain as _spmv          # (bit comparison; cvr_spmv_device on torch buffers, y_ext pre-filled with NaN)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = K.cases()
CASES32 = K.cases(np.float32)
ALL_LAYOUTS = K.ALL_LAYOUTS
PRECS = ["fp64", "fp32"]


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _cases(dtype):
    return CASES if dtype == np.float64 else CASES32


def _make(nrows, ncols, rp, ci, va, opts, **kw):
    try:
        return cvr_amd.CvrMatrix(nrows, ncols, rp, ci, va, **dict(opts, **kw))
    except capi.CvrError:          # (a layout the options cannot build for this matrix)
        return None


def _rng(*key):
    return np.random.default_rng([20261017, *key])


class Seen:
    """what a parametrised test must have met: a built case, a row expected non-finite, a non-empty row expected finite, rows cut over chunks"""

    def __init__(self):
        self.built = self.nonfinite = self.finite = self.cut = self.empty = 0

    def handle(self, H):
        self.built += 1
        self.cut += H.info.nshared > 0

    def rows(self, want, rp):
        nz = np.diff(rp) > 0
        self.nonfinite += int(np.any(want != K.FINITE))
        self.finite += int(np.any((want == K.FINITE) & nz))
        self.empty += int(np.any(~nz))

    def check(self, finite=True):
        assert self.built > 0
        assert self.nonfinite > 0, "no case contributed a row expected non-finite"
        if finite:
            assert self.finite > 0, "no case contributed a non-empty row expected finite"
        assert self.cut > 0, "no case with rows cut over chunks"


def _check_rows(y, y0, want, ctx):
    """the class of every row, and the rows classed finite bit for bit those of the run without the poison"""
    got = K.classify(y)
    assert np.array_equal(got, want), (ctx, "rows", np.flatnonzero(got != want)[:8], "got", got[got != want][:8], "want", want[got != want][:8])
    fin = want == K.FINITE
    assert _bits_equal(y[fin], y0[fin]), (ctx, "finite rows differ", np.flatnonzero(fin)[np.flatnonzero(y[fin] != y0[fin])[:8]])


def _containment(H, rp, ci, va, seen, ctx, names=None):
    """test 1 on one handle (rp, ci, va: the CSR of the matrix the handle multiplies by)"""
    x = synth.x_rand(H.ncols).astype(H.dtype)
    for pname, cols, fill in K.poison_patterns(H.nrows, H.ncols, rp, ci, _rng(H.nrows, H.ncols)):
        if names is not None and pname not in names:
            continue
        xp, x0 = K.poisoned(x, cols, fill)
        want = K.expected_class(rp, ci, va, xp)
        y0 = _spmv(H, x0)
        assert np.isfinite(y0).all(), (ctx, pname)
        y = _spmv(H, xp)
        _check_rows(y, y0, want, (ctx, pname))
        assert _bits_equal(_spmv(H, x0), y0), (ctx, pname, "the poisoned run left state behind")
        seen.rows(want, rp)


def _positive(va):
    """no zero value: every term of x = +Inf is +Inf"""
    return (np.abs(va) + va.dtype.type(0.25)).astype(va.dtype)


def _all_poisoned(H, rp, seen, ctx, host=False):
    """test 2 on one handle whose values are all positive: x = +Inf (NaN) everywhere but x_ext[ncols] = 0"""
    nz = np.diff(rp) > 0
    for fillv in (np.inf, np.nan):
        x = np.full(H.ncols, fillv, dtype=H.dtype)
        ys = [_spmv(H, x)] + ([H.spmv(x)[0]] if host else [])          # (the host entry builds x_ext itself)
        for y in ys:
            assert np.isnan(y[nz]).all() if np.isnan(fillv) else np.all(y[nz] == np.inf), (ctx, fillv, np.flatnonzero(nz)[:8])
            assert _bits_equal(y[~nz], np.zeros(int((~nz).sum()), dtype=H.dtype)), (ctx, fillv, "an empty row is not +0.0")
    seen.nonfinite += int(nz.any())
    seen.empty += int((~nz).any())


# ---- 1. containment in x ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_containment_in_x(layout, prec):
    dtype = _dtype(prec)
    seen = Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        A = _make(nrows, ncols, rp, ci, va, ALL_LAYOUTS[layout])
        if A is None:
            continue
        seen.handle(A)
        _containment(A, rp, ci, va, seen, (layout, prec, name))
        A.close()
    seen.check()


# ---- 2. pad slots read only x_ext[ncols] ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_pad_slots_read_only_the_pad_element(layout, prec):
    dtype = _dtype(prec)
    seen = Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        A = _make(nrows, ncols, rp, ci, _positive(va), ALL_LAYOUTS[layout])
        if A is None:
            continue
        seen.handle(A)
        _all_poisoned(A, rp, seen, (layout, prec, name), host=True)
        A.close()
    seen.check(finite=False)          # (every row with a non-zero is Inf / NaN here; the rows that must stay clean are the empty ones)
    assert seen.empty > 0


# ---- 3. non-finite matrix values ----
def _nan_payloads(dtype):
    if dtype == np.float64:
        return np.array([0x7FF8000000000001, 0xFFF8000000000ABC], dtype=np.uint64).view(np.float64)
    return np.array([0x7FC00001, 0xFFC00ABC], dtype=np.uint32).view(np.float32)


def _specials(dtype):
    """NaN, +Inf, -Inf, -0.0, a second NaN of another payload, +0.0"""
    n1, n2 = _nan_payloads(dtype)
    return np.array([n1, np.inf, -np.inf, -0.0, n2, 0.0], dtype=dtype)


def _poison_values(va, rng):
    """(va with about 1 % of its positions -- at least one -- holding the specials in turn, those positions)"""
    out = va.copy()
    if len(va) == 0:
        return out, np.zeros(0, dtype=np.int64)
    pos = np.sort(rng.choice(len(va), size=min(len(va), max(1, len(va) // 100)), replace=False))
    sp = _specials(va.dtype.type)
    out[pos] = sp[np.arange(len(pos)) % len(sp)]
    return out, pos


FEW = np.array([1.0, -1.0, 0.5, 3.0, 1e-3, -7.25, 2.0, 0.25])


def _mirror_of(A, nrows, ncols, rp, ci, va):
    """the CPU mirror of a one-image handle (oraclelib.mirror_of_handle) and the tables to compare; None for column panels or where none is built"""
    if A.info.col_panels != 1:
        return None
    try:
        return O.mirror_of_handle(A.info, A.f32, nrows, ncols, rp, ci, va)
    except RuntimeError:
        return None


def _image_differs_from_mirror(A, nrows, ncols, rp, ci, va):
    m = _mirror_of(A, nrows, ncols, rp, ci, va)
    if m is None:
        return None
    mir, keys = m
    img = A.export_image()
    return [k for k in keys if not _bits_equal(np.asarray(img[k]).reshape(-1), np.asarray(getattr(mir, k)).reshape(-1))]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("values", ["many", "few"])
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_non_finite_matrix_values(layout, values, prec):
    """NaN, +Inf, -Inf, -0.0 (and with few values +0.0 and a second NaN payload) in about 1 % of the positions of the values, x finite: the rows'
    classes, the rows without such a position bit for bit those of the handle of the clean values; many distinct values (no dictionary) and a
    dictionary-sized set, whose image is the mirror's bit for bit"""
    dtype = _dtype(prec)
    seen = Seen()
    dicts = compared = 0
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        rng = _rng(idx, 3)
        if values == "few":
            va = rng.choice(FEW, size=len(va)).astype(dtype)
        vp, pos = _poison_values(va, rng)
        A, B = _make(nrows, ncols, rp, ci, vp, ALL_LAYOUTS[layout]), _make(nrows, ncols, rp, ci, va, ALL_LAYOUTS[layout])
        assert (A is None) == (B is None), (layout, name)
        if A is None:
            continue
        seen.handle(A)
        ctx = (layout, values, prec, name)
        if values == "few":
            assert len(np.unique(vp.view(np.uint64 if dtype == np.float64 else np.uint32))) <= 200
            if layout in ("plain", "default") and len(va):
                assert A.info.value_dict > 0, ctx
        elif len(np.unique(va)) > 256:
            assert A.info.value_dict == 0, ctx
        dicts += A.info.value_dict > 0
        x = synth.x_rand(ncols).astype(dtype)
        want = K.expected_class(rp, ci, vp, x)
        y, y0 = _spmv(A, x), _spmv(B, x)
        assert np.isfinite(y0).all(), ctx
        got = K.classify(y)
        assert np.array_equal(got, want), (ctx, np.flatnonzero(got != want)[:8])
        touched = np.zeros(nrows, dtype=bool)
        touched[np.searchsorted(rp, pos, side="right") - 1] = True
        assert not ((want != K.FINITE) & ~touched).any()          # (a non-finite row owns a poisoned position)
        assert _bits_equal(y[~touched], y0[~touched]), (ctx, "untouched rows differ")
        seen.rows(want, rp)
        if values == "few":
            control = _image_differs_from_mirror(B, nrows, ncols, rp, ci, va)
            diff = _image_differs_from_mirror(A, nrows, ncols, rp, ci, vp)
            if control is not None and diff is not None:
                compared += 1
                assert control == [], (ctx, "the clean image differs from the mirror", control)
                assert diff == [], (ctx, "the poisoned image differs from the mirror", diff)
        A.close()
        B.close()
    seen.check()
    if values == "few":
        assert compared > 0 or ALL_LAYOUTS[layout].get("col_panels", 1) > 1, "no image was compared with the mirror"
        if layout in ("plain", "default"):
            assert dicts > 0


# ---- 4. SpMM: one poisoned vector ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", ["nvec", "plain"])
def test_spmm_one_poisoned_vector(layout, prec):
    """nvec = 2, 5, 8, 11 (one block, a ragged block, two blocks): Inf / NaN in vector j alone -- every other column of Y is bit for bit the clean Y,
    column j has the classes of test 1 and its finite rows are those of the run with the poisoned entries set to 0; once with leading dimensions
    and offsets off the 16-byte grid, so that both the wide and the scalar gather of X run"""
    from test_gpu_spmm import _spmm, _x_block
    dtype = _dtype(prec)
    opts = dict(nvec=4) if layout == "nvec" else dict(K.LAYOUTS["plain"], waves_per_block=1, x_window=0)
    seen = Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        A = _make(nrows, ncols, rp, ci, va, opts)
        assert A is not None and A.spmm_supported, (layout, name)
        seen.handle(A)
        pats = [p for p in K.poison_patterns(nrows, ncols, rp, ci, _rng(idx, 4)) if p[0] in ("last_col", "hot", "random2pct")]
        for k in (2, 5, 8, 11):
            X = _x_block(ncols, k, dtype, k)
            strides = [dict()] + ([dict(ldx=12, ldy=9, xoff=1, yoff=1)] if k == 8 else [])
            for kw in strides:
                clean = _spmm(A, X, fill_y=np.nan, **kw)
                assert np.isfinite(clean).all()
                for pname, cols, fill in pats:
                    for j in sorted({0, k - 1, min(k - 1, 8)}):
                        Xp, X0 = X.copy(), X.copy()
                        Xp[cols, j] = fill.astype(dtype)
                        X0[cols, j] = 0
                        Y, Y0 = _spmm(A, Xp, fill_y=np.nan, **kw), _spmm(A, X0, fill_y=np.nan, **kw)
                        ctx = (layout, prec, name, k, j, pname, kw)
                        others = np.arange(k) != j
                        assert _bits_equal(Y[:, others], clean[:, others]), (ctx, "the poison of one vector reached another")
                        want = K.expected_class(rp, ci, va, Xp[:, j])
                        _check_rows(Y[:, j], Y0[:, j], want, ctx)
                        seen.rows(want, rp)
        A.close()
    seen.check()


# ---- 5. the scaled product ----
SCALED_PAIRS = [(2.5, 0.0), (-0.75, 0.5), (1.0, 1.0)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_scaled_product(layout, prec, monkeypatch):
    """y = alpha A x + beta y: Inf / NaN in a few rows of the y passed in (x finite) make exactly those rows non-finite when beta != 0 -- none when
    beta == 0, y is not read -- and leave every other row bit for bit; Inf / NaN in x give the classes of alpha * s + beta * y with s the plain product
    of the same handle (the formula of test_gpu_spmv_scaled._expect); the fused write-out and CVR_DEBUG=scaled_two_pass agree"""
    from test_gpu_spmv_scaled import _expect, _scaled, _y0
    dtype = _dtype(prec)
    seen = Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        x = synth.x_rand(ncols).astype(dtype)
        pname, cols, fill = [p for p in K.poison_patterns(nrows, ncols, rp, ci, _rng(idx, 5)) if p[0] == "random2pct"][0]
        xp, x0 = K.poisoned(x, cols, fill)
        want_s = K.expected_class(rp, ci, va, xp)
        rows = np.unique(np.array([0, nrows // 2, nrows - 1]))
        forms = {}
        for form in ("fused", "scaled_two_pass"):
            monkeypatch.delenv("CVR_DEBUG", raising=False)
            if form != "fused":
                monkeypatch.setenv("CVR_DEBUG", form)
            A = _make(nrows, ncols, rp, ci, va, ALL_LAYOUTS[layout])
            if A is None:
                break
            if form == "fused":
                seen.handle(A)
            s, s0 = _spmv(A, xp), _spmv(A, x0)
            _check_rows(s, s0, want_s, (layout, prec, name, form, "plain"))
            out = []
            for a, b in SCALED_PAIRS:
                ctx = (layout, prec, name, form, a, b)
                yold = _y0(nrows, dtype, idx)
                ybad = yold.copy()
                ybad[rows] = np.array([np.inf, np.nan, -np.inf], dtype=dtype)[: len(rows)]
                # poisoned y, finite x
                clean = _scaled(A, x, yold, a, b)
                assert np.isfinite(clean).all(), ctx
                y = _scaled(A, x, ybad, a, b)
                hit = np.zeros(nrows, dtype=bool)
                hit[rows] = b != 0
                assert np.array_equal(~np.isfinite(y), hit), (ctx, np.flatnonzero(~np.isfinite(y) != hit)[:8])
                assert _bits_equal(y[~hit], clean[~hit]), ctx
                if b != 0:
                    assert np.array_equal(K.classify(y[rows]), K.classify(_expect(s0, ybad, a, b, dtype)[rows])), ctx
                # poisoned x, finite y
                y = _scaled(A, xp, yold, a, b)
                want = K.classify(_expect(s, yold, a, b, dtype))
                _check_rows(y, _scaled(A, x0, yold, a, b), want, ctx)
                assert np.array_equal(want != K.FINITE, want_s != K.FINITE), ctx
                out.append(y)
            forms[form] = out
            seen.rows(want_s, rp)
            A.close()
        if len(forms) == 2:
            for (a, b), yf, yt in zip(SCALED_PAIRS, forms["fused"], forms["scaled_two_pass"]):
                assert np.array_equal(K.classify(yf), K.classify(yt)), (layout, prec, name, a, b)
                fin = np.isfinite(yf)
                assert _bits_equal(yf[fin], yt[fin]), (layout, prec, name, a, b)
    seen.check()


# ---- 6. cvr_update_values copies bits ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_update_values_copies_bits(layout, prec):
    """a mutable handle updated to values that hold two NaN payloads, +Inf, -Inf, -0.0 and explicit +0.0: the image, bit for bit, of a fresh mutable
    handle created with those values (interleaved images leave the steal targets and may leave gang tables unwritten, as test_gpu_update_values.py
    explains: those two tables are not compared), and the classes of y.  Column panels export no image: there the copy is checked through y alone
    (classes, and bits against the fresh handle), which cannot show a NaN payload or the sign of a zero -- the bit-for-bit check is that of the
    single-image layouts."""
    from test_gpu_update_values import _diff_keys
    dtype = _dtype(prec)
    seen = Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        v2, pos = _poison_values((np.random.default_rng(idx).random(len(va)) * 4 - 2).astype(dtype), _rng(idx, 6))
        A = _make(nrows, ncols, rp, ci, va, ALL_LAYOUTS[layout], mutable_values=1)
        if A is None:
            continue
        seen.handle(A)
        ctx = (layout, prec, name)
        A.update_values(v2)
        B = cvr_amd.CvrMatrix(nrows, ncols, rp, ci, v2, mutable_values=1, **ALL_LAYOUTS[layout])
        assert not (_diff_keys(A, B) - ({"target", "gbase"} if A.info.interleave else set())), ctx
        x = synth.x_rand(ncols).astype(dtype)
        want = K.expected_class(rp, ci, v2, x)
        y, yb = _spmv(A, x), _spmv(B, x)
        _check_rows(y, yb, want, ctx)
        assert np.array_equal(K.classify(yb), want), ctx
        seen.rows(want, rp)
        A.close()
        B.close()
    seen.check()


# ---- 7. transposed and cached handles ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", ["default", "panels"])
def test_transposed_handles(layout, prec):
    from test_gpu_transpose import stable_transpose
    dtype = _dtype(prec)
    seen, seen2 = Seen(), Seen()
    todo = dict(_cases(dtype))
    # The transposes of the seeded cases have rows of at most 75 entries, below the split threshold of every chunk length from 5 steps on (16 entries
    # per step): none has a row cut over chunks.  One more matrix, whose transpose is dense_row_plus_singletons with its row of 20 000 entries.
    n0, m0, rp0, ci0, va0 = todo["dense_row_plus_singletons"]
    todo["hot_column"] = stable_transpose(n0, m0, rp0, ci0, va0)[:5]
    for name, (nrows, ncols, rp, ci, va) in todo.items():
        tn, tm, trp, tci, tva, _ = stable_transpose(nrows, ncols, rp, ci, va)
        H = _make(nrows, ncols, rp, ci, va, ALL_LAYOUTS[layout], transpose=1)
        if H is not None:
            assert (H.nrows, H.ncols) == (tn, tm)
            seen.handle(H)
            _containment(H, trp, tci, tva, seen, (layout, prec, name, "transpose"))
            H.close()
        P = _make(nrows, ncols, rp, ci, _positive(va), ALL_LAYOUTS[layout], transpose=1)
        if P is not None:
            seen2.handle(P)
            _all_poisoned(P, trp, seen2, (layout, prec, name, "transpose"))
            P.close()
    seen.check()
    seen2.check(finite=False)
    assert seen2.empty > 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", ["default", "hub_reorder", "gang"])
def test_cached_handles(layout, prec, tmp_path):
    dtype = _dtype(prec)
    seen, seen2 = Seen(), Seen()
    for idx, (name, (nrows, ncols, rp, ci, va)) in enumerate(_cases(dtype).items()):
        for vals, which in ((va, 1), (_positive(va), 2)):
            A = _make(nrows, ncols, rp, ci, vals, ALL_LAYOUTS[layout])
            if A is None:
                continue
            path = str(tmp_path / f"{name}_{which}.cvr")
            A.save_image(path)
            A.close()
            H = cvr_amd.CvrMatrix.from_image(path, **ALL_LAYOUTS[layout])
            ctx = (layout, prec, name, "cached")
            if which == 1:
                seen.handle(H)
                _containment(H, rp, ci, va, seen, ctx)
            else:
                seen2.handle(H)
                _all_poisoned(H, rp, seen2, ctx)
            H.close()
    seen.check()
    seen2.check(finite=False)
    assert seen2.empty > 0


# ---- 8. conjugate gradients ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", ["default", "panels"])
def test_cg_breaks_down_on_non_finite_data(layout, prec):
    """a NaN or an Inf in b, or a NaN among A's values (b finite): p . q of step 0 is not finite -- CVR_CG_BREAKDOWN at iterations == 0, x bit for bit
    the start vector, whatever check_every; the call returns instead of running on to max_iters"""
    from test_gpu_cg import MAX_ITERS, RTOL, _solve, _spd
    dtype = _dtype(prec)
    n, _, rp, ci, va = _spd("rmat", dtype)
    b = synth.x_rand(n).astype(dtype)
    x0 = (np.random.default_rng(5).random(n) * 2 - 1).astype(dtype)
    at = n // 3
    b_nan, b_inf = b.copy(), b.copy()
    b_nan[at] = np.nan
    b_inf[at] = np.inf
    va_nan = va.copy()
    va_nan[int(rp[at]) + (int(rp[at + 1]) - int(rp[at])) // 2] = np.nan
    A = _make(n, n, rp, ci, va, ALL_LAYOUTS[layout])
    N = _make(n, n, rp, ci, va_nan, ALL_LAYOUTS[layout])
    assert A is not None and N is not None
    for H, rhs, what in ((A, b_nan, "NaN in b"), (N, b, "NaN in A"), (A, b_inf, "+Inf in b")):
        for start in (x0, None):
            for every in (1, 8):
                x, res = _solve(H, rhs, x0=start, rtol=RTOL[dtype], max_iters=MAX_ITERS, check_every=every)
                ctx = (layout, prec, what, "zero start" if start is None else "random start", every)
                assert res.status == capi.CG_BREAKDOWN and res.iterations == 0, (ctx, res.status, res.iterations)
                assert _bits_equal(x, np.zeros(n, dtype=dtype) if start is None else start), ctx
                assert res.spmv_count <= 1 + every, (ctx, res.spmv_count)          # (it returned at the first check, not at max_iters)
    # the clean system still converges on the same handle afterwards
    x, res = _solve(A, b, rtol=RTOL[dtype], max_iters=MAX_ITERS)
    assert res.status == capi.CG_CONVERGED and np.isfinite(x).all()
    A.close()
    N.close()
