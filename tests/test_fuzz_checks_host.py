"""No GPU: the pieces tests/test_gpu_fuzz_derived.py rests on, before it meets a device.

  * cases.random_case is the generator test_gpu_fuzz.py always had: a digest of its first cases, recorded from the function as it stood in that
    file, for the seeds of its two loops
  * fuzz_checks.stable_transpose against a dense numpy transposition
  * every checker of fuzz_checks.py rejects a subtly wrong result -- an unstable transposition, a row off by one, a stale or exchanged value after an
    update, a fused or wrongly rounded scaled product, exchanged SpMM columns, a sentinel overwritten -- on generated matrices, a rectangular one
    with duplicates and empty columns among them; the CPU mirror of the format (oraclelib.Cvr64) stands in for the handle's image, the CSR oracle
    rounded to the type for its product
  * the coverage conditions of the fuzz's default seeds and counts, which depend on the generator alone
"""
import hashlib
from fractions import Fraction

import numpy as np
import pytest

import cases as K
import fuzz_checks as FC
import oraclelib as O

PARENT_DIGEST = {20261002: "5332f3476ce358f39bf9c4d579a3cf17b75cc964f762bb84111195e2f9544b55",
                 20261006: "dd55debf2517494832cb08ff277153f57de6590efc28d56f1fccfc761079f738"}


@pytest.mark.parametrize("seed", sorted(PARENT_DIGEST))
def test_random_case_draws_what_the_fuzz_always_drew(seed):
    """sha256 over (nrows, ncols, sorted) as int64 and the bytes of row_ptr, col_idx, vals of the first 8 cases"""
    rng = np.random.default_rng(seed)
    h = hashlib.sha256()
    for _ in range(8):
        nrows, ncols, rp, ci, va, srt = K.random_case(rng)
        h.update(np.int64([nrows, ncols, int(srt)]).tobytes())
        for a in (rp, ci, va):
            h.update(a.tobytes())
    assert h.hexdigest() == PARENT_DIGEST[seed]


def test_max_nnz_bounds_the_case_and_keeps_the_shapes():
    rng = np.random.default_rng(5)
    shapes = []
    for _ in range(40):
        nrows, ncols, rp, ci, va, srt = K.random_case(rng, max_nnz=100_000)
        assert len(rp) == nrows + 1 and rp[0] == 0 and rp[-1] == len(ci) == len(va) <= 100_000
        assert 1 <= nrows < 4000 and 1 <= ncols < 6000
        shapes.append((nrows, ncols))
    assert max(s[0] for s in shapes) > 2048 and max(s[1] for s in shapes) > 4096          # (the window edges stay inside the shapes)


def test_random_options_keeps_the_guards():
    rng = np.random.default_rng(7)
    seen = dict(default=0, plain=0, ilv=0)
    for i in range(800):
        ncols, srt = int(rng.integers(1, 6000)), bool(rng.integers(0, 2))
        o = K.random_options(rng, ncols, srt)
        if not o:
            seen["default"] += 1
            continue
        if o.get("interleave"):
            seen["ilv"] += 1
            assert o["steps_per_chunk"] <= 508 and "col_phases" not in o and "hub_table" not in o
            continue
        seen["plain"] += 1
        if o["col_phases"] > 1:
            assert srt and ncols >= 320 and o["col_panels"] == 1 and o["hub_table"] == 0
        else:
            assert o["row_tags16"] == -1 and o["piece_max"] == -1
        if o["hub_reorder"]:
            assert o["hub_table"] > 0 and o["col_panels"] == 1
    assert 60 <= seen["default"] <= 140 and seen["plain"] > 300 and seen["ilv"] > 200, seen


# ---- the matrices the wrong results are made on ----
def _rect_with_duplicates(dtype):
    """37 x 90, unsorted rows, every entry of rows 3 and 20 twice (different values), columns 60 .. 89 empty, row_ptr[0] = 0"""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 9, size=37)
    lens[3], lens[20] = 6, 8
    nrows, ncols, rp, ci, va = K.csr_from_lengths(lens, 60, rng, dtype, sort=False)
    for r in (3, 20):
        h = (rp[r + 1] - rp[r]) // 2
        ci[rp[r] + h: rp[r] + 2 * h] = ci[rp[r]: rp[r] + h]
    return nrows, 90, rp, ci, va


def _generated(dtype):
    out = [_rect_with_duplicates(dtype)]
    rng = np.random.default_rng(20261020)
    while len(out) < 4:
        nrows, ncols, rp, ci, va, srt = K.random_case(rng, max_nnz=20_000)
        if len(ci) >= 64:
            out.append((nrows, ncols, rp, ci, va.astype(dtype)))
    return out


MATRICES = {np.float64: _generated(np.float64), np.float32: _generated(np.float32)}
IDS = ["rect_dup_empty", "gen1", "gen2", "gen3"]


def _duplicate_pair(nrows, ncols, rp, ci, va):
    """positions p < q of two entries of one row and one column whose values differ"""
    for r in range(nrows):
        seen = {}
        for p in range(int(rp[r]), int(rp[r + 1])):
            q = seen.setdefault(int(ci[p]), p)
            if q != p and va[q] != va[p]:
                return q, p
    raise AssertionError("no duplicate pair")


def _product(rp, ci, va, x):
    """the CSR oracle's y rounded to the type: what stands for a handle's plain product on the CPU"""
    return O.csr_spmv64(rp, ci, va, x.astype(va.dtype))[0].astype(va.dtype)


def _rejects(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ---- transpose ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stable_transpose_is_the_dense_transposition(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rng = np.random.default_rng(3)
    for nrows, ncols, lens, srt, off in ((1, 1, [1], True, 0), (5, 3, [0, 2, 3, 0, 1], False, 0), (4, 9, [9, 0, 0, 4], True, 5), (12, 7, None, False, 3), (1, 40, [17], False, 0)):
        lens = rng.integers(0, 6, size=nrows) if lens is None else lens
        n, m, rp, ci, va = K.csr_from_lengths(lens, ncols, rng, dtype, sort=srt)
        va = np.arange(1, len(va) + 1).astype(dtype)          # distinct values: the order inside a row of A^T shows
        rp, ci, va = rp + off, np.concatenate([np.full(off, ncols - 1, np.int32), ci]), np.concatenate([np.full(off, np.nan, dtype), va])
        tn, tm, trp, tci, tva, pos = FC.stable_transpose(n, m, rp, ci, va)
        assert (tn, tm) == (m, n) and trp[0] == 0 and trp[-1] == len(tci) == len(tva) == rp[-1] - rp[0]
        D = np.zeros((n, m))
        rows = np.repeat(np.arange(n), np.diff(rp))
        np.add.at(D, (rows, ci[off:]), va[off:].astype(np.float64))
        DT = np.zeros((m, n))
        np.add.at(DT, (np.repeat(np.arange(m), np.diff(trp)), tci), tva.astype(np.float64))
        assert np.array_equal(DT, D.T)
        assert np.array_equal(va[pos], tva)
        for j in range(m):          # row j of A^T: A's entries of column j in ascending CSR position
            p = pos[trp[j]:trp[j + 1]]
            assert np.all(np.diff(p) > 0) and np.all(ci[p] == j)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", range(4), ids=IDS)
def test_a_wrong_transposition_is_rejected(which, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = MATRICES[dtype][which]
    tn, tm, trp, tci, tva, pos = FC.stable_transpose(nrows, ncols, rp, ci, va)
    right = FC.image_of_mirror(tn, tm, trp, tci, tva)
    FC.assert_same_image(FC.image_of_mirror(tn, tm, trp, tci, tva), right)
    x = (np.random.default_rng(1).random(nrows) * 2 - 1).astype(dtype)
    FC.assert_transposed_product(_product(trp, tci, tva, x), nrows, ncols, rp, ci, va, x)
    # an unstable sort: the two duplicates of one (row, column) of A exchanged inside the row of A^T
    p, q = _duplicate_pair(nrows, ncols, rp, ci, va)
    ip, iq = int(np.flatnonzero(pos == p)[0]), int(np.flatnonzero(pos == q)[0])
    assert tci[ip] == tci[iq] and np.searchsorted(trp, ip, side="right") == np.searchsorted(trp, iq, side="right")
    uva = tva.copy()
    uva[ip], uva[iq] = tva[iq], tva[ip]
    assert _rejects(FC.assert_same_image, FC.image_of_mirror(tn, tm, trp, tci, uva), right)
    # one element's row off by one (a neighbouring row of A^T takes it)
    j = int(np.flatnonzero(np.diff(trp) > 0)[0])
    wrp = trp.copy()
    if j + 1 < tn:
        wrp[j + 1] -= 1          # row j loses its last element to row j + 1
    else:
        wrp[j] += 1              # (the last row: its first element goes to the row before)
    assert _rejects(FC.assert_same_image, FC.image_of_mirror(tn, tm, wrp, tci, tva), right)
    xs = np.arange(1, nrows + 1).astype(dtype)          # (no cancellation: the misplaced term shows in two rows)
    va1 = (np.abs(va) + dtype(0.5)).astype(dtype)
    _, _, _, _, tva1, _ = FC.stable_transpose(nrows, ncols, rp, ci, va1)
    FC.assert_transposed_product(_product(trp, tci, tva1, xs), nrows, ncols, rp, ci, va1, xs)
    assert _rejects(FC.assert_transposed_product, _product(wrp, tci, tva1, xs), nrows, ncols, rp, ci, va1, xs)


# ---- value updates ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", range(4), ids=IDS)
def test_a_wrong_update_is_rejected(which, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, v1 = MATRICES[dtype][which]
    rng = np.random.default_rng(2)
    v2 = (rng.random(len(v1)) * 4 - 2).astype(dtype)
    fresh = FC.image_of_mirror(nrows, ncols, rp, ci, v2)
    FC.assert_same_image(FC.image_of_mirror(nrows, ncols, rp, ci, v2.copy()), fresh)
    x = (rng.random(ncols) * 2 - 1).astype(dtype)
    for slot in (0, len(v1) // 2, len(v1) - 1):
        stale = v2.copy()
        stale[slot] = v1[slot]          # one slot keeps its old value
        assert _rejects(FC.assert_same_image, FC.image_of_mirror(nrows, ncols, rp, ci, stale), fresh), slot
        assert not FC._bits_equal(_product(rp, ci, stale, x), _product(rp, ci, v2, x))
    a, b = len(v1) // 3, len(v1) // 3 + 1
    swapped = v2.copy()
    swapped[a], swapped[b] = v2[b], v2[a]          # two slots exchanged
    assert _rejects(FC.assert_same_image, FC.image_of_mirror(nrows, ncols, rp, ci, swapped), fresh)
    # the allowance of interleaved images covers `target` and `gbase` alone, never the stream
    assert _rejects(FC.assert_same_image, FC.image_of_mirror(nrows, ncols, rp, ci, stale), fresh, interleave=True, loose={"gbase"})
    assert _rejects(FC.assert_same_image, fresh, fresh, interleave=False, loose={"target"})
    assert _rejects(FC.assert_same_image, fresh, fresh, interleave=True, loose={"image"})
    other = dict(fresh, target=fresh["target"] + 1)
    FC.assert_same_image(other, fresh, interleave=True)
    assert _rejects(FC.assert_same_image, other, fresh)


# ---- the scaled product ----
def _fma(a, s, t, dtype):
    """a * s + t with one rounding, element by element (exact rational arithmetic, rounded to the type once)"""
    out = np.empty(len(s), dtype=dtype)
    fa = Fraction(float(a))
    for i in range(len(s)):
        v = fa * Fraction(float(s[i])) + Fraction(float(t[i]))
        if dtype == np.float64:
            out[i] = float(v)
        else:          # round the exact value to fp32 once: fp64 first would round twice
            f = np.float32(float(v))
            lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
            out[i] = min((lo, f, hi), key=lambda c: abs(Fraction(float(c)) - v))
    return out


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", range(4), ids=IDS)
def test_a_wrong_scaled_product_is_rejected(which, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = MATRICES[dtype][which]
    rng = np.random.default_rng(4)
    x = (rng.random(ncols) * 2 - 1).astype(dtype)
    s = _product(rp, ci, va, x)
    s = np.concatenate([s[s != 0][:400], s[s == 0][:4]])          # (rows with a product, and a few empty ones)
    n = len(s)
    assert n >= 20
    y0 = (rng.random(n) * 4 - 2).astype(dtype)
    y0[n // 2] = -0.0
    alpha, beta = FC._unrepresentable(rng), FC._unrepresentable(rng)
    a, b = dtype(alpha), dtype(beta)
    FC.assert_scaled(FC._expect(s, y0, alpha, beta, dtype), s, y0, alpha, beta, dtype)
    # a fused multiply-add in place of two rounded products and a rounded sum
    fused = _fma(a, s, (b * y0).astype(dtype), dtype)
    assert (fused.view(FC.dtype_bits(dtype)) != FC._expect(s, y0, alpha, beta, dtype).view(FC.dtype_bits(dtype))).any(), "the fused form does not differ here"
    assert _rejects(FC.assert_scaled, fused, s, y0, alpha, beta, dtype)
    # beta = 0 that reads y
    nan = np.full(n, np.nan, dtype=dtype)
    with np.errstate(all="ignore"):
        read = (a * s + dtype(0) * nan).astype(dtype)
    assert _rejects(FC.assert_scaled, read, s, nan, alpha, 0.0, dtype)
    FC.assert_scaled((a * s).astype(dtype), s, nan, alpha, 0.0, dtype)
    # alpha = 0 that reads s
    with np.errstate(all="ignore"):
        assert _rejects(FC.assert_scaled, (dtype(0) * nan + b * y0).astype(dtype), nan, y0, 0.0, beta, dtype)
    FC.assert_scaled((b * y0).astype(dtype), nan, y0, 0.0, beta, dtype)
    if dtype == np.float32:
        # alpha and beta not rounded to fp32 first
        late = (np.float64(alpha) * s.astype(np.float64)).astype(np.float32)
        assert _rejects(FC.assert_scaled, late, s, nan, alpha, 0.0, dtype)
        late2 = ((np.float64(alpha) * s.astype(np.float64)).astype(np.float32) + (np.float64(beta) * y0.astype(np.float64)).astype(np.float32)).astype(np.float32)
        assert _rejects(FC.assert_scaled, late2, s, y0, alpha, beta, dtype)


# ---- SpMM ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("which", range(4), ids=IDS)
def test_a_wrong_spmm_block_is_rejected(which, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    nrows, ncols, rp, ci, va = MATRICES[dtype][which]
    rng = np.random.default_rng(6)
    k, ldy, scratch = 5, 8, 3
    X = (rng.random((ncols, k)) * 2 - 1).astype(dtype)
    cols = np.stack([_product(rp, ci, va, X[:, j]) for j in range(k)], axis=1)
    Yall = np.full((nrows + scratch, ldy), FC.SENTINEL, dtype=dtype)
    Yall[:nrows, :k] = cols
    Yall[nrows:, :k] = 123.0          # (scratch rows: the kernel may write their first k positions)
    FC.assert_spmm_block(Yall, nrows, k, cols)
    for j in (0, k - 2):          # columns j and j + 1 exchanged
        W = Yall.copy()
        W[:, [j, j + 1]] = Yall[:, [j + 1, j]]
        assert _rejects(FC.assert_spmm_block, W, nrows, k, cols), j
    for r, c in ((0, k), (nrows - 1, ldy - 1), (nrows + scratch - 1, k)):          # a sentinel beyond nvec overwritten: first row, last row, a scratch row
        W = Yall.copy()
        W[r, c] = 0.0
        assert _rejects(FC.assert_spmm_block, W, nrows, k, cols), (r, c)
    W = Yall.copy()
    W[nrows // 2, 1] = np.nan
    assert _rejects(FC.assert_spmm_block, W, nrows, k, cols)
    # and the oracle check of a column: one term dropped from the longest row
    r = int(np.argmax(np.diff(rp)))
    y = cols[:, 0].copy()
    FC.assert_oracle(y, rp, ci, va, X[:, 0])
    p = int(rp[r]) + int(np.argmax(np.abs(va[rp[r]:rp[r + 1]].astype(np.float64) * X[ci[rp[r]:rp[r + 1]], 0])))
    y[r] -= va[p] * X[ci[p], 0]
    assert _rejects(FC.assert_oracle, y, rp, ci, va, X[:, 0])


# ---- what the default seeds and counts reach ----
def test_the_default_cases_cover_what_the_fuzz_is_for(monkeypatch):
    monkeypatch.delenv("CVR_FUZZ_SEED", raising=False)
    monkeypatch.delenv("CVR_FUZZ_CASES", raising=False)
    derived, spmm = FC.all_cases()
    assert len(derived) == len(spmm) == FC.BLOCKS * FC.CASES_PER_BLOCK == 48
    got = FC.coverage(derived, spmm)
    print(got)
    for name, least in FC.COVERAGE_MIN.items():
        assert got[name] >= least, (name, got[name], least)
    # the draws of the cases themselves
    for c in derived:
        assert len(c.pairs) == 4 and all(float(np.float32(v)) != v for p in c.pairs[2:] for v in p) and all(p in FC.FIXED_PAIRS for p in c.pairs[:2])
        assert c.v2.dtype == c.v3.dtype == c.va.dtype == c.dtype and len(c.xt) == c.nrows and len(c.x) == c.ncols
    assert 8 <= sum(c.transposed_update for c in derived) <= 24
    for c in spmm:
        assert 1 <= c.k <= 16 and c.k <= c.ldx <= c.k + 5 and c.k <= c.ldy <= c.k + 5 and 0 <= c.xoff <= 3 and 0 <= c.yoff <= 3
    assert 6 <= sum(c.mutable for c in spmm) <= 20
    assert {c.nvec for c in spmm} == {2, 3, 4, 8, 16} and {c.S for c in spmm} == {4, 8, 16, 32, 64} and {c.thr for c in spmm} == {0, 1, 7, 16, 64, 10**6}
