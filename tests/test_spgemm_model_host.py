"""CPU: tests/spgemm_model.py, the definition of C = A B's bits, against dense fp64 products and scipy.sparse: exactly the structural pattern, and
every value within the standard summation bound gamma = (t + 1) * eps * sum |a| |b| of an entry of t terms (one rounding per product, one per
addition, the input's own rounding none: the operands are the stored values)."""
import numpy as np
import pytest

import spgemm_model as SM


def _eps(dtype):
    return float(np.finfo(dtype).eps)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", SM.CASE_NAMES + ["collisions-8"])
def test_the_model_against_the_dense_product(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    a, b = SM.named(name, dtype)
    c = SM.spgemm(a, b)
    assert c.rp[0] == 0 and len(c.rp) == a.nrows + 1 and c.rp[-1] == len(c.ci) == len(c.va) and c.va.dtype == dtype
    # the structural pattern: that of |A| |B| with every value replaced by 1
    ones_a, ones_b = SM.Csr(a.nrows, a.ncols, a.rp, a.ci, np.ones(len(a.ci))), SM.Csr(b.nrows, b.ncols, b.rp, b.ci, np.ones(len(b.ci)))
    pattern = ones_a.dense() @ ones_b.dense() if a.nrows and b.ncols else np.zeros((a.nrows, b.ncols))
    want = a.dense() @ b.dense() if a.nrows and b.ncols else np.zeros((a.nrows, b.ncols))
    for i in range(a.nrows):
        cols = c.ci[c.rp[i]: c.rp[i + 1]]
        assert (np.diff(cols.astype(np.int64)) > 0).all(), (name, i)
        assert np.array_equal(cols, np.flatnonzero(pattern[i])), (name, i)
        terms = c.terms[c.rp[i]: c.rp[i + 1]]
        assert np.array_equal(terms, pattern[i][cols].astype(np.int64)), (name, i)
        got = c.va[c.rp[i]: c.rp[i + 1]].astype(np.float64)
        bound = (terms + 1) * _eps(dtype) * c.absum[c.rp[i]: c.rp[i + 1]]
        assert (np.abs(got - want[i][cols]) <= bound).all(), (name, i, np.abs(got - want[i][cols]).max())
    assert np.array_equal(SM.products(a, b), (ones_a.dense() @ np.diff(b.rp).astype(np.float64)).astype(np.int64) if a.nrows else np.zeros(0, dtype=np.int64))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["banded-65", "laplacian-24", "rect-7x130x5", "a-empty-rows", "b-empty-rows", "dense-row"])
def test_the_model_against_scipy(name, prec):
    sp = pytest.importorskip("scipy.sparse")
    dtype = np.float64 if prec == "fp64" else np.float32
    a, b = SM.named(name, dtype)
    c = SM.spgemm(a, b)
    sa = sp.csr_matrix((a.va.astype(np.float64), a.ci, a.rp), shape=(a.nrows, a.ncols))
    sb = sp.csr_matrix((b.va.astype(np.float64), b.ci, b.rp), shape=(b.nrows, b.ncols))
    s = (sa @ sb).tocsr()
    s.sort_indices()
    # (seeded values of magnitude 0.5 .. 1.5: no entry of these cases cancels to zero, so scipy's pattern is the structural one)
    assert np.array_equal(s.indptr, c.rp) and np.array_equal(s.indices, c.ci), name
    assert (np.abs(c.va.astype(np.float64) - s.data) <= (c.terms + 1) * _eps(dtype) * c.absum).all(), name


def test_a_cancelling_entry_stays():
    for dtype in (np.float64, np.float32):
        a = SM.Csr(1, 2, [0, 2], [0, 1], np.array([1, -1], dtype=dtype))
        b = SM.Csr(2, 1, [0, 1, 2], [0, 0], np.array([1, 1], dtype=dtype))
        c = SM.spgemm(a, b)
        assert list(c.rp) == [0, 1] and list(c.ci) == [0] and c.va[0] == 0.0 and not np.signbit(c.va[0]) and c.terms[0] == 2


def test_the_sum_runs_in_ascending_p_and_rounds_each_step():
    # 1 + 2^-24 + 2^-24 in fp32: left to right both small terms are lost; any other order keeps 2^-23
    t = np.float32(2.0 ** -24)
    a = SM.Csr(1, 3, [0, 3], [2, 0, 1], np.array([1, 1, 1], dtype=np.float32))
    b = SM.Csr(3, 1, [0, 1, 2, 3], [0, 0, 0], np.array([t, t, 1], dtype=np.float32))
    assert SM.spgemm(a, b).va[0] == np.float32(1.0)
    a = SM.Csr(1, 3, [0, 3], [0, 1, 2], np.array([1, 1, 1], dtype=np.float32))
    assert SM.spgemm(a, b).va[0] == np.float32(1.0) + np.float32(2.0 ** -23)


def test_the_row_classes():
    assert SM.row_classes([0, 1, 31, 32, 4095, 4096, 10 ** 7]) == (1, 2, 2, 2)
    assert SM.row_classes([0, 1, 7, 8, 63, 64], 8, 64) == (1, 2, 2, 1)
    assert SM.row_classes([0, 1, 2], 1, 1) == (1, 0, 0, 2)
