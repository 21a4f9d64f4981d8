"""CPU: tests/fsai_model.py against dense linear algebra -- the model the host twin and the device set-up are pinned to is an FSAI factor, and
conjugate gradients with it need fewer steps."""
import numpy as np
import pytest

import fsai_model as FM
import krylov_model as KM
from cvr_amd import synth


def _dense_w(n, wrp, wci, w):
    return FM.dense(n, wrp, wci, w)


CASES = {
    "laplacian-24": lambda: synth.laplacian_2d(24),
    "spd-65": lambda: KM.banded("spd", 65, np.float64),
    "dense-8": lambda: FM.dense_spd(8, np.float64),
    "dense-32": lambda: FM.dense_spd(32, np.float64),
    "dense-40": lambda: FM.dense_spd(40, np.float64),
    "arrow-100": lambda: FM.arrow(100, np.float64),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_is_an_fsai_factor(name):
    n, _, rp, ci, va = CASES[name]()
    A = FM.dense(n, rp, ci, va)
    assert np.array_equal(A, A.T) or np.allclose(A, A.T, rtol=0, atol=1e-15)
    assert np.linalg.eigvalsh(A).min() > 0
    wrp, wci, wa, wb, bad = FM.factor(rp, ci, va, np.float64)
    assert bad is None
    Wa, Wb = _dense_w(n, wrp, wci, wa), _dense_w(n, wrp, wci, wb)
    assert np.array_equal(np.diag(Wa), np.ones(n)) and np.array_equal(Wa, np.tril(Wa))
    M = Wb.T @ Wa
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()          # Wb = D^-1 Wa: symmetric to rounding
    assert np.abs(np.diag(Wa @ A @ Wb.T) - 1).max() <= 1e-12           # the Kolotilina-Yeremin scaling
    _, _, _, max_row, truncated = FM.pattern(rp, ci)
    assert max_row == min(max(np.sum(ci[rp[i]: rp[i + 1]] <= i) for i in range(n)), FM.MAX_ROW)
    assert truncated == {"dense-40": 8, "arrow-100": 1}.get(name, 0)
    assert FM.lanes(max_row) == {"laplacian-24": 4, "spd-65": 4, "dense-8": 8, "dense-32": 32, "dense-40": 32, "arrow-100": 32}[name]


@pytest.mark.parametrize("n", [1, 2, 8, 32])
def test_dense_spd_up_to_32_is_inverted_exactly(n):
    _, _, rp, ci, va = FM.dense_spd(n, np.float64)
    wrp, wci, wa, wb, bad = FM.factor(rp, ci, va, np.float64)
    assert bad is None
    M = _dense_w(n, wrp, wci, wb).T @ _dense_w(n, wrp, wci, wa)
    assert np.abs(M @ FM.dense(n, rp, ci, va) - np.eye(n)).max() <= 1e-10


def test_the_apply_is_the_two_products():
    n, _, rp, ci, va = synth.laplacian_2d(7)
    wrp, wci, wa, wb, _ = FM.factor(rp, ci, va, np.float64)
    pa, pbt = FM.cpu_products(n, wrp, wci, wa, wb, np.float64)
    r = KM.inputs(n, np.float64)[0]
    want = _dense_w(n, wrp, wci, wb).T @ (_dense_w(n, wrp, wci, wa) @ r)
    assert np.abs(FM.apply(pa, pbt, r) - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("m", [24, 40])
def test_pcg_needs_at_most_two_thirds_of_cgs_iterations(m):
    """measured with this model: 44 of 77 on the 24 x 24 grid, 72 of 125 on the 40 x 40 one"""
    n, _, rp, ci, va = synth.laplacian_2d(m)
    wrp, wci, wa, wb, bad = FM.factor(rp, ci, va, np.float64)
    assert bad is None
    product = FM.csr_product(n, rp, ci, va, np.float64)
    pa, pbt = FM.cpu_products(n, wrp, wci, wa, wb, np.float64)
    b = KM.inputs(n, np.float64)[0]
    plain = KM.CgModel(product, np.float64).run(b, None, None, rtol=1e-8, max_iters=400).last
    pre = FM.FsaiPcg(product, np.float64, pa, pbt).run(b, None, rtol=1e-8, max_iters=400).last
    print(f"laplacian_2d({m}): FSAI-PCG {pre.iterations} steps, CG {plain.iterations}")
    assert plain.terminal and pre.terminal and plain.status == KM.CONVERGED and pre.status == KM.CONVERGED
    assert 3 * pre.iterations <= 2 * plain.iterations


def test_bad_pivots():
    n, _, rp, ci, va = KM.banded("spd", 10, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    neg = va.copy()
    neg[d[0]] = -1.0
    assert FM.factor(rp, ci, neg, np.float64)[4] == 0          # a negative diagonal: row 0's own pivot
    for v in (0.0, np.nan, np.inf):
        broken = va.copy()
        broken[d[4]] = v
        wrp, wci, wa, wb, bad = FM.factor(rp, ci, broken, np.float64)
        assert bad == 4 and not wa[wrp[4]:].any() and np.isfinite(wa).all(), v          # the lowest row that meets it: its own
    # indefinite without a bad diagonal: the 2 x 2 system of row 1 has the pivot 1 - 2 * 2 < 0
    wrp, wci, wa, wb, bad = FM.factor(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 2.0, 1.0]), np.float64)
    assert bad == 1
