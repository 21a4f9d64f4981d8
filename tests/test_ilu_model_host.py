"""CPU: tests/ilu_model.py itself -- the numpy model of cvr_precond_ilu0 that the GPU tests compare the device with.

  * banded "spd" and "nonsym" have no fill, so ILU(0) is LU: ||L U - A||_max <= 4 eps ||A||_max
  * the 24 x 24 Laplacian has 47 levels each way and its widest level has 24 rows
  * model PCG in fp64 on the 24 x 24 and 40 x 40 Laplacians needs at most half of plain CG's iterations
  * the pieces: the butterfly is krylov_model's on zero-padded lanes, the plan, G, the transposed pattern"""
import numpy as np
import pytest

import ilu_model as IM
import krylov_model as KM
import precond_model as PM
from cvr_amd import synth


@pytest.mark.parametrize("kind", ["spd", "nonsym"])
@pytest.mark.parametrize("n", [1, 2, 65, 200])
def test_banded_has_no_fill_so_the_factor_is_exact(kind, n):
    _, _, rp, ci, va = KM.banded(kind, n, np.float64)
    f, bad = IM.factor(rp, ci, va, np.float64)
    assert bad is None
    L, U = IM.dense_lu(n, rp, ci, f)
    A = PM.dense_of(n, rp, ci, va)
    err, scale = np.abs(L @ U - A).max(), np.abs(A).max()
    print(f"{kind} n = {n}: ||L U - A||_max = {err:.3g}, ||A||_max = {scale:.3g}")
    assert err <= 4 * np.finfo(np.float64).eps * scale


def test_levels_of_the_laplacian():
    m = 24
    n, _, rp, ci, _ = synth.laplacian_2d(m)
    lo, up, nlo, nup = IM.levels(rp, ci)
    assert (nlo, nup) == (2 * m - 1, 2 * m - 1) == (47, 47)
    i, j = np.divmod(np.arange(n), m)
    assert np.array_equal(lo, i + j) and np.array_equal(up, (m - 1 - i) + (m - 1 - j))          # the anti-diagonals of the grid
    assert IM.widths(lo, nlo).max() == 24 and IM.widths(up, nup).max() == 24
    assert IM.widths(lo, nlo).sum() == n


def test_plan():
    level = np.array([0, 0, 0, 1, 2, 2, 2, 3, 4, 4], dtype=np.int32)          # widths 3 1 3 1 2
    assert IM.plan(level, 5, wide=1) == [(l, 1, False) for l in range(5)]
    assert IM.plan(level, 5, wide=1000000) == [(0, 5, True)]
    assert IM.plan(level, 5, wide=3) == [(0, 1, False), (1, 1, True), (2, 1, False), (3, 2, True)]
    assert IM.plan(level, 5, wide=2) == [(0, 1, False), (1, 1, True), (2, 1, False), (3, 1, True), (4, 1, False)]
    assert IM.plan(np.zeros(0, dtype=np.int32), 0) == []


def test_lanes():
    assert IM.default_lanes(1, 1) == 1 and IM.default_lanes(0, 0) == 1
    n, _, rp, _, _ = synth.laplacian_2d(24)
    assert IM.default_lanes(n, int(rp[-1])) == 2
    assert IM.default_lanes(100, 100 + 2 * 100 * 3) == 4 and IM.default_lanes(100, 100 + 2 * 100 * 3 + 1) == 4
    assert IM.default_lanes(100, 100 + 2 * 100 * 4 + 1) == 8
    assert IM.default_lanes(10, 10 + 2 * 10 * 1000) == 64


@pytest.mark.parametrize("G", [1, 2, 4, 16, 64])
def test_butterfly_is_krylov_models_on_padded_lanes(G):
    rng = np.random.default_rng(G)
    s = rng.standard_normal(G)
    padded = np.zeros(KM.LANES)
    padded[:G] = s
    assert np.float64(IM.butterfly(s)).tobytes() == np.float64(KM.butterfly(padded)).tobytes()


@pytest.mark.parametrize("G", [1, 2, 4])
def test_apply_solves_with_the_factors(G):
    """z = U^-1 L^-1 r: L U z = r within the substitution's backward error, n * eps * |L| |U| |z|, for every G"""
    n, _, rp, ci, va = synth.laplacian_2d(7)
    ilu = IM.Ilu.of(rp, ci, va, np.float64, G=G)
    r = KM.inputs(n, np.float64)[0]
    z = ilu.apply(r)
    L, U = IM.dense_lu(n, rp, ci, ilu.f)
    bound = 2 * n * np.finfo(np.float64).eps * (np.abs(L) @ (np.abs(U) @ np.abs(z)))
    assert (np.abs(L @ (U @ z) - r) <= bound + np.finfo(np.float64).tiny).all()
    if G > 1:
        assert np.allclose(z, IM.Ilu.of(rp, ci, va, np.float64, G=1).apply(r), rtol=1e-13, atol=0)
    # the fp64 right-hand side is used as it is
    assert ilu.apply(r, rhs_is_fp64=True).tobytes() == z.tobytes()


def test_zero_pivot_is_named():
    n, _, rp, ci, va = KM.banded("spd", 9, np.float64)
    d = IM.diagonal_positions(rp, ci)
    v = va.copy()
    v[d[4]] = np.nan
    assert IM.factor(rp, ci, v, np.float64)[1] == 4


def test_wide_matrix_and_its_transpose():
    n, _, rp, ci, va = IM.wide_matrix(np.float64)
    assert n == 4097
    lo, up, nlo, nup = IM.levels(rp, ci)
    assert (nlo, nup) == (2, 1) and IM.widths(lo, nlo).tolist() == [2049, 2048]
    _, _, rpt, cit, vat = IM.transpose(n, rp, ci, va)
    lo, up, nlo, nup = IM.levels(rpt, cit)
    assert (nlo, nup) == (1, 2) and IM.widths(up, nup).tolist() == [2048, 2049]          # the later rows first: U runs backwards
    assert np.array_equal(PM.dense_of(n, rpt, cit, vat), PM.dense_of(n, rp, ci, va).T)
    assert IM.plan(lo, nlo) == [(0, 1, False)] and IM.plan(up, nup) == [(0, 1, False), (1, 1, False)]


@pytest.mark.parametrize("m, plain_measured, ilu_measured", [(24, 77, 27), (40, 125, 43)])
def test_model_pcg_halves_the_iterations_of_plain_cg(m, plain_measured, ilu_measured):
    n, _, rp, ci, va = synth.laplacian_2d(m)
    product = PM.host_product(n, rp, ci, va, np.float64)
    b = KM.inputs(n, np.float64)[0]
    plain = KM.cg_model(product, b, None, None, rtol=1e-8, max_iters=400).last
    ilu = IM.IluPcg(product, np.float64, IM.Ilu.of(rp, ci, va, np.float64)).run(b, None, rtol=1e-8, max_iters=400).last
    print(f"laplacian_2d({m}): plain CG {plain.iterations}, ILU(0)-PCG {ilu.iterations} (measured when written: {plain_measured}, {ilu_measured})")
    assert plain.terminal and plain.status == KM.CONVERGED and ilu.terminal and ilu.status == KM.CONVERGED
    assert 2 * ilu.iterations <= plain.iterations
