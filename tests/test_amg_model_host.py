"""CPU: tests/amg_model.py against dense linear algebra -- the model the host set-up and the device cycle are pinned to is a Galerkin hierarchy, its
cycle a symmetric positive definite operator, and conjugate gradients with it need far fewer steps."""
import numpy as np
import pytest

import amg_model as AM
import krylov_model as KM
from cvr_amd import synth

# PCG steps to 1e-8 by the model with the CSR-loop products (plain CG, AMG-PCG): pinned, and written into README.md and DESIGN.md 5.40
PINNED = {24: (77, 27), 40: (125, 32), 100: (307, 54)}
FSAI_RECORD = {24: 44, 40: 72}          # tests/test_fsai_model_host.py


@pytest.mark.parametrize("name", ["laplacian-24", "spd-65", "spd-1025", "singletons", "blocks"])
def test_the_coarse_operator_is_the_galerkin_product(name):
    n, _, rp, ci, va = AM.matrix(name, np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    assert H.bad is None and len(H.levels) >= 2
    for f, c in zip(H.levels, H.levels[1:]):
        A, P = AM.dense(f.n, f.rp, f.ci, f.va), AM.prolongator(f)
        assert (P.sum(axis=1) == 1).all() and (P.sum(axis=0) >= 1).all()          # a partition: every row in one aggregate, none empty
        G, Ac = P.T @ A @ P, AM.dense(c.n, c.rp, c.ci, c.va)
        assert np.abs(G - Ac).max() <= 1e-13 * np.abs(A).sum(axis=1).max() * max(np.bincount(f.agg)) ** 2, name
        assert ((Ac != 0) <= (np.abs(P.T @ np.abs(A) @ P) > 0)).all()
        assert c.n <= 0.8 * f.n
        assert (np.diff(c.ci.astype(np.int64))[np.diff(np.repeat(np.arange(c.n), np.diff(c.rp))) == 0] > 0).all()          # the rows come out sorted


def test_singletons_and_blocks_aggregate_as_the_text_says():
    n, _, rp, ci, va = AM.singletons(np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    size = np.bincount(H.levels[0].agg)
    lonely = np.flatnonzero(np.diff(rp) == 1)
    assert len(lonely) == n // 3 and (size[H.levels[0].agg[lonely]] == 1).all()          # a row without strong neighbours is its own aggregate
    n, _, rp, ci, va = AM.two_blocks(np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    agg = H.levels[0].agg
    assert not set(agg[:81]) & set(agg[81:])          # no aggregate spans the two blocks


@pytest.mark.parametrize("case", [("laplacian-3", {}), ("spd-65", {}), ("singletons", {}), ("laplacian-10", {}), ("laplacian-10", dict(sweeps=2, coarse_scale=1.5)),
                                  ("laplacian-10", dict(max_levels=1)), ("coarse-102", {})], ids=AM.case_id)
def test_the_cycle_is_symmetric_positive_definite(case):
    """M^-1 column by column, n <= 102 (coarse-102: the 24 x 24 Laplacian's first coarse level, taken as a matrix of its own)"""
    name, options = case
    if name == "coarse-102":
        c = AM.setup(*synth.laplacian_2d(24)[2:], np.float64).levels[1]
        n, rp, ci, va = c.n, c.rp, c.ci, c.va
    else:
        n, _, rp, ci, va = AM.matrix(name, np.float64)
    assert n <= 102
    H = AM.setup(rp, ci, va, np.float64, **options)
    pr = AM.cpu_products(H)
    M = np.column_stack([AM.apply(H, pr, e) for e in np.eye(n)])
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max(), case
    assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0, case


def test_the_direct_coarsest_level_is_the_inverse():
    n, _, rp, ci, va = KM.banded("spd", 64, np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    assert len(H.levels) == 1 and H.coarse_direct and np.array_equal(H.winv, H.winv.T)
    A = AM.dense(n, rp, ci, va)
    assert np.abs(H.winv @ A - np.eye(n)).max() <= 1e-12
    r = KM.inputs(n, np.float64)[0]
    assert np.abs(AM.apply(H, AM.cpu_products(H), r) - np.linalg.solve(A, r)).max() <= 1e-12


def test_the_stop_rules():
    n, _, rp, ci, va = AM.diagonal(np.float64)
    H = AM.setup(rp, ci, va, np.float64)
    assert len(H.levels) == 1 and not H.coarse_direct and H.levels[0].agg is None and H.products_per_apply() == 1          # a stall: 300 singletons
    _, _, rp, ci, va = synth.laplacian_2d(24)
    assert [l.n for l in AM.setup(rp, ci, va, np.float64).levels] == [576, 102, 15]
    H = AM.setup(rp, ci, va, np.float64, max_levels=1)
    assert len(H.levels) == 1 and not H.coarse_direct
    H = AM.setup(rp, ci, va, np.float64, max_levels=2)
    assert [l.n for l in H.levels] == [576, 102] and H.coarse_direct and H.products_per_apply() == 2
    H = AM.setup(rp, ci, va, np.float64, coarse_size=1)
    assert H.levels[-1].n == 1 and H.coarse_direct
    assert abs(AM.setup(rp, ci, va, np.float64).operator_complexity() - 1.2475) < 1e-4


@pytest.mark.parametrize("m", sorted(PINNED))
def test_pcg_step_counts(m):
    """the seeded right-hand side and the stop rule of krylov_model: at most half of plain CG's steps on 24 x 24 and 40 x 40 and fewer than FSAI's
    recorded ones, at most a quarter on 100 x 100; the exact counts pinned"""
    n, _, rp, ci, va = synth.laplacian_2d(m)
    H = AM.setup(rp, ci, va, np.float64)
    pr = AM.cpu_products(H)
    b = KM.inputs(n, np.float64)[0]
    plain = KM.CgModel(pr[0], np.float64).run(b, None, None, rtol=1e-8, max_iters=2000).last
    pre = AM.AmgPcg(pr[0], np.float64, H, pr).run(b, None, rtol=1e-8, max_iters=400).last
    print(f"laplacian_2d({m}): AMG-PCG {pre.iterations} steps, CG {plain.iterations}")
    assert plain.terminal and pre.terminal and plain.status == KM.CONVERGED and pre.status == KM.CONVERGED
    if m in FSAI_RECORD:
        assert 2 * pre.iterations <= plain.iterations and pre.iterations < FSAI_RECORD[m]
    else:
        assert 4 * pre.iterations <= plain.iterations
    assert (plain.iterations, pre.iterations) == PINNED[m]


def test_bad_diagonals_and_pivots():
    n, _, rp, ci, va = KM.banded("spd", 100, np.float64)
    d = [int(rp[i] + np.flatnonzero(ci[rp[i]: rp[i + 1]] == i)[0]) for i in range(n)]
    for v, row in ((-1.0, 0), (0.0, 57), (np.nan, 57), (np.inf, 99)):
        broken = va.copy()
        broken[d[row]] = v
        assert AM.setup(rp, ci, broken, np.float64).bad == (0, row, "diagonal"), v
    H = AM.setup(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 2.0, 1.0]), np.float64)          # indefinite: 1 - 2 * 2
    assert H.bad == (0, 1, "pivot")
