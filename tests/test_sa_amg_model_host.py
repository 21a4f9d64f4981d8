"""CPU: tests/sa_amg_model.py against dense fp64 algebra -- the yardstick here is numpy's dense arithmetic, not the library -- and the PCG step
counts of the model on the Laplacians, pinned.

The bound of a level.  With u = the type's epsilon (2^-52 or 2^-23), row sums of |.| taken entry-wise on the dense matrices:
  * P.  g_ij is a sum of at most kA terms (kA = the longest row of A_l), each product exact (a * 1.0): |g - g*| <= kA u (|A| T)_ij to first order.
    p_ij = T(t - w g) adds three roundings in fp64 (below u) and one in T.  So |p - p*| <= (kA + 2) u * (T_ij + omega dinv_i (|A| T)_ij) =: E_P.
  * A_next = R (A P): (A P)_ij is a sum of at most kA terms with one rounding per product and per addition, R (A P) of at most kR terms (kR = the
    longest row of R_l): |c - c*| <= (kA + kR + 2) u (|R| |A| |P|)_IJ for exact P, and P's own error enters twice, as E_P^T |A| |P| + |P|^T |A| E_P.
Both are first-order bounds with the constants above and a factor 2 for the second-order terms; nothing is fitted to what the model gives."""
import numpy as np
import pytest

import amg_model as AM
import krylov_model as KM
import sa_amg_model as SA

PLAIN_STEPS = {24: 27, 40: 32, 100: 54}          # tests/test_amg_model_host.py: plain aggregation
SMOOTHED_STEPS = {24: 14, 40: 16, 100: 18}       # this model's own counts


def _dense_csr(c):
    d = np.zeros((c.nrows, c.ncols))
    rows = np.repeat(np.arange(c.nrows), np.diff(c.rp))
    d[rows, c.ci] = c.va.astype(np.float64)
    return d


CASES = [("laplacian-24", {}, 0.0), ("laplacian-23", {}, 0.0), ("singletons", {}, 0.0), ("blocks", {}, 0.0), ("zero-entry", {}, 0.0), ("laplacian-24", {}, 0.9),
         ("laplacian-40", dict(max_levels=2), 0.0), ("spd-1025", {}, 0.0)]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]},{c[1]},omega={c[2]}")
def test_prolongators_and_coarse_operators_against_dense_algebra(case, prec):
    name, options, omega = case
    dtype = np.float64 if prec == "fp64" else np.float32
    u = float(np.finfo(dtype).eps)
    H = SA.cached_setup(name, dtype, omega, **options)
    assert H.bad is None and len(H.P) == len(H.levels) - 1 >= 1
    assert H.omega == (4.0 / 3.0 if omega == 0.0 else omega)
    for l, lv in enumerate(H.levels):
        d = lv.diagonal()
        assert (d > 0).all(), (name, l)          # a positive diagonal in every row ...
        for i in range(lv.n):
            assert (np.diff(lv.ci[lv.rp[i]: lv.rp[i + 1]].astype(np.int64)) > 0).all(), (name, l, i)          # ... and sorted rows
    for l, (P, R) in enumerate(zip(H.P, H.R)):
        lv, nxt = H.levels[l], H.levels[l + 1]
        A = AM.dense(lv.n, lv.rp, lv.ci, lv.va)
        Tm = AM.prolongator(lv)
        dinv = lv.dinv.astype(np.float64)
        kA, kR = int(np.diff(lv.rp).max()), int(np.diff(R.rp).max())
        Pd = _dense_csr(P)
        exact_P = Tm - (H.omega * dinv)[:, None] * (A @ Tm)
        E_P = 2 * (kA + 2) * u * (Tm + (H.omega * dinv)[:, None] * (np.abs(A) @ Tm))
        assert (np.abs(Pd - exact_P) <= E_P).all(), (name, prec, l, float(np.abs(Pd - exact_P).max()), float(E_P.max()))
        assert np.array_equal(_dense_csr(R), Pd.T)
        C = AM.dense(nxt.n, nxt.rp, nxt.ci, nxt.va)
        exact_C = exact_P.T @ A @ exact_P
        aP, aA = np.abs(exact_P), np.abs(A)
        E_C = 2 * ((kA + kR + 2) * u * (aP.T @ aA @ aP) + E_P.T @ aA @ aP + aP.T @ aA @ E_P)
        assert (np.abs(C - exact_C) <= E_C).all(), (name, prec, l, float(np.abs(C - exact_C).max()), float(E_C.max()))
        assert (np.abs(C - C.T) <= 2 * E_C).all()          # symmetric to rounding only


def test_a_stored_zero_keeps_its_entry_and_singleton_rows_hold_one_entry():
    n, _, rp, ci, va = SA.zero_entry(np.float64)
    H = SA.cached_setup("zero-entry", np.float64)
    P = H.P[0]
    lv = H.levels[0]
    # G's pattern is structural: row i holds agg[j] of every stored j, also where a_ij = 0.0
    for i in range(n):
        assert set(P.ci[P.rp[i]: P.rp[i + 1]]) == set(lv.agg[ci[rp[i]: rp[i + 1]]]), i
    zero_only = [(i, j) for i in range(n) for j, v in zip(ci[rp[i]: rp[i + 1]], va[rp[i]: rp[i + 1]])
                 if v == 0.0 and lv.agg[j] not in lv.agg[[c for c, w in zip(ci[rp[i]: rp[i + 1]], va[rp[i]: rp[i + 1]]) if w != 0.0]]]
    assert zero_only, "the case must hold a stored zero that alone reaches its aggregate"
    for i, j in zero_only:
        q = P.rp[i] + int(np.flatnonzero(P.ci[P.rp[i]: P.rp[i + 1]] == lv.agg[j])[0])
        assert P.va[q] == 0.0          # the entry stays, with the value -(w * 0.0)
    # a singleton row (its diagonal alone): one entry 1 - omega * dinv * a_ii, and dinv = 1 / a_ii up to its rounding
    H = SA.cached_setup("singletons", np.float64)
    P, lv = H.P[0], H.levels[0]
    alone = np.flatnonzero(np.diff(lv.rp) == 1)
    assert len(alone) == 30
    for i in alone:
        assert P.rp[i + 1] - P.rp[i] == 1 and P.ci[P.rp[i]] == lv.agg[i]
        assert P.va[P.rp[i]] == 1.0 - (H.omega * float(lv.dinv[i])) * float(lv.va[lv.rp[i]])
    # the diagonal matrix stalls (every row a singleton: 300 aggregates of 300 rows), so it has one level and no prolongator at all
    H = SA.cached_setup("diagonal", np.float64)
    assert (len(H.levels), len(H.P), H.coarse_direct, H.products_per_apply()) == (1, 0, False, 1)


@pytest.mark.parametrize("m", [24, 40, 100])
def test_pcg_steps_on_the_laplacian_are_pinned_and_below_plain_aggregation(m):
    steps, H = SA.pcg_steps(m)
    print(f"laplacian_2d({m}): smoothed {steps} steps, plain aggregation {PLAIN_STEPS[m]}; levels {[l.n for l in H.levels]}, "
          f"operator complexity {H.operator_complexity():.3f}, longest row of A_l / P_l {max(int(np.diff(l.rp).max()) for l in H.levels)} / "
          f"{max(int(np.diff(p.rp).max()) for p in H.P)}")
    assert steps == SMOOTHED_STEPS[m]
    assert steps < PLAIN_STEPS[m]          # the issue's condition: strictly below the plain count on every grid


def test_the_plain_counts_this_file_compares_with_are_the_plain_models():
    """27 and 32 of tests/test_amg_model_host.py, recomputed by amg_model on the two small grids (the third takes the plain model too long here)"""
    for m in (24, 40):
        n, _, rp, ci, va = AM.matrix(f"laplacian-{m}", np.float64)
        H = AM.setup(rp, ci, va, np.float64)
        prods = AM.cpu_products(H)
        last = AM.AmgPcg(prods[0], np.float64, H, prods).run(KM.inputs(n, np.float64)[0], None, rtol=1e-8, max_iters=200).last
        assert last.iterations == PLAIN_STEPS[m]
