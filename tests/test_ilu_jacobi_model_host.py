"""CPU: tests/ilu_jacobi_model.py itself -- the numpy model of cvr_precond_ilu0_jacobi that the GPU tests compare the device with -- against
tests/ilu_model.py, the model of the exact object.

  * once s reaches the level count the swept apply is the exact one bit for bit (8 x 8 Laplacian, 15 levels each way, and irr-spd-700; fp64 and
    fp32, the fp64 right-hand side included); one sweep below the bound max(levels_lower, levels_upper - 1) at least one row differs
  * model PCG in fp64 to 1e-8 on the 24 x 24 and 40 x 40 Laplacians, b = default_rng(1).standard_normal(n): the step counts are non-increasing in s,
    equal the exact model's by s = 8 and are strictly below plain CG's at s = 1 (measured when written: 24 x 24 plain 77, exact 27,
    s = 1 .. 8: 43 33 29 28 28 27 27 27; 40 x 40 plain 124, exact 43, s = 1 .. 8: 70 53 46 44 43 43 43 43)
  * a diagonal matrix gives z = T(r / d) for every s; n = 0 gives nothing"""
import numpy as np
import pytest

import ilu_jacobi_model as JM
import ilu_model as IM
import krylov_model as KM
import precond_model as PM
from cvr_amd import synth


def _case(name, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    if name == "laplacian-8":
        n, _, rp, ci, va = synth.laplacian_2d(8, dtype)
        f, bad = IM.factor(rp, ci, va, dtype)
        assert bad is None
        return (n, rp, ci, f) + IM.levels(rp, ci)[2:] + (dtype,)
    n, rp, ci, _, f, _, _, nlo, nup, _ = IM.irregular_case(name, prec)
    return n, rp, ci, f, nlo, nup, dtype


def test_the_8_by_8_laplacian_has_15_levels_each_way():
    assert _case("laplacian-8", "fp64")[4:6] == (15, 15)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["laplacian-8", "irr-nonsym-2500"])
def test_exact_once_s_reaches_the_level_count(name, prec):
    """s = max(levels) and s = the header's bound max(levels_lower, levels_upper - 1) give ilu_model.apply's bits (irr-nonsym-2500 is the irregular
    case whose 26 and 28 levels fit under CVR_ILU0_MAX_SWEEPS).  The bound is sufficient, not sharp: with r of type T, y(0) = r already holds level
    0's values (y_i = T(r_i - 0) = r_i), so L is exact one sweep earlier, and the sweeps reach the exact bits numerically before they do so
    structurally where the factors' entries are small.  Below the bound, therefore: on the Laplacian s = max(levels) - 2 = 13 differs in at least one
    row (the corner-to-corner paths of 14 steps are missing; measured: s = 14 is exact); on the strictly row-dominant irregular case the bits are the
    exact ones from s = 22 (fp64) and 13 (fp32) on, measured, and what is asserted is that s = 1 .. 4, the sweep counts of use, all differ."""
    n, rp, ci, f, nlo, nup, dtype = _case(name, prec)
    G = IM.default_lanes(n, int(rp[-1]))
    r = KM.inputs(n, dtype)[0]
    want = IM.apply(rp, ci, f, r, G, dtype)
    assert np.isfinite(want).all() and want.any()
    got = JM.IluJacobi(rp, ci, f, G, dtype, max(nlo, nup)).apply(r)
    assert got.dtype == dtype and got.tobytes() == want.tobytes()
    bound = max(nlo, nup - 1)
    assert JM.exact_sweeps(nlo, nup) == bound <= JM.MAX_SWEEPS
    assert JM.IluJacobi(rp, ci, f, G, dtype, bound).apply(r).tobytes() == want.tobytes()
    below = [max(nlo, nup) - 2] if name == "laplacian-8" else [1, 2, 3, 4]
    for s in below:
        differ = np.flatnonzero(JM.IluJacobi(rp, ci, f, G, dtype, s).apply(r) != want)
        print(f"{name} {prec}: levels {nlo}, {nup}; s = {s}: {len(differ)} of {n} rows differ")
        assert len(differ) >= 1, s
    # the fp64 right-hand side (GMRES's u) is used as it is
    u = KM.inputs(n, np.float64, seed=3)[0]
    assert JM.IluJacobi(rp, ci, f, G, dtype, bound).apply(u, rhs_is_fp64=True).tobytes() == IM.apply(rp, ci, f, u, G, dtype, rhs_is_fp64=True).tobytes()


@pytest.mark.parametrize("m, measured", [(24, (77, 27, [43, 33, 29, 28, 28, 27])), (40, (124, 43, [70, 53, 46, 44, 43, 43]))])
def test_model_pcg_step_counts_by_s(m, measured):
    n, _, rp, ci, va = synth.laplacian_2d(m)
    product = PM.host_product(n, rp, ci, va, np.float64)
    b = np.random.default_rng(1).standard_normal(n)
    plain = KM.cg_model(product, b, None, None, rtol=1e-8, max_iters=400).last
    f, bad = IM.factor(rp, ci, va, np.float64)
    assert bad is None
    G = IM.default_lanes(n, int(rp[-1]))
    exact = IM.IluPcg(product, np.float64, IM.Ilu(rp, ci, f, G, np.float64)).run(b, None, rtol=1e-8, max_iters=400).last
    swept = [IM.IluPcg(product, np.float64, JM.IluJacobi(rp, ci, f, G, np.float64, s)).run(b, None, rtol=1e-8, max_iters=400).last for s in range(1, 9)]
    counts = [e.iterations for e in swept]
    print(f"laplacian_2d({m}): plain CG {plain.iterations}, exact ILU(0) {exact.iterations}, s = 1 .. 8: {counts} (the issue's dense numpy check: {measured})")
    assert plain.terminal and plain.status == KM.CONVERGED and exact.terminal and exact.status == KM.CONVERGED
    assert all(e.terminal and e.status == KM.CONVERGED for e in swept)
    assert all(a >= b_ for a, b_ in zip(counts, counts[1:])), counts          # non-increasing in s
    assert counts[7] == exact.iterations
    assert counts[0] < plain.iterations


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_a_diagonal_matrix_and_n_zero(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n = 9
    rp, ci = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)
    d = (1.5 + np.arange(n)).astype(dtype)
    r = KM.inputs(n, dtype)[0]
    want = (r.astype(np.float64) / d.astype(np.float64)).astype(dtype)
    for s in (1, 2, 5):
        assert JM.IluJacobi.of(rp, ci, d, dtype, s).apply(r).tobytes() == want.tobytes()
    empty = JM.IluJacobi(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype), 1, dtype, 3)
    assert len(empty.apply(np.zeros(0, dtype=dtype))) == 0
