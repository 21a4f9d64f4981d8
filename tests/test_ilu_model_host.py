"""CPU: tests/ilu_model.py itself -- the numpy model of cvr_precond_ilu0 that the GPU tests compare the device with.

  * banded "spd" and "nonsym" have no fill, so ILU(0) is LU: ||L U - A||_max <= 4 eps ||A||_max
  * the 24 x 24 Laplacian has 47 levels each way and its widest level has 24 rows
  * model PCG in fp64 on the 24 x 24 and 40 x 40 Laplacians needs at most half of plain CG's iterations
  * the pieces: the butterfly is krylov_model's on zero-padded lanes, the plan, G, the transposed pattern
  * the irregular cases (ilu_model.IRREGULAR, from ilu_model.irregular) held to what the GPU tests need of them, so that an edit of the generator
    cannot hollow those out: the generator's rules; every pivot and a finite apply in fp64 and fp32; irr-spd-700 and irr-nonsym-700 with G = 4,
    irr-dense-spd-320 with G = 64 and irr-dense-nonsym-320 with G = 32, both with rows of more than 64 entries in each triangle; irr-nonsym-2500
    plans merged, wide, merged in both sweeps under the default threshold; max(2, median level width) gives at least 3 merged and 3 wide launches
    a sweep on the other four; seven lane counts, seven fp64 results on the dense cases; rows with more and with fewer entries than G in one level;
    a merged level of more than 1024 / G rows
  * the mutants those cases tell apart, as variants of _sweep and factor in this file: lanes take contiguous pieces, the butterfly 1 .. G/2, the lanes
    summed in order, the last entry dropped, one entry read beyond the row, the k of an update descending, a fused update (Python before 3.13 has no
    math.fma: it is emulated exactly in rational arithmetic).  fp64: each is caught by the 700-row and the dense cases, the three lane-schedule ones by
    none of the banded or Laplacian cases.  fp32: only the two off-by-one mutants change bytes (see the tests' docstrings); the tables are printed"""
import math
from fractions import Fraction

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


# ---- the irregular cases (IM.IRREGULAR): the conditions tests/test_gpu_ilu0_irregular.py relies on, and the mutants they tell apart ----
IRR = list(IM.IRREGULAR)
DENSE = ["irr-dense-spd-320", "irr-dense-nonsym-320"]
LANES = [1, 2, 4, 8, 16, 32, 64]


def _counts(rp, ci):
    d = IM.diagonal_positions(rp, ci)
    return d - rp[:-1], rp[1:] - d - 1


def _kinds(plan):
    return sum(1 for p in plan if p[2]), sum(1 for p in plan if not p[2])


@pytest.mark.parametrize("name", IRR)
def test_irregular_follows_its_rules(name):
    n, seed, sym, kmax, near, shallow = IM.IRREGULAR[name]
    _, _, rp, ci, va = IM.irregular(n, seed, sym, kmax, np.float64, near, shallow)
    again = IM.irregular(n, seed, sym, kmax, np.float64, near, shallow)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rp, ci, va), again[2:]))          # everything comes from the seed
    d = IM.diagonal_positions(rp, ci)          # (asserts: columns strictly increasing, a diagonal in every row)
    cl, cu = _counts(rp, ci)
    assert cl.max() <= kmax and (sym or cu.max() <= kmax)
    none = np.count_nonzero(cl == 0) / n
    assert 1 / 9 < none < 2 / 9, none          # about one row in six
    assert np.flatnonzero(cl == 0).max() > n * 3 // 4 and np.count_nonzero(cl[: n // 4] == 0) > 0          # ... scattered
    A = PM.dense_of(n, rp, ci, va)
    off = A - np.diag(np.diag(A))
    assert (np.abs(off) < 1).all() and (np.diag(A) > 1 + np.abs(off).sum(axis=1)).all()          # strictly row dominant
    assert np.array_equal(A, A.T) == sym
    f32 = IM.irregular(n, seed, sym, kmax, np.float32, near, shallow)
    assert f32[4].dtype == np.float32 and np.array_equal(f32[3], ci)
    assert d[0] == 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", IRR)
def test_irregular_cases_have_every_pivot_and_a_finite_apply(name, prec):
    n, rp, ci, va, f = IM.irregular_case(name, prec)[:5]          # (asserts that factor reports no bad pivot)
    dtype = f.dtype.type
    assert np.isfinite(f).all() and (f[IM.diagonal_positions(rp, ci)] != 0).all()
    z = IM.apply(rp, ci, f, KM.inputs(n, dtype)[0], IM.default_lanes(n, int(rp[-1])), dtype)
    assert np.isfinite(z).all() and z.any()


def test_default_lanes_of_the_irregular_cases():
    G = {name: IM.default_lanes(IM.IRREGULAR[name][0], int(IM.irregular_case(name, "fp64")[1][-1])) for name in IRR}
    print(G)
    assert G["irr-spd-700"] == 4 and G["irr-nonsym-700"] == 4
    assert sorted(G[name] for name in DENSE)[1] == 64 and sorted(G[name] for name in DENSE)[0] in (16, 32)
    for name in DENSE:          # the strided loop takes a second pass even at G = 64, in each triangle
        cl, cu = _counts(*IM.irregular_case(name, "fp64")[1:3])
        assert cl.max() > 64 and cu.max() > 64, (name, cl.max(), cu.max())


def test_the_2500_case_mixes_launches_under_the_default_threshold():
    n, rp, ci, va, f, lo, up, nlo, nup, _ = IM.irregular_case("irr-nonsym-2500", "fp64")
    for level, nl in ((lo, nlo), (up, nup)):
        plan = IM.plan(level, nl)          # DEFAULT_WIDE
        merged, wide = _kinds(plan)
        print(plan, IM.widths(level, nl)[:4])
        assert wide >= 1 and merged >= 2, plan
        kinds = [p[2] for p in plan]
        assert any(kinds[i: i + 3] == [True, False, True] for i in range(len(kinds)))          # a wide launch between two merged ones


@pytest.mark.parametrize("name", IRR[:4])
def test_the_width_threshold_mixes_launches(name):
    n, rp, ci, va, f, lo, up, nlo, nup, w = IM.irregular_case(name, "fp64")
    assert w == max(2, int(np.median(np.concatenate([IM.widths(lo, nlo), IM.widths(up, nup)]))))
    for level, nl in ((lo, nlo), (up, nup)):
        merged, wide = _kinds(IM.plan(level, nl, w))
        print(name, "threshold", w, "merged", merged, "wide", wide, "of", nl, "levels")
        assert merged >= 3 and wide >= 3


@pytest.mark.parametrize("name", DENSE)
def test_every_lane_count_has_bytes_of_its_own_on_the_dense_cases(name):
    n, rp, ci, va, f = IM.irregular_case(name, "fp64")[:5]
    r = KM.inputs(n, np.float64)[0]
    z = [IM.apply(rp, ci, f, r, g, np.float64).tobytes() for g in LANES]
    assert len(set(z)) == len(LANES)


@pytest.mark.parametrize("name", IRR)
def test_rows_of_unrelated_lengths_share_a_level(name):
    """for the default G, in each sweep: one level holds a row with cnt > G and a row with 0 < cnt < G (a group that loops beside a group with idle
    lanes).  A row with cnt = 0 is a row of level 0 and every row of level 0 has cnt = 0, so no level holds it beside the others: level 0 is asserted
    to have more than one row, which a wavefront of G >= 2 shares."""
    n, rp, ci, va, f, lo, up, nlo, nup, _ = IM.irregular_case(name, "fp64")
    G = IM.default_lanes(n, int(rp[-1]))
    for cnt, level, nl in zip(_counts(rp, ci), (lo, up), (nlo, nup)):
        both = [l for l in range(1, nl) if (cnt[level == l] > G).any() and ((cnt[level == l] > 0) & (cnt[level == l] < G)).any()]
        assert both, (name, G)
        assert np.count_nonzero(cnt == 0) > 1 and (level[cnt == 0] == 0).all()


def test_a_merged_level_needs_several_rounds_of_the_workgroup():
    """some level under a merged launch is wider than 1024 / G, so the loop on `base` goes round again: the dense cases with their own G and the default
    threshold (one merged launch), irr-spd-700 from G = 16 on (test_every_lane_count builds it so).  With G = 2 (irr-nonsym-2500) a round is 512 rows,
    the default threshold: no merged level can be wider"""
    for name, lanes in [(d, None) for d in DENSE] + [("irr-spd-700", 16)]:
        n, rp, ci, va, f, lo, up, nlo, nup, _ = IM.irregular_case(name, "fp64")
        G = IM.default_lanes(n, int(rp[-1])) if lanes is None else lanes
        assert max(IM.widths(lo, nlo).max(), IM.widths(up, nup).max()) < IM.DEFAULT_WIDE          # everything merged
        assert IM.widths(lo, nlo).max() > 1024 // G, (name, G, IM.widths(lo, nlo).max())
        if name != "irr-dense-spd-320":          # (its U has levels of at most 4 rows: the mirrored pattern is a chain)
            assert IM.widths(up, nup).max() > 1024 // G, (name, G)


# the mutants: each a small variant of IM._sweep or IM.factor.  A sweep mutant returns z, a factor mutant the factors.
def _fma(a, b, c):
    """a * b + c rounded once"""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))          # exact, then one rounding to nearest even


def _mutant_sweep(kind, rp, ci, d, f, rhs, G, T, upper):
    n = len(rp) - 1
    v = [0.0] * n
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        beg, end = (d[i] + 1, rp[i + 1]) if upper else (rp[i], d[i])
        cnt = end - beg
        if kind == "drop the last entry":
            end -= 1 if cnt else 0
        if kind == "one entry beyond":          # L: the row's diagonal (v_i still 0 here), U: the next row's first entry
            end = min(end + 1, rp[n])
        s = [0.0] * G
        piece = -(-cnt // G)
        for e, q in enumerate(range(beg, end)):
            l = e // piece if kind == "contiguous pieces" else e % G
            s[l] = s[l] + f[q] * v[ci[q]]
        if kind == "butterfly 1 .. G/2":
            o = 1
            while o < G:
                s = [s[l] + s[l ^ o] for l in range(G)]
                o <<= 1
            acc = s[0]
        elif kind == "lanes in order":
            acc = 0.0
            for x in s:
                acc = acc + x
        else:
            acc = IM.butterfly(s)
        t = rhs[i] - acc
        if upper:
            t = t / f[d[i]]
        v[i] = float(T(t))
    return v


def _mutant_apply(kind, rp, ci, f, r, G, dtype):
    T = np.dtype(dtype).type
    rp_, ci_ = [int(v) for v in rp], [int(v) for v in ci[: rp[-1]]]
    d = [int(v) for v in IM.diagonal_positions(rp, ci)]
    fl = np.asarray(f, dtype=T).astype(np.float64).tolist()
    y = _mutant_sweep(kind, rp_, ci_, d, fl, np.asarray(r, dtype=T).astype(np.float64).tolist(), G, T, False)
    return np.array(_mutant_sweep(kind, rp_, ci_, d, fl, y, G, T, True)).astype(T)


def _mutant_factor(kind, rp, ci, va, dtype):
    """IM.factor entry by entry (row i, columns ascending: a_ij less its a_ik a_kj over the k < min(i, j) of row i whose row has j, then the division
    below the diagonal) -- with the k ascending and two roundings it is IM.factor bit for bit, which the test asserts"""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    d = IM.diagonal_positions(rp, ci)
    a = np.asarray(va[: rp[-1]], dtype=T).astype(np.float64).tolist()
    where = [{int(ci[q]): q for q in range(rp[i], rp[i + 1])} for i in range(n)]
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            j = int(ci[q])
            ks = [(p, where[int(ci[p])].get(j)) for p in range(rp[i], min(q, d[i])) if int(ci[p]) < j]
            ks = [(p, pk) for p, pk in ks if pk is not None]
            for p, pk in (reversed(ks) if kind == "k descending" else ks):
                a[q] = _fma(-a[p], a[pk], a[q]) if kind == "fused update" else a[q] - a[p] * a[pk]
            if j < i:
                a[q] = a[q] / a[d[j]]
    return np.array(a).astype(T)


SWEEP_MUTANTS = ["contiguous pieces", "butterfly 1 .. G/2", "lanes in order", "drop the last entry", "one entry beyond"]
FACTOR_MUTANTS = ["k descending", "fused update"]
OLD = ["spd-65", "nonsym-65", "laplacian-24"]


def _old_case(name, dtype):
    kind, _, size = name.partition("-")
    n, _, rp, ci, va = synth.laplacian_2d(int(size), dtype) if kind == "laplacian" else KM.banded(kind, int(size), dtype)
    return n, rp, ci, va, IM.factor(rp, ci, va, dtype)[0]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_irregular_cases_tell_the_sweep_mutants_apart(prec):
    """fp64: every mutant of the apply differs in bytes from the model on a new case, with the case's default G; on the old banded and Laplacian cases
    (G = 2, at most 2 entries a row) only the off-by-one mutants can show, and the table says which do.  fp32: the sums are fp64 and every y_i, z_i is
    rounded to fp32, so another order of the same terms moves a result about once in 2^29 rows: the two off-by-one mutants are asserted, the three
    orders are printed (fp64 is where the GPU tests tell the lane schedules apart)"""
    dtype = np.float64 if prec == "fp64" else np.float32
    caught = {m: [] for m in SWEEP_MUTANTS}
    for name in IRR[:4] + OLD:          # (irr-nonsym-2500 has G = 2 and at most 3 entries a row: nothing the 700 cases do not show)
        n, rp, ci, va, f = IM.irregular_case(name, prec)[:5] if name in IRR else _old_case(name, dtype)
        G = IM.default_lanes(n, int(rp[-1]))
        r = KM.inputs(n, dtype)[0]
        want = IM.apply(rp, ci, f, r, G, dtype).tobytes()
        assert _mutant_apply("none", rp, ci, f, r, G, dtype).tobytes() == want          # the scaffold itself is the model
        for m in SWEEP_MUTANTS:
            if _mutant_apply(m, rp, ci, f, r, G, dtype).tobytes() != want:
                caught[m].append(name)
    for m in SWEEP_MUTANTS:
        print(f"{prec} {m}: caught by {caught[m]}")
        if prec == "fp64" or m in SWEEP_MUTANTS[3:]:
            assert set(caught[m]) & set(IRR), m
    for m in SWEEP_MUTANTS[:3]:          # a lane schedule cannot show where every row has at most G entries
        assert not set(caught[m]) & set(OLD), (m, caught[m])


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_irregular_cases_tell_the_factor_mutants_apart(prec):
    """fp64: both mutants of the factorisation change exported bytes on the new cases (the fused one is emulated exactly: math.fma where Python has
    it, else rational arithmetic rounded once; it runs on the 700-row cases only, for time).  fp32: the factors are rounded to fp32 once at the end, a
    last-bit difference in fp64 survives that rounding about once in 2^29 entries: the table is printed and nothing is asserted of it."""
    dtype = np.float64 if prec == "fp64" else np.float32
    caught = {m: [] for m in FACTOR_MUTANTS}
    for name in IRR[:4] + OLD:
        n, rp, ci, va, f = IM.irregular_case(name, prec)[:5] if name in IRR else _old_case(name, dtype)
        assert _mutant_factor("none", rp, ci, va, dtype).tobytes() == f.tobytes()
        for m in FACTOR_MUTANTS:
            if m == "fused update" and name in DENSE:
                continue
            if _mutant_factor(m, rp, ci, va, dtype).tobytes() != f.tobytes():
                caught[m].append(name)
    for m in FACTOR_MUTANTS:
        print(f"{prec} {m}: caught by {caught[m]}")
        if prec == "fp64":
            assert set(caught[m]) & set(IRR), m
