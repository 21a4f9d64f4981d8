"""CPU: tests/mis2_amg_model.py against itself -- the properties of the MIS(2) aggregation, a hand-worked example entry by entry, and the pinned
levels, rounds and PCG step counts on the Laplacians."""
import numpy as np
import pytest

import amg_model as AM
import mis2_amg_model as M

# the serial aggregation's counts (tests/test_sa_amg_model_host.py): 14 / 16 / 18
LEVELS = {24: [576, 85, 13], 40: [1600, 233, 31], 100: [10000, 1425, 159, 22]}
ROUNDS = {24: [8, 5], 40: [10, 6], 100: [8, 8, 5]}
STEPS = {24: 19, 40: 19, 100: 22}


def test_the_hash_is_murmur3s_finaliser():
    # fmix32 of 0, 1, 2 and 0xffffffff, from the reference implementation's constants worked by hand in Python integers
    def fmix(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    got = M.murmur3_fmix32(np.array([0, 1, 2, 12345, 0x7FFFFFFE, 0xFFFFFFFF], dtype=np.uint64))
    assert [int(v) for v in got] == [fmix(v) for v in (0, 1, 2, 12345, 0x7FFFFFFE, 0xFFFFFFFF)]
    assert int(got[0]) == 0 and fmix(1) == 0x514E28B7
    k = M.keys(np.array([1, 2, 0]))
    assert [int(v) >> 62 for v in k] == [1, 2, 0] and [int(v) & 0x7FFFFFFF for v in k] == [0, 1, 2]
    assert [(int(v) >> 31) & 0x7FFFFFFF for v in k] == [fmix(i) >> 1 for i in range(3)]


@pytest.mark.parametrize("name", M.AGGREGATION_CASES)
def test_every_row_is_assigned_and_the_roots_are_numbered_in_ascending_order(name):
    lv = M.level_of(name, np.float64)
    agg, nc, rounds = M.cached_aggregate(name, np.float64)
    rows, cols, _ = M.strong_graph(lv, 0.08)
    assert agg.dtype == np.int32 and len(agg) == lv.n and agg.min() >= 0 and agg.max() == nc - 1 and len(np.unique(agg)) == nc
    # replay the rounds: the roots
    state = np.full(lv.n, M.UNDECIDED, dtype=np.int64)
    for _ in range(rounds):
        assert (state == M.UNDECIDED).any()
        state, _, _ = M.mis2_round(state, rows, cols)
    assert not (state == M.UNDECIDED).any()
    roots = np.flatnonzero(state == M.ROOT)
    assert len(roots) == nc and np.array_equal(agg[roots], np.arange(nc))          # numbered by ascending row
    # every other row is within two directed steps of the root of its aggregate
    nb = [set(cols[rows == i].tolist()) for i in range(lv.n)]
    for i in np.flatnonzero(state != M.ROOT):
        r = int(roots[agg[i]])
        assert r in nb[i] or any(r in nb[j] for j in nb[i]), (name, i, r)
    # a row without strong neighbours is a singleton root
    for i in range(lv.n):
        if not nb[i]:
            assert state[i] == M.ROOT and (agg == agg[i]).sum() == 1 + sum(1 for j in range(lv.n) if j != i and agg[j] == agg[i])
    if name == "chain":
        assert rounds <= 32          # where the serial passes' dependency chain is n / 3 long
    if name == "diagonal":
        assert (nc, rounds) == (lv.n, 1)


@pytest.mark.parametrize("name", ["laplacian-24", "singletons", "two-blocks", "chain", "zero-entry"])
def test_no_two_roots_lie_within_two_steps_on_a_symmetric_graph(name):
    lv = M.level_of(name, np.float64)
    agg, nc, _ = M.cached_aggregate(name, np.float64)
    rows, cols, _ = M.strong_graph(lv, 0.08)
    S = np.zeros((lv.n, lv.n), dtype=bool)
    S[rows, cols] = True
    assert (S == S.T).all(), "the case's strong graph is symmetric"
    two = S | (S.astype(np.int64) @ S.astype(np.int64) > 0)
    roots = np.array([int(np.flatnonzero(agg == a)[0]) for a in range(nc)])          # candidates: the root is some member -- find it by the rounds
    state = np.full(lv.n, M.UNDECIDED, dtype=np.int64)
    while (state == M.UNDECIDED).any():
        state, _, _ = M.mis2_round(state, rows, cols)
    roots = np.flatnonzero(state == M.ROOT)
    sub = two[np.ix_(roots, roots)]
    np.fill_diagonal(sub, False)
    assert not sub.any()
    # ... and maximal: every row has a root within two steps
    assert (two[:, roots].any(axis=1) | (state == M.ROOT)).all()


def test_the_lopsided_case_is_what_its_name_says():
    lv = M.level_of("lopsided", np.float64)
    P = np.zeros((lv.n, lv.n), dtype=bool)
    P[lv.rows(), lv.ci] = True
    assert (P & ~P.T).any()          # some (i, j) without (j, i)
    rows, cols, _ = M.strong_graph(lv, 0.08)
    S = np.zeros((lv.n, lv.n), dtype=bool)
    S[rows, cols] = True
    assert (S & ~S.T & P.T).any()          # a stored pair of which one direction is strong and the other is not
    assert 50 <= lv.n <= 70


def test_a_hand_worked_example_entry_by_entry():
    """Six rows, the path 0 - 1 - 2 - 3 - 4 - 5 with the diagonal 2 and -1 beside it, except a_23 = a_32 = -0.1, which is weak at strength 0.08
    (0.01 < 0.0064 * 4 = 0.0256), and a_45 = a_54 = -1.5: N = {0: 1, 1: 0 2, 2: 1, 3: 4, 4: 3 5, 5: 4}.
    The hashes h(i) >> 1 of 0 .. 5: 0x00000000, 0x28a7145b, 0x187a6183, 0x42f85a13, 0x124e5942, 0x6606a9e6 -- so by key 5 > 3 > 1 > 2 > 4 > 0.
    Round 1: m1 = key of (1, 1, 1, 3, 5, 5), m2 = key of (1, 1, 1, 5, 5, 5): rows 1 and 5 see themselves and become roots, nobody goes out (no
    state 2 was visible at the start).  Round 2: m1 of rows 0, 1, 2 carries the root 1, of rows 4, 5 the root 5, of row 3 (whose only neighbour 4 is
    undecided) its own key; m2 of row 3 sees m1(4) = the root 5: rows 0, 2, 3, 4 go out.  Two rounds.  Roots 1 and 5 are aggregates 0 and 1.
    Pass 1: 0 -> 0 (root 1), 2 -> 0 (root 1; 3 is not strong), 4 -> 1 (root 5), 3 has no root beside it.  Pass 2: 3 -> agg of 4 = 1."""
    n = 6
    A = np.zeros((n, n))
    for i in range(n):
        A[i, i] = 2.0
    for i, v in ((0, -1.0), (1, -1.0), (2, -0.1), (3, -1.0), (4, -1.5)):
        A[i, i + 1] = A[i + 1, i] = v
    _, _, rp, ci, va = AM._csr_of_dense(A, np.float64)
    lv = AM.Level(n, rp, ci, va)
    rows, cols, mag = M.strong_graph(lv, 0.08)
    assert list(zip(rows.tolist(), cols.tolist())) == [(0, 1), (1, 0), (1, 2), (2, 1), (3, 4), (4, 3), (4, 5), (5, 4)]
    assert mag.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.5, 1.5]
    h = [int(v) >> 1 for v in M.murmur3_fmix32(np.arange(n))]
    assert h == [0x00000000, 0x28A7145B, 0x187A6183, 0x42F85A13, 0x124E5942, 0x6606A9E6]
    key = lambda s, i: (s << 62) | (h[i] << 31) | i          # noqa: E731
    state = np.full(n, M.UNDECIDED, dtype=np.int64)
    assert [int(k) for k in M.keys(state)] == [key(1, i) for i in range(n)]
    state, m1, m2 = M.mis2_round(state, rows, cols)
    assert [int(v) for v in m1] == [key(1, i) for i in (1, 1, 1, 3, 5, 5)]
    assert [int(v) for v in m2] == [key(1, i) for i in (1, 1, 1, 5, 5, 5)]
    assert state.tolist() == [1, 2, 1, 1, 1, 2]
    state, m1, m2 = M.mis2_round(state, rows, cols)
    assert [int(v) for v in m1] == [key(2, 1), key(2, 1), key(2, 1), key(1, 3), key(2, 5), key(2, 5)]
    assert [int(v) for v in m2] == [key(2, 1), key(2, 1), key(2, 1), key(2, 5), key(2, 5), key(2, 5)]
    assert state.tolist() == [0, 2, 0, 0, 0, 2]
    agg, nc, rounds = M.aggregate(lv, 0.08)
    assert (agg.tolist(), nc, rounds) == ([0, 0, 0, 1, 1, 1], 2, 2)
    # a tie in |a_ij| goes to the lowest j: with a_23 = a_32 = -1 the only root of round 1 is 5; 3 and 4 go out in round 2, 1 becomes a root in
    # round 3 and 0 and 2 go out in round 4.  Pass 1 leaves row 3 free (neither 2 nor 4 is a root); pass 2 finds 2 (aggregate 0) and 4 (aggregate 1)
    # equally strong and takes the lower one
    A[2, 3] = A[3, 2] = -1.0
    _, _, rp, ci, va = AM._csr_of_dense(A, np.float64)
    agg, nc, rounds = M.aggregate(AM.Level(n, rp, ci, va), 0.08)
    assert (agg.tolist(), nc, rounds) == ([0, 0, 0, 0, 1, 1], 2, 4)


def test_n_zero_and_one():
    lv = AM.Level(0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    agg, nc, rounds = M.aggregate(lv, 0.08)
    assert (len(agg), nc, rounds) == (0, 0, 0)
    lv = AM.Level(1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([3.0]))
    agg, nc, rounds = M.aggregate(lv, 0.08)
    assert (agg.tolist(), nc, rounds) == ([0], 1, 1)


@pytest.mark.parametrize("m", [24, 40, 100])
def test_levels_rounds_and_pcg_steps_on_the_laplacian_are_pinned(m):
    steps, H = M.pcg_steps(m)
    print(f"laplacian_2d({m}): MIS(2) {steps} steps; levels {[l.n for l in H.levels]}, rounds {H.rounds}, operator complexity {H.operator_complexity():.3f}")
    assert [l.n for l in H.levels] == LEVELS[m] and H.rounds == ROUNDS[m] and H.coarse_direct
    assert steps == STEPS[m]
    assert 1.3 < H.operator_complexity() < 1.4


# ---- the irregular and the large cases (M.IRREGULAR): the conditions tests/test_gpu_mis2_amg_irregular.py relies on, and the mutants they tell apart ----
NEW = M.IRREGULAR_CASES
SMALL_NEW = ["irr-spd-3000", "irr-directed-3000", "star-2000"]
MUTANT_CASES = SMALL_NEW + M.TIES_CASES          # (the three edge cases are ties-62290's band without the pairs: nothing it does not show)
SYMMETRIC = [name for name in NEW if name != "irr-directed-3000"]


def _pattern_code(n, rp, ci):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + ci


@pytest.mark.parametrize("name", NEW)
def test_the_generators_keep_their_rules(name):
    n, ncols, rp, ci, va = M.matrix(name, np.float64)
    assert n == ncols == len(rp) - 1 and rp[0] == 0 and rp[-1] == len(ci) == len(va) and ci.dtype == np.int32 and rp.dtype == np.int64
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    inner = rows[1:] == rows[:-1]
    assert (np.diff(ci.astype(np.int64))[inner] > 0).all(), "strictly increasing columns"
    assert np.array_equal(np.flatnonzero(ci == rows) >= 0, np.ones(n, dtype=bool)) and (ci == rows).sum() == n, "a diagonal entry in every row"
    again = M.IRREGULAR[name][0](np.float64)          # the seed: made twice, the same bytes; fp32 is the rounded fp64
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[2:], (rp, ci, va)))
    assert M.matrix(name, np.float32)[4].tobytes() == va.astype(np.float32).tobytes()
    code = _pattern_code(n, rp, ci)
    back = ci.astype(np.int64) * n + rows
    order = np.argsort(back, kind="stable")
    if name in SYMMETRIC:
        assert np.array_equal(back[order], code) and np.array_equal(va[order], va), "symmetric"
        off = ci != rows
        d = va[~off]
        assert (va[off] <= 0).all() and (d > np.bincount(rows[off], weights=-va[off], minlength=n)).all(), "an M-matrix, strictly dominant"
        assert np.array_equal(va.astype(np.float32).astype(np.float64)[off], va[off]) or name == "irr-spd-3000"          # the distinct weights are fp32 numbers
    else:
        assert not np.isin(code, back).all(), "some (i, j) without (j, i)"


def test_the_irregular_matrices_are_what_the_issue_asks_for():
    n, _, rp, ci, va = M.matrix("irr-spd-3000", np.float64)
    lv = AM.Level(n, rp, ci, va)
    length = np.diff(rp) - 1
    hist = np.bincount(length)
    print(f"irr-spd-3000: off-diagonal row lengths 0 .. {length.max()}, {hist[:8].tolist()} rows of 0 .. 7, {(length > 20).sum()} of more than 20")
    assert n == 3000 and 40 <= length.max() <= 70 and (length == 0).mean() >= 0.05
    assert np.median(length) <= 4 and (length > 20).sum() >= 30          # a power law: most rows short, a tail of long ones
    off = ci != lv.rows()
    weak = 1.0 - AM.strong_entries(lv, 0.08).sum() / off.sum()
    print(f"irr-spd-3000: {100 * weak:.1f} % of the off-diagonal entries fail the strength test at 0.08")
    assert 0.05 <= weak <= 0.25
    mag = np.abs(va[off])
    assert (mag == 0).sum() == 24 and 0.05 <= mag[mag > 0].min() and mag.max() <= 1.0          # 12 edges stored as explicit zeros
    grid = (mag * 8 == np.round(mag * 8)) & (mag > 0)
    assert 0.15 <= grid.mean() <= 0.25
    # equal magnitudes inside a row beside distinct ones
    r = lv.rows()[off]
    order = np.lexsort((mag, r))
    same = (r[order][1:] == r[order][:-1]) & (mag[order][1:] == mag[order][:-1]) & (mag[order][1:] > 0)
    assert same.sum() >= 100 and len(np.unique(mag)) > 1000
    # the directed case: irr-spd's pattern less one direction of about 30 % of the edges, a third of the survivors weak
    m, _, rp2, ci2, va2 = M.matrix("irr-directed-3000", np.float64)
    code, code2 = _pattern_code(n, rp, ci), _pattern_code(m, rp2, ci2)
    assert m == n and np.isin(code2, code).all()
    gone = (len(code) - len(code2)) / (off.sum() / 2)
    lv2 = AM.Level(m, rp2, ci2, va2)
    rows2, cols2, _ = M.strong_graph(lv2, 0.08)
    one_way = ~np.isin(cols2 * n + rows2, rows2 * n + cols2)
    scaled = (np.abs(va2) < 0.02) & (va2 != 0) & (ci2 != lv2.rows())          # (w * 2^-7 <= 2^-7, and no unscaled weight is below 0.05)
    print(f"irr-directed-3000: {100 * gone:.1f} % of the edges lost a direction, {scaled.sum()} survivors scaled, {one_way.sum()} strong entries without a strong reverse")
    assert 0.25 <= gone <= 0.35 and 0.08 <= scaled.sum() / (off.sum() / 2) <= 0.12 and one_way.sum() >= 500
    assert not AM.strong_entries(lv2, 0.08)[scaled].any()
    # the star
    n, _, rp, ci, va = M.matrix("star-2000", np.float64)
    assert n == 2000 and rp[1] == 2000 and len(np.unique(va[1: rp[1]])) == 1999          # row 0: every other row, pairwise distinct weights
    lv = AM.Level(n, rp, ci, va)
    rows, cols, _ = M.strong_graph(lv, 0.08)
    assert 0 < (rows == 0).sum() < 100          # a few spokes are strong


@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES)
def test_the_models_setup_of_the_irregular_cases(name):
    for dtype in (np.float64, np.float32):
        H = M.cached_setup(name, dtype)
        print(f"{name} {np.dtype(dtype).name}: levels {[l.n for l in H.levels]}, nnz {[l.nnz for l in H.levels]}, rounds {H.rounds}, coarse_direct {H.coarse_direct}")
        assert H.bad is None and len(H.levels) >= (3 if name == "irr-spd-3000" else 2)
        assert all((lv.diagonal() > 0).all() for lv in H.levels)


def test_the_stars_products_reach_the_block_and_the_spill_class():
    """level 0's coarsening of star-2000 under the default limits (32 and 4096): what the device SpGEMM meets inside the set-up without a debug knob"""
    import spgemm_model as SM
    H = M.cached_setup("star-2000", np.float64)
    lv = H.levels[0]
    A = SM.Csr(lv.n, lv.n, lv.rp, lv.ci, lv.va)
    AP = SM.spgemm(A, H.P[0])
    first, second = SM.products(A, H.P[0]), SM.products(H.R[0], AP)
    c1, c2 = SM.row_classes(first), SM.row_classes(second)
    print(f"star-2000: (empty, group, block, spill) of A P {c1}, of R (A P) {c2}; row 0 of A P has {first[0]} products and {AP.rp[1]} entries, the longest row of R (A P) {second.max()} products")
    assert c1[2] >= 1 and c2[2] >= 1 and c1[3] + c2[3] >= 1
    assert lv.rp[1] - lv.rp[0] >= 1999 and first[0] >= SM.BLOCK_LIMIT
    assert (SM.GROUP_LIMIT, SM.BLOCK_LIMIT) == (32, 4096)


def test_the_equal_hash_pairs_and_their_isolation():
    pairs = M.equal_hash_pairs(513 * 513)
    print(f"rows below 513^2 whose 31 hash bits agree: {pairs}")
    assert len(pairs) == 12 and pairs[0] == (52799, 62289) and M.equal_hash_pairs(62289) == [] and M.equal_hash_pairs(62290) == [(52799, 62289)]
    assert {(70665, 76500), (64972, 102456), (80037, 117520)} <= set(pairs)
    h = M.murmur3_fmix32(np.arange(513 * 513)) >> np.uint64(1)
    assert len(np.unique(h)) == 513 * 513 - 12 and all(h[i] == h[j] for i, j in pairs)
    for name in M.TIES_CASES:
        lv = M.level_of(name, np.float64)
        rows, cols, _ = M.strong_graph(lv, 0.08)
        mine = M.equal_hash_pairs(lv.n)
        assert len(mine) == (12 if name == "ties-grid-513" else 1)
        for i, j in mine:
            assert cols[rows == i].tolist() == [j] and cols[rows == j].tolist() == [i], (name, i, j)
            assert not np.isin(cols[(rows != i) & (rows != j)], [i, j]).any()
        # round 1 decides the pair by the index bits alone: the higher row becomes the root
        state, m1, m2 = M.mis2_round(np.full(lv.n, M.UNDECIDED, dtype=np.int64), rows, cols)
        assert all(state[j] == M.ROOT and state[i] == M.UNDECIDED for i, j in mine)
    assert 513 * 513 - M.GRID_THREADS == 1025 and 512 * 512 == M.GRID_THREADS


def test_rounds_of_the_new_cases_cross_the_read_back_interval():
    rounds = {name: M.cached_aggregate(name, np.float64)[2] for name in NEW}
    print(f"rounds of the new cases: {rounds}")
    assert max(rounds.values()) > 4
    # the three sizes around one grid are one band: the same aggregates up to the last rows
    a, b = M.cached_aggregate("edge-262143", np.float64)[0], M.cached_aggregate("edge-262145", np.float64)[0]
    assert np.array_equal(a[:262000], b[:262000])


# The mutants: `_variant` is M.aggregate with one rule changed; "none" is the model itself.
MUTANTS = ["the join ignores magnitudes", "join ties go to the highest j", "pass 2 reads its own output", "pass 2 accepts roots only", "the key has no index bits",
           "key ties go to the lower row", "m2 is taken from the keys", "the strong graph is symmetrised", "the strength test in T", "an inclusive scan numbers the roots"]
# what has to catch what, by construction of the cases
MUST = {"the join ignores magnitudes": SMALL_NEW, "join ties go to the highest j": SMALL_NEW, "pass 2 reads its own output": SMALL_NEW, "pass 2 accepts roots only": SMALL_NEW,
        "the key has no index bits": M.TIES_CASES, "key ties go to the lower row": M.TIES_CASES, "m2 is taken from the keys": MUTANT_CASES,
        "the strong graph is symmetrised": ["irr-directed-3000"], "an inclusive scan numbers the roots": MUTANT_CASES}


def _variant_keys(state, kind):
    i = np.arange(len(state), dtype=np.uint64)
    low = np.zeros_like(i) if kind == "the key has no index bits" else np.uint64(0x7FFFFFFF) - i if kind == "key ties go to the lower row" else i
    return (state.astype(np.uint64) << np.uint64(62)) | ((M.murmur3_fmix32(i) >> np.uint64(1)) << np.uint64(31)) | low


def _variant_join(free, ok, agg, rows, cols, mag, n, kind):
    on = free[rows] & ok[cols]
    r, c, m = rows[on], cols[on], mag[on]
    if kind == "the join ignores magnitudes":
        m = np.ones(len(m))
    best = np.full(n, -1.0)
    np.maximum.at(best, r, m)
    at = np.flatnonzero(m == best[r])
    out = np.full(n, -1, dtype=np.int64)
    if kind == "join ties go to the highest j":
        pick = np.full(n, -1, dtype=np.int64)
        np.maximum.at(pick, r[at], at)
        have = pick >= 0
    else:
        pick = np.full(n, len(r), dtype=np.int64)
        np.minimum.at(pick, r[at], at)
        have = pick < len(r)
    out[have] = agg[c[pick[have]]]
    return out


def _variant(lv, strength, kind, T=np.float64):
    n = lv.n
    if kind == "the strength test in T":
        r_, c_, a, d = lv.rows(), lv.ci.astype(np.int64), np.asarray(lv.va, dtype=T), lv.diagonal().astype(T)
        on = (c_ != r_) & (a != 0) & (a * a >= ((T(strength) * T(strength)) * d[r_]) * d[c_])
        assert (a * a).dtype == np.dtype(T)
        rows, cols, mag = r_[on], c_[on], np.abs(M._f64(lv.va))[on]
    else:
        rows, cols, mag = M.strong_graph(lv, strength)
    if kind == "the strong graph is symmetrised":
        code = np.r_[rows * n + cols, cols * n + rows]
        _, first = np.unique(code, return_index=True)          # (sorted by row, then column; of an entry present both ways the row's own magnitude)
        rows, cols, mag = np.r_[rows, cols][first], np.r_[cols, rows][first], np.r_[mag, mag][first]
    state = np.full(n, M.UNDECIDED, dtype=np.int64)
    rounds = 0
    while (state == M.UNDECIDED).any() and rounds < 200:
        key = _variant_keys(state, kind)
        m1 = M._spread_max(key, rows, cols)
        m2 = M._spread_max(key if kind == "m2 is taken from the keys" else m1, rows, cols)
        und = state == M.UNDECIDED
        new = state.copy()
        new[und & (m2 == key)] = M.ROOT
        new[und & ((m2 >> np.uint64(62)) == np.uint64(M.ROOT))] = M.OUT
        state = new
        rounds += 1
    root = state == M.ROOT
    number = np.cumsum(root) - (0 if kind == "an inclusive scan numbers the roots" else root)
    nc = int(root.sum())
    agg = np.where(root, number, -1).astype(np.int64)
    one = _variant_join(~root, root, agg, rows, cols, mag, n, kind)
    agg1 = np.where(root, agg, one)
    if kind == "pass 2 reads its own output":          # in place, row by row
        agg2 = agg1.copy()
        start = np.searchsorted(rows, np.arange(n + 1))
        for i in np.flatnonzero(agg1 < 0):
            c, m = cols[start[i]: start[i + 1]], mag[start[i]: start[i + 1]]
            ok = agg2[c] >= 0
            if ok.any():
                agg2[i] = agg2[c[ok][int(np.argmax(m[ok]))]]
    else:
        two = _variant_join(agg1 < 0, root if kind == "pass 2 accepts roots only" else agg1 >= 0, agg1, rows, cols, mag, n, kind)
        agg2 = np.where(agg1 >= 0, agg1, two)
    return agg2.astype(np.int32), nc, rounds, int((agg1 < 0).sum())


def _caught(name, kind, dtype):
    want = M.cached_aggregate(name, dtype)
    got = _variant(M.level_of(name, dtype), 0.08, kind, np.dtype(dtype).type)
    return not (got[0].tobytes() == want[0].tobytes() and got[1:3] == want[1:])


@pytest.mark.parametrize("name", MUTANT_CASES + M.AGGREGATION_CASES)
def test_the_scaffold_of_the_mutants_is_the_model(name):
    for dtype in (np.float64, np.float32):
        assert not _caught(name, "none", dtype)


def test_the_new_cases_tell_the_mutants_apart():
    """Byte comparison of (agg, nc, rounds) in fp64.  Every mutant but the strength test in T (fp32 only, below) is caught by the new cases named in
    MUST; the printed lines say which of the old cases catch it -- before the new cases a mutant with an empty list there passed the whole suite."""
    for kind in MUTANTS:
        if kind == "the strength test in T":
            continue
        new = [name for name in MUTANT_CASES if _caught(name, kind, np.float64)]
        old = [name for name in M.AGGREGATION_CASES if _caught(name, kind, np.float64)]
        print(f"fp64 {kind}: caught by {new}; of the old cases by {old}, not by {[c for c in M.AGGREGATION_CASES if c not in old]}")
        assert set(MUST[kind]) <= set(new), (kind, new)
    # ... and the conditions behind them, row by row, on the three small cases
    for name in SMALL_NEW:
        lv = M.level_of(name, np.float64)
        want = M.cached_aggregate(name, np.float64)[0]
        free_after_pass_1 = _variant(lv, 0.08, "none")[3]
        lowest = _variant(lv, 0.08, "the join ignores magnitudes")[0]
        highest = _variant(lv, 0.08, "join ties go to the highest j")[0]
        print(f"{name}: pass 2 assigns {free_after_pass_1} rows; {(lowest != want).sum()} rows do not follow their lowest eligible neighbour, {(highest != want).sum()} are decided by the tie rule")
        assert free_after_pass_1 >= 1 and (lowest != want).sum() >= 1 and (highest != want).sum() >= 1


def test_the_strength_test_in_fp32_is_printed():
    """fp32 only: a_ij^2 >= ((s s) a_ii) a_jj evaluated in float instead of double moves an entry across the threshold only when the two sides agree
    to 2^-24; where no case holds such an entry the mutant cannot show, and the line says so (nothing is asserted of it, as in the ILU file)"""
    new = [name for name in MUTANT_CASES if _caught(name, "the strength test in T", np.float32)]
    old = [name for name in M.AGGREGATION_CASES if _caught(name, "the strength test in T", np.float32)]
    print(f"fp32 the strength test in T: caught by {new}; of the old cases by {old}")


def test_the_directed_case_has_a_one_way_entry_that_matters():
    """some i with j in N(i) and i not in N(j) influences the result: with the strong graph symmetrised the bytes change"""
    assert _caught("irr-directed-3000", "the strong graph is symmetrised", np.float64) and _caught("irr-directed-3000", "the strong graph is symmetrised", np.float32)
    for name in ("irr-spd-3000", "star-2000", "ties-62290"):          # ... and on a symmetric strong graph it is the identity
        assert not _caught(name, "the strong graph is symmetrised", np.float64)


IRREGULAR_STEPS = {"irr-spd-3000": 21, "star-2000": 17}          # tests/test_gpu_mis2_amg_irregular.py pins the same counts


@pytest.mark.parametrize("name", M.IRREGULAR_SETUP_CASES)
def test_pcg_steps_on_the_irregular_cases_are_pinned(name):
    import krylov_model as KM
    import sa_amg_model as SA
    H = M.cached_setup(name, np.float64)
    A, P, R = SA.cpu_products(H)
    b = KM.inputs(H.levels[0].n, np.float64)[0]
    last = SA.SaAmgPcg(A[0], np.float64, H, A, P, R).run(b, None, rtol=1e-8, max_iters=200).last
    print(f"{name}: MIS(2) smoothed AMG-PCG {last.iterations} steps to 1e-8, operator complexity {H.operator_complexity():.3f}")
    assert last.terminal and last.status == KM.CONVERGED and last.iterations == IRREGULAR_STEPS[name]
