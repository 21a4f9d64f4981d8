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
