"""CPU: tests/mcsgs_model.py against itself -- the colouring by rounds and by the greedy pass, its properties on every case the GPU tests use, a
hand-worked example, the pinned Laplacian table, the dense identity of the apply, and the mutants of the definition that the cases must reject."""
import numpy as np
import pytest

import krylov_model as KM
import mcsgs_model as M


def test_hash_and_key():
    """murmur3's finaliser on known values; the key keeps the index in its low 31 bits and 31 hash bits above them"""
    assert [int(h) for h in M.hash32(np.arange(6))] == [0x0, 0x514E28B7, 0x30F4C306, 0x85F0B427, 0x249CB285, 0xCC0D53CD]
    k = M.key(np.arange(6))
    assert [int(v) & 0x7FFFFFFF for v in k] == list(range(6))
    assert [int(v) >> 31 for v in k] == [0x0, 0x514E28B7 >> 1, 0x30F4C306 >> 1, 0x85F0B427 >> 1, 0x249CB285 >> 1, 0xCC0D53CD >> 1]
    assert int(M.key(np.array([2**31 - 2]))[0]) < 2**62


def test_hand_worked_six_rows():
    """the path 0-1-2-3-4-5 with the chords 1-3 and 3-5.  The keys in descending order: rows 5, 3, 1, 2, 4, 0.
    round 1: only row 5 beats all its uncoloured neighbours (3 and 4)             -> 5 takes 0
    round 2: row 3 (neighbours 1, 2, 4 are smaller, 5 is coloured)                  -> 3 takes 1 (5 holds 0)
    round 3: row 1 (0 and 2 are smaller) and row 4 (3 and 5 are coloured)           -> 1 takes 0 (3 holds 1), 4 takes 2 (3: 1, 5: 0)
    round 4: row 2 (1 and 3 coloured) and row 0 (1 coloured)                        -> 2 takes 2 (1: 0, 3: 1), 0 takes 1 (1: 0)"""
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (1, 3), (3, 5)]
    n, _, rp, ci, va = M._symmetric(6, pairs, np.random.default_rng(6))
    assert np.argsort(-M.key(np.arange(6))).tolist() == [5, 3, 1, 2, 4, 0]
    color, ncolors, rounds, perm, ptr = M.coloring(rp, ci)
    assert color.tolist() == [1, 0, 2, 1, 2, 0] and (ncolors, rounds) == (3, 4)
    assert perm.tolist() == [1, 5, 0, 3, 2, 4] and ptr.tolist() == [0, 2, 4, 6]
    assert color.dtype == np.int32 and perm.dtype == np.int32 and ptr.dtype == np.int32


@pytest.mark.parametrize("name", M.CASES)
def test_properties_of_every_case(name):
    """the rounds and the greedy definition agree (asserted inside M.coloring), the colouring is valid, the colours are contiguous from 0, perm is
    the stable order, every row's colour is at most its degree"""
    n, rp, ci, va, color, ncolors, rounds, perm, ptr = M.case(name)
    assert M.check_pattern(rp, ci) is None
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = rows != ci
    assert (color[rows[off]] != color[ci[off]]).all()
    assert sorted(set(color.tolist())) == list(range(ncolors)) and 1 <= rounds <= n and ncolors <= rounds
    assert (color <= np.diff(rp) - 1).all()
    assert perm.tobytes() == np.array(sorted(range(n), key=lambda i: (color[i], i)), dtype=np.int32).tobytes()
    assert ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) == np.bincount(color, minlength=ncolors)).all()


def test_empty_matrix():
    color, ncolors, rounds, perm, ptr = M.coloring(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    assert (len(color), ncolors, rounds, len(perm), ptr.tolist()) == (0, 0, 0, 0, [0])


def test_the_cases_are_what_their_names_say():
    n, rp, ci, va = M.matrix("irr-sym-3000")
    length = np.diff(rp) - 1
    assert n == 3000 and length.min() == 0 and 40 <= length.max() <= 48 and (length == 0).sum() >= 5 and (va == 0).sum() > 100
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    assert not np.array_equal(dense, dense.T)          # a symmetric pattern (check_pattern) with nonsymmetric values
    assert M.case("clique-70")[5] >= 70 and M.case("clique-70")[0] == 300
    n, rp, ci, va = M.matrix("star-2000")
    assert rp[1] - rp[0] == n and (ci[rp[:-1]] == 0).all()          # row and column 0 full
    assert M.matrix("grid-513")[0] == 513 * 513 > 1024 * 256
    n, rp, ci, va = M.matrix("ties-62291")
    ties = M.tie_pairs(n)
    assert ties and all((M.key(np.array([i]))[0] >> 31) == (M.key(np.array([j]))[0] >> 31) for i, j in ties)
    assert any(j in ci[rp[i]: rp[i + 1]] for i, j in ties)          # at least one such pair is adjacent


def test_pinned_laplacians():
    """colours (rows per colour) and rounds of the 5-point Laplacian, as first prototyped from the definition"""
    want = {"laplacian-24": (4, 10, [211, 215, 109, 41]), "laplacian-40": (5, 10, [594, 591, 309, 103, 3])}
    for name, (nc, rounds, sizes) in want.items():
        c = M.case(name)
        assert (c[5], c[6], np.diff(c[8]).tolist()) == (nc, rounds, sizes), name


def test_the_model_names_the_lowest_offending_row_and_column():
    assert M.check_pattern([0, 2, 5, 7], [0, 2, 0, 1, 2, 1, 2]) == ("symmetric", 0, 2)
    assert M.check_pattern([0, 2, 5, 7], [0, 1, 0, 1, 2, 2, 1]) == ("increasing", 2, 1)
    assert M.check_pattern([0, 2, 4, 7], [0, 1, 0, 2, 0, 1, 2]) == ("diagonal", 1, None)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["nonsym-65", "laplacian-24", "clique-70"])
def test_the_apply_is_the_dense_identity(name, prec):
    """z = (D + U)^-1 D (D + L)^-1 r: to 1e-13 relative in fp64; in fp32 to the rounding of y and z to T"""
    dtype = np.float64 if prec == "fp64" else np.float32
    n, rp, ci, _, color = M.case(name)[:5]
    va = M.values(name, dtype)
    r = KM.inputs(n, dtype)[0]
    want = M.dense_apply(n, rp, ci, va, color, r)
    for G in (1, M.default_lanes(n, int(rp[-1])), 64):
        got = M.apply(rp, ci, va, color, r, G, dtype).astype(np.float64)
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= (1e-13 if prec == "fp64" else 1e-5), (name, prec, G, err)


def test_the_cases_reject_every_mutant():
    """byte comparison of (color, ncolors, rounds); the in-place mutant is a Python loop over the rows and is run on the cases below 5000 rows"""
    caught = {m: [] for m in M.MUTANTS}
    for name in M.CASES:
        n, rp, ci, va, color, ncolors, rounds = M.case(name)[:7]
        for m in M.MUTANTS:
            if m == "in-place" and n > 5000:
                continue
            got = M.color_rounds(rp, ci, m)
            if (got[0].tobytes(), got[1], got[2]) != (color.tobytes(), ncolors, rounds):
                caught[m].append(name)
    for m, names in caught.items():
        print(f"{m}: rejected by {', '.join(names)}")
    assert all(caught.values()), {m: v for m, v in caught.items() if not v}
    assert caught["key-without-index"] == ["ties-62291"] and caught["mask-of-64"] == ["clique-70"]          # the cases built for them


@pytest.mark.parametrize("name", ["laplacian-24", "laplacian-40"])
def test_pcg_steps_of_the_model(name):
    """the model's PCG with a numpy product: fewer steps than plain CG, the prototype's counts within a few steps (another b)"""
    n, rp, ci, va, color = M.case(name)[:5]
    rows = np.repeat(np.arange(n), np.diff(rp))

    def product(p):
        return np.bincount(rows, weights=va * np.asarray(p, dtype=np.float64)[ci], minlength=n)

    b = KM.inputs(n, np.float64)[0]
    pcg = M.McSgsPcg(product, np.float64, M.McSgs(rp, ci, va, np.float64, color=color)).run(b, None, rtol=1e-8, max_iters=300).last
    cg = KM.CgModel(product, np.float64, "tree").run(b, None, None, rtol=1e-8, max_iters=300).last
    print(f"{name}: multicolour SGS PCG {pcg.iterations} steps, CG {cg.iterations}")
    assert pcg.status == cg.status == KM.CONVERGED and pcg.iterations < cg.iterations
    assert abs(pcg.iterations - {"laplacian-24": 42, "laplacian-40": 67}[name]) <= 6
