"""Smoothed-aggregation AMG with the MIS(2) aggregation (cvr_precond_amg_mis2, cvr_amg_mis2_setup_host, cvr_amg_mis2_aggregate_host / _device) in
numpy, written from the text of include/cvr_amd.h (not from the library's code), on top of sa_amg_model.py -- whose set-up it repeats with
`aggregate` below in place of amg_model.aggregate -- and of amg_model.py's strength test.

The aggregation, a pure function of the level's CSR and `strength`, in parallel rounds:
  * N(i): the columns j != i of row i that pass the strength test, row by row, never symmetrised (`strong_graph`);
  * key(i) = state_i << 62 | (h(i) >> 1) << 31 | i with h = murmur3's 32-bit finaliser of the row index and the states 1 undecided, 2 root, 0 out;
  * a round: m1 = max of key over {i} + N(i), m2 = max of m1 over {i} + N(i); an undecided i with m2 == key(i) becomes a root, an undecided i
    whose m2 carries state 2 goes out; rounds repeat until nothing is undecided (`rounds`: those that began with an undecided row);
  * the aggregates are numbered by their roots in ascending row order;
  * join pass 1: a non-root with a root in N(i) takes the aggregate of the root with the largest |a_ij| (ties: the lowest j); pass 2: a still-free
    i takes that of the j in N(i) that is a root or was assigned by pass 1, by the same rule.  Nothing is left free."""
import numpy as np

import amg_model as AM
import krylov_model as KM
import sa_amg_model as SA
from cvr_amd import synth

UNDECIDED, ROOT, OUT = 1, 2, 0
_f64 = AM._f64


def murmur3_fmix32(i):
    """murmur3's 32-bit finaliser on uint32 values, modulo 2^32"""
    x = np.asarray(i).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def keys(state, n=None):
    """key(i) of every row as uint64"""
    n = len(state) if n is None else n
    i = np.arange(n, dtype=np.uint64)
    return (np.asarray(state).astype(np.uint64) << np.uint64(62)) | ((murmur3_fmix32(i) >> np.uint64(1)) << np.uint64(31)) | i


def strong_graph(lv, strength):
    """(rows, cols, |a|) of the strong entries, in CSR order"""
    on = AM.strong_entries(lv, strength)
    return lv.rows()[on], lv.ci[: lv.nnz].astype(np.int64)[on], np.abs(_f64(lv.va[: lv.nnz]))[on]


def _spread_max(v, rows, cols):
    """max of v over {i} + N(i) for every i"""
    m = v.copy()
    np.maximum.at(m, rows, v[cols])
    return m


def mis2_round(state, rows, cols):
    """(the states after one round, m1, m2)"""
    key = keys(state)
    m1 = _spread_max(key, rows, cols)
    m2 = _spread_max(m1, rows, cols)
    und = state == UNDECIDED
    new = state.copy()
    new[und & (m2 == key)] = ROOT
    new[und & ((m2 >> np.uint64(62)) == np.uint64(ROOT))] = OUT
    return new, m1, m2


def _join(free, ok, agg, rows, cols, mag, n):
    """for every free row with a strong neighbour j that has ok[j]: agg of the j with the largest |a_ij|, the lowest j among equal ones; else -1"""
    out = np.full(n, -1, dtype=np.int64)
    on = free[rows] & ok[cols]
    r, c, m = rows[on], cols[on], mag[on]
    best = np.full(n, -1.0)
    np.maximum.at(best, r, m)
    at = np.flatnonzero(m == best[r])          # (the entries are in column order within a row: the first of them is the lowest j)
    first = np.full(n, len(r), dtype=np.int64)
    np.minimum.at(first, r[at], at)
    have = first < len(r)
    out[have] = agg[c[first[have]]]
    return out


def aggregate(lv, strength):
    """(agg[n] as int32, the number of aggregates, rounds)"""
    n = lv.n
    rows, cols, mag = strong_graph(lv, strength)
    state = np.full(n, UNDECIDED, dtype=np.int64)
    rounds = 0
    while (state == UNDECIDED).any():
        before = int((state == UNDECIDED).sum())
        state, _, _ = mis2_round(state, rows, cols)
        rounds += 1
        assert int((state == UNDECIDED).sum()) < before, "a round decides at least one row"
    root = state == ROOT
    number = np.cumsum(root) - root          # the exclusive scan of the root flags
    nc = int(root.sum())
    agg = np.where(root, number, -1).astype(np.int64)
    one = _join(~root, root, agg, rows, cols, mag, n)
    agg1 = np.where(root, agg, one)
    two = _join(agg1 < 0, agg1 >= 0, agg1, rows, cols, mag, n)
    agg2 = np.where(agg1 >= 0, agg1, two)
    assert (agg2 >= 0).all(), "every out row has a root within two directed steps"
    return agg2.astype(np.int32), nc, rounds


class Hierarchy(SA.Hierarchy):
    def __init__(self, opts, dtype, omega):
        super().__init__(opts, dtype, omega)
        self.rounds = []          # of every level that was coarsened


def setup(rp, ci, va, dtype, omega=0.0, **kw):
    """sa_amg_model.setup with `aggregate` in place of amg_model.aggregate"""
    opts = dict(AM.DEFAULTS, **kw)
    T = np.dtype(dtype).type
    H = Hierarchy(opts, T, SA.used_omega(omega))
    n = len(rp) - 1
    AM.check_structure(rp, ci)
    nnz = int(rp[n])
    lv = AM.Level(n, np.asarray(rp, dtype=np.int64).copy(), np.asarray(ci[:nnz], dtype=np.int32).copy(), np.asarray(va[:nnz], dtype=T).copy())
    with np.errstate(all="ignore"):
        while True:
            lv.dinv, bad = AM.smoother_diagonal(lv, T)
            if bad is not None:
                H.bad = (len(H.levels), bad, "diagonal")
                return H
            H.levels.append(lv)
            if lv.n <= opts["coarse_size"] or len(H.levels) == opts["max_levels"]:
                break
            agg, nc, rounds = aggregate(lv, opts["strength"])
            if nc > 0.8 * lv.n:
                break
            lv.agg, lv.nc = agg, nc
            H.rounds.append(rounds)
            P, R, lv = SA.coarsen(lv, H.omega, T)
            H.P.append(P)
            H.R.append(R)
        last = H.levels[-1]
        if last.n <= AM.MAX_COARSE:
            H.winv, bad = AM.dense_inverse(last, T)
            if bad is not None:
                H.bad = (len(H.levels) - 1, bad, "pivot")
    return H


def same_rounds(H, minfo):
    """"" when a cvr_amg_mis2_info (capi.AmgMis2Info) fits the model's Hierarchy, else what differs"""
    want = H.rounds + [0] * (AM.MAX_LEVELS - len(H.rounds))
    if minfo.mis2 != 1 or minfo.reserved0 != 0 or list(minfo.rounds) != want or any(minfo.reserved):
        return f"mis2 / rounds = {(minfo.mis2, list(minfo.rounds))}, model {(1, want)}"
    return ""


# ---- the cases ----
def lopsided(dtype, n=60):
    """~60 rows for the aggregation alone: a structurally unsymmetric pattern (some (i, j) without (j, i)) and pairs with a_ij != a_ji of which one
    direction is strong and the other is not; the diagonal is 4, so that with strength 0.08 an entry is strong from |a| >= 0.32"""
    A = np.zeros((n, n))
    for i in range(n):
        A[i, i] = 4.0
        if i + 1 < n:          # a chain whose two directions differ: forward strong, backward weak on every third link
            A[i, i + 1] = -1.0 - 0.125 * (i % 4)
            A[i + 1, i] = -0.25 if i % 3 == 0 else -1.0 - 0.125 * (i % 4)
        if i + 7 < n and i % 2 == 0:          # one-way entries: (i, i + 7) without (i + 7, i)
            A[i, i + 7] = -0.5 - 0.0625 * (i % 5)
        if i >= 11 and i % 5 == 1:          # ... and backwards, some of them weak
            A[i, i - 11] = -0.125 if i % 2 else -0.75
    return AM._csr_of_dense(A, dtype)


def chain(dtype, n=200):
    """synth.banded_sym(n, half_band=1) made SPD, a tridiagonal matrix: the serial aggregation's dependency chain is n / 3 long, the rounds stay few"""
    n, _, rp, ci, _ = synth.banded_sym(n, half_band=1)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


def matrix(name, dtype):
    """sa_amg_model.matrix and lopsided, chain, two-blocks (amg_model's `blocks`), and the irregular cases"""
    if name in IRREGULAR:
        return irregular_matrix(name, dtype)
    if name == "lopsided":
        return lopsided(dtype)
    if name == "chain":
        return chain(dtype)
    return SA.matrix("blocks" if name == "two-blocks" else name, dtype)


def level_of(name, dtype):
    n, _, rp, ci, va = matrix(name, dtype)
    return AM.Level(n, rp, ci, va)


AGGREGATION_CASES = ["laplacian-24", "laplacian-40", "singletons", "two-blocks", "diagonal", "zero-entry", "lopsided", "chain"]
SETUP_CASES = [("laplacian-24", {}), ("laplacian-40", {}), ("singletons", {}), ("two-blocks", {}), ("diagonal", {}), ("zero-entry", {}), ("laplacian-40", dict(max_levels=2))]


# ---- the irregular and the large cases ----
# What the Laplacians and the hand-made matrices above leave unrun: magnitudes that differ inside a row (the join's "strongest" is more than its
# "first"), a strong graph that is not symmetric at 3000 rows, rows of thousands of entries and of thousands of products, rows whose 31 hash bits
# agree (the key's index bits decide), and levels of more rows than one grid of 1024 x 256 threads holds.  Everything is seeded: a case is a pure
# function of its name and dtype.  The values are drawn in fp64 and rounded to the dtype; the weights that have to be pairwise distinct are
# multiples of 2^-21 below 1, which fp32 holds exactly.
GRID_THREADS = 1024 * 256          # one trip of the row kernels (cvr_amg_mis2.hip: launch_rows)
SEED = 20261020
SHIFT = 0.5                        # the diagonal's excess over the row's off-diagonal sum
IRR_SHIFT = 2.0 ** -6                # ... of the irregular cases: a larger one grows with the aggregates and leaves level 1 without strong entries
PAIR_WEIGHT = 1.0                  # the edge i - j of an isolated pair: with the diagonals 1 + shift it is strong whatever the shift below 11


def _csr_of_coo(n, r, c, v, dtype):
    """rows ascending in column; (r, c) pairs are unique"""
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    assert not ((r[1:] == r[:-1]) & (c[1:] == c[:-1])).any()
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return n, n, rp, c.astype(np.int32), v.astype(dtype)


def _laplacian_of_edges(n, i, j, w, dtype, shift=SHIFT):
    """the symmetric matrix with -w on (i, j) and (j, i) and the diagonal sum of w + shift: a weighted graph Laplacian plus a positive shift"""
    d = np.bincount(i, weights=w, minlength=n) + np.bincount(j, weights=w, minlength=n) + shift
    k = np.arange(n, dtype=np.int64)
    return _csr_of_coo(n, np.r_[i, j, k], np.r_[j, i, k], np.r_[-w, -w, d], dtype)


def _distinct_weights(count, seed):
    """`count` pairwise distinct weights in [0.5, 1), multiples of 2^-21"""
    assert count <= 1 << 20
    return 0.5 + np.random.default_rng(seed).permutation(1 << 20)[:count] * 2.0 ** -21


def equal_hash_pairs(n):
    """the pairs i < j < n whose 31 hash bits h >> 1 agree, in ascending j: computed, never listed"""
    h = murmur3_fmix32(np.arange(n, dtype=np.uint64)) >> np.uint64(1)
    order = np.argsort(h, kind="stable")
    at = np.flatnonzero(h[order][1:] == h[order][:-1])
    pairs = sorted(((int(order[k]), int(order[k + 1])) for k in at), key=lambda p: p[1])
    assert len({r for p in pairs for r in p}) == 2 * len(pairs), "no row lies in two pairs"
    return pairs


def _isolate_pairs(n, i, j, w):
    """every edge at a row of an equal-hash pair removed, the edge between the two added: N(i) = {j}, N(j) = {i}"""
    pairs = equal_hash_pairs(n)
    rows = np.array([r for p in pairs for r in p], dtype=np.int64)
    keep = ~(np.isin(i, rows) | np.isin(j, rows))
    pi, pj = np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)
    return np.r_[i[keep], pi], np.r_[j[keep], pj], np.r_[w[keep], np.full(len(pairs), PAIR_WEIGHT)]


def _band_edges(n, half=2, seed=SEED + 1):
    """edges (i, i + d), d = 1 .. half, of the first n rows of one endless band: the weight of an edge does not depend on n"""
    big = GRID_THREADS + 1
    assert n <= big
    w = _distinct_weights(big * half, seed).reshape(big, half)
    i = np.repeat(np.arange(n, dtype=np.int64), half)
    j = i + np.tile(np.arange(1, half + 1, dtype=np.int64), n)
    on = j < n
    return i[on], j[on], w[:n].ravel()[on]


def band(n, dtype, ties=False):
    """the first n rows and columns of a weighted band of half-width 2 with pairwise distinct weights, made dominant"""
    i, j, w = _band_edges(n)
    if ties:
        i, j, w = _isolate_pairs(n, i, j, w)
    return _laplacian_of_edges(n, i, j, w, dtype)


def ties_grid(m, dtype):
    """the m x m 5-point grid with pairwise distinct edge weights and a diagonal shift, the rows of every equal-hash pair tied to each other alone"""
    n = m * m
    k = np.arange(n, dtype=np.int64)
    right, down = k[k % m != m - 1], k[k < n - m]
    i, j = np.r_[right, down], np.r_[right + 1, down + m]
    return _laplacian_of_edges(n, *_isolate_pairs(n, i, j, _distinct_weights(len(i), SEED + 2)), dtype, shift=IRR_SHIFT)


def _irregular_edges(n=3000, seed=SEED + 3):
    """(i, j, w, zero) with i < j: row lengths by a power law (1 + 59 * u^30 draws a row, a draw landing within max(6, draws) rows, one in 32
    anywhere; the longest row has 48 entries), 6 % of the rows kept out of every edge, weights 1 - 0.95 * u^6 in [0.05, 1], a fifth of them rounded
    up to the grid k / 8, and `zero` marks 12 edges stored as 0.0.  The long rows' diagonals are large, so nearly all their entries are weak: 19 %
    of the off-diagonal entries fail the strength test at 0.08 (a smaller share needs fewer long rows)"""
    r = np.random.default_rng(seed)
    alone = np.zeros(n, dtype=bool)
    alone[r.choice(n, size=n * 6 // 100, replace=False)] = True
    draws = np.where(alone, 0, 1 + (59 * r.random(n) ** 30).astype(np.int64))
    src = np.repeat(np.arange(n, dtype=np.int64), draws)
    near = src + (1 + (r.random(len(src)) * np.maximum(6, draws[src])).astype(np.int64)) * r.choice([-1, 1], len(src))
    dst = np.where(r.random(len(src)) < 1 / 32, r.integers(0, n, len(src)), near)
    on = (dst >= 0) & (dst < n) & (dst != src)
    on[on] = ~alone[dst[on]]
    lo, hi = np.minimum(src[on], dst[on]), np.maximum(src[on], dst[on])
    code = np.unique(lo * n + hi)
    lo, hi = code // n, code % n
    w = 1.0 - 0.95 * r.random(len(lo)) ** 6
    grid = r.random(len(lo)) < 0.2
    w[grid] = np.ceil(w[grid] * 8) / 8
    zero = np.zeros(len(lo), dtype=bool)
    zero[r.choice(len(lo), size=12, replace=False)] = True
    return lo, hi, np.where(zero, 0.0, w), zero


def irr_spd(dtype, n=3000):
    return _laplacian_of_edges(n, *_irregular_edges(n)[:3], dtype, shift=IRR_SHIFT)


def irr_directed(dtype, n=3000, seed=SEED + 4):
    """irr_spd with one direction removed from 30 % of its edges; of a third of those the surviving direction is scaled by 2^-7, which is below the
    strength test whatever the shift is (a_ii and a_jj are at least the unscaled |a_ij|, and 2^-14 < 0.0064).  The diagonal is irr_spd's"""
    lo, hi, w, _ = _irregular_edges(n)
    r = np.random.default_rng(seed)
    u, up = r.random(len(lo)), r.random(len(lo)) < 0.5          # up: the direction (lo, hi) is the one that goes
    one_way, weak = u < 0.3, u < 0.1
    d = np.bincount(lo, weights=w, minlength=n) + np.bincount(hi, weights=w, minlength=n) + IRR_SHIFT
    a, b = ~(one_way & up), ~(one_way & ~up)          # (lo, hi) stays, (hi, lo) stays
    ws = np.where(weak, w * 2.0 ** -7, w)
    k = np.arange(n, dtype=np.int64)
    return _csr_of_coo(n, np.r_[lo[a], hi[b], k], np.r_[hi[a], lo[b], k], np.r_[-ws[a], -ws[b], d], dtype)


STAR_HALF_BAND = 3


def star(dtype, n=2000, seed=SEED + 5):
    """row 0 joined to every other row with pairwise distinct weights -- 16 spokes of 3 and more, which are strong, the others below 2^-5, which
    are not --, the other rows a band of half-width STAR_HALF_BAND (not a chain: level 1 is dense through row 0, and with 226 rows the Python SpGEMM stays quick) whose weights are distinct
    but for every fifth, rounded up to the grid k / 8; symmetric and dominant by SHIFT"""
    i, j, w = _band_edges(n - 1, half=STAR_HALF_BAND, seed=seed)
    k = np.arange(1, n, dtype=np.int64)
    spoke = np.where(k % 125 == 7, 3.0 + k / 2048.0, 2.0 ** -6 + k * 2.0 ** -17)
    w = np.where(np.arange(len(w)) % 5 == 0, np.ceil(w * 8) / 8, w)          # equal magnitudes inside a row beside distinct ones
    return _laplacian_of_edges(n, np.r_[np.zeros(n - 1, dtype=np.int64), i + 1], np.r_[k, j + 1], np.r_[spoke, w], dtype)


IRREGULAR = {          # name -> (the generator, whether a set-up is run on it)
    "irr-spd-3000": (irr_spd, True),
    "irr-directed-3000": (irr_directed, False),
    "star-2000": (star, True),
    "ties-grid-513": (lambda dtype: ties_grid(513, dtype), True),
    "edge-262143": (lambda dtype: band(GRID_THREADS - 1, dtype), False),
    "edge-262144": (lambda dtype: band(GRID_THREADS, dtype), False),
    "edge-262145": (lambda dtype: band(GRID_THREADS + 1, dtype), False),
    "ties-62290": (lambda dtype: band(62290, dtype, ties=True), False),
}
IRREGULAR_CASES = list(IRREGULAR)
IRREGULAR_SETUP_CASES = ["irr-spd-3000", "star-2000"]          # those whose whole hierarchy the Python model computes
TIES_CASES = ["ties-grid-513", "ties-62290"]
_MATRICES = {}


def irregular_matrix(name, dtype):
    """(n, n, row_ptr, col_idx, vals) of an irregular case, made once per process; nobody writes into it"""
    key = (name, np.dtype(dtype).name)
    if key not in _MATRICES:
        _MATRICES[key] = IRREGULAR[name][0](dtype)
    return _MATRICES[key]


_CACHE = {}


def cached_setup(name, dtype, omega=0.0, **options):
    """the model's hierarchy of a named case, computed once per process (the Python SpGEMM is slow); nobody writes into it"""
    key = (name, np.dtype(dtype).name, omega, tuple(sorted(options.items())))
    if key not in _CACHE:
        n, _, rp, ci, va = matrix(name, dtype)
        _CACHE[key] = setup(rp, ci, va, dtype, omega, **options)
    return _CACHE[key]


def cached_aggregate(name, dtype, strength=AM.DEFAULTS["strength"]):
    key = ("agg", name, np.dtype(dtype).name, strength)
    if key not in _CACHE:
        _CACHE[key] = aggregate(level_of(name, dtype), strength)
    return _CACHE[key]


def pcg_steps(m, rtol=1e-8, max_iters=400):
    """steps of the model's PCG on the m x m Laplacian in fp64 with krylov_model's right-hand side and stop rule: (steps, the Hierarchy)"""
    n = m * m
    H = cached_setup(f"laplacian-{m}", np.float64)
    A, P, R = SA.cpu_products(H)
    b = KM.inputs(n, np.float64)[0]
    last = SA.SaAmgPcg(A[0], np.float64, H, A, P, R).run(b, None, rtol=rtol, max_iters=max_iters).last
    assert last.terminal and last.status == KM.CONVERGED
    return last.iterations, H
