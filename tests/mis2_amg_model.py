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
    """sa_amg_model.matrix and lopsided, chain, two-blocks (amg_model's `blocks`)"""
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
