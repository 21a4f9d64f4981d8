"""The graph colouring (cvr_color_host, cvr_color_device) and the multicolour symmetric Gauss-Seidel preconditioner (cvr_precond_mcsgs, kind 5) in
numpy, written from the text of include/cvr_amd.h (not from the kernels), beside ilu_model.py, whose lane sums (`butterfly`, `default_lanes`) and
PCG model it uses.

What the header fixes and this file does, in the header's order:
  * the pattern rules (`check_pattern`): the columns of every row strictly increasing, a diagonal entry in every row, and for every stored (i, j),
    j != i, a stored (j, i); stored zeros count; the lowest offending row and its lowest such column are named;
  * the key (`key`): key(i) = (h(i) >> 1) << 31 | i with h murmur3's 32-bit finaliser of uint32(i) -- no seed, no level;
  * a round (`color_rounds`), a pure function of the state before it: every uncoloured row whose key is greater than the key of each uncoloured
    neighbour takes the smallest colour >= 0 that none of its neighbours holds; rounds repeat until no row is uncoloured; `rounds` counts the
    rounds that coloured at least one row.
    The result equals greedy first-fit colouring in descending key order (`color_greedy`): a row is coloured in the round in which the last
    neighbour with a larger key has been coloured before it, so when it chooses, exactly its neighbours with larger keys hold colours -- what
    the serial greedy pass sees when it reaches the row.  `coloring` asserts the equality for every pattern it is given;
  * perm (the rows by (colour, row number)) and color_ptr (`order_of`);
  * M = (D + L) D^-1 (D + U) with L the entries a_ij of color[j] < color[i] and U those of color[j] > color[i]; the apply (`apply`): lane l of a
    row's G lanes adds double(a_ij) * double(v_j) over the entries l, l + G, .. of the row's part in column order from +0, the lanes by the xor
    butterfly; forward over the colours y_i = T((double(r_i) - s) / double(a_ii)), backward z_i = T(double(y_i) - s / double(a_ii));
  * cvr_pcg_device's recurrences with this apply where they have T(minv * r) (`McSgsPcg`).
The arithmetic of the apply is Python's float (IEEE fp64, one rounding per operation, never fused)."""
import functools

import numpy as np

import ilu_model as IM
import krylov_model as KM
from cvr_amd import synth

default_lanes = IM.default_lanes
butterfly = IM.butterfly


def hash32(i):
    """murmur3's 32-bit finaliser of uint32 values (an array)"""
    x = np.asarray(i, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def key(i):
    """key(i) = (h(i) >> 1) << 31 | i as int64 (below 2^62)"""
    i = np.asarray(i, dtype=np.uint64)
    return (((hash32(i) >> np.uint64(1)) << np.uint64(31)) | i).astype(np.int64)


def check_pattern(rp, ci):
    """None, or (what, row, column) of the lowest offending row: "increasing", "diagonal" (column None) or "symmetric" (its lowest column j whose
    row j has no entry in column `row`)"""
    n = len(rp) - 1
    rows = [np.asarray(ci[rp[i]: rp[i + 1]], dtype=np.int64) for i in range(n)]
    for i in range(n):
        if len(rows[i]) > 1 and not (np.diff(rows[i]) > 0).all():
            k = int(np.flatnonzero(np.diff(rows[i]) <= 0)[0]) + 1
            return ("increasing", i, int(rows[i][k]))
        if i not in rows[i]:
            return ("diagonal", i, None)
    for i in range(n):
        for j in rows[i].tolist():
            if j != i and i not in rows[j]:
                return ("symmetric", i, j)
    return None


def _entries(rp, ci):
    """(row, column) of every off-diagonal entry"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rp, dtype=np.int64)))
    cols = np.asarray(ci[rp[0]: rp[-1]], dtype=np.int64)
    off = rows != cols
    return rows[off], cols[off]


MUTANTS = ("key-without-index", "ascending-keys", "largest-plus-one", "mask-of-64", "in-place")


def color_rounds(rp, ci, mutant=None):
    """(color int32[n], ncolors, rounds) by the rounds.  mutant: one of MUTANTS -- a wrong reading of the definition, for the model's own test (a
    mutant that colours nothing in a round stops there and leaves -1)"""
    n = len(rp) - 1
    if mutant == "in-place":
        return _color_rounds_in_place(rp, ci)
    rows, cols = _entries(rp, ci)
    k = key(np.arange(n))
    if mutant == "key-without-index":
        k = (k >> 31) << 31
    if mutant == "ascending-keys":
        k = -k - 1
    color = np.full(n, -1, dtype=np.int64)
    rounds = 0
    while (color < 0).any():
        unc = color < 0
        live = unc[rows] & unc[cols]
        best = np.full(n, np.iinfo(np.int64).min, dtype=np.int64)          # the largest key among the uncoloured neighbours
        np.maximum.at(best, rows[live], k[cols[live]])
        win = unc & (k > best)
        if not win.any():
            break          # (a mutant's deadlock)
        # the winners' neighbours that hold a colour, in the state before the round
        sel = win[rows] & ~unc[cols]
        wr, wc = rows[sel], color[cols[sel]]
        new = np.zeros(n, dtype=np.int64)
        if mutant == "largest-plus-one":
            top = np.full(n, -1, dtype=np.int64)
            np.maximum.at(top, wr, wc)
            new = top + 1
        else:
            limit = 64 if mutant == "mask-of-64" else None
            while True:
                hit = np.zeros(n, dtype=bool)
                hit[wr[wc == new[wr]]] = True
                if limit is not None:
                    hit &= new < limit          # the mask sees colours 0 .. 63 only: past them nothing is taken
                if not hit.any():
                    break
                new[hit] += 1
        color[win] = new[win]
        rounds += 1
    ncolors = int(color.max()) + 1 if n else 0
    return color.astype(np.int32), ncolors, rounds


def _color_rounds_in_place(rp, ci):
    """the mutant whose round reads the state being written: the rows in ascending order, each seeing the colours rows before it took this round"""
    n = len(rp) - 1
    k = key(np.arange(n)).tolist()
    nb = [[int(j) for j in ci[rp[i]: rp[i + 1]] if j != i] for i in range(n)]
    color = [-1] * n
    rounds = 0
    while any(c < 0 for c in color):
        did = False
        for i in range(n):
            if color[i] >= 0 or any(color[j] < 0 and k[j] > k[i] for j in nb[i]):
                continue
            used = {color[j] for j in nb[i]}
            c = 0
            while c in used:
                c += 1
            color[i] = c
            did = True
        rounds += did
    return np.array(color, dtype=np.int32), (max(color) + 1 if n else 0), rounds


def color_greedy(rp, ci):
    """greedy first-fit in descending key order, serial: color int32[n]"""
    n = len(rp) - 1
    rp_, ci_ = [int(v) for v in rp], [int(v) for v in ci[: rp[-1]]] if n else []
    color = [-1] * n
    for i in np.argsort(-key(np.arange(n)), kind="stable").tolist():
        used = {color[j] for j in ci_[rp_[i]: rp_[i + 1]] if j != i}
        c = 0
        while c in used:
            c += 1
        color[i] = c
    return np.array(color, dtype=np.int32)


def order_of(color, ncolors):
    """(perm int32[n]: the rows by (colour, row number); color_ptr int32[ncolors + 1])"""
    color = np.asarray(color, dtype=np.int64)
    perm = np.argsort(color, kind="stable").astype(np.int32)
    ptr = np.zeros(ncolors + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(np.bincount(color, minlength=ncolors)[:ncolors])
    return perm, ptr


def coloring(rp, ci):
    """(color, ncolors, rounds, perm, color_ptr) of a pattern that passes check_pattern; the rounds and the greedy definition are held equal"""
    assert check_pattern(rp, ci) is None, check_pattern(rp, ci)
    color, ncolors, rounds = color_rounds(rp, ci)
    assert color.tobytes() == color_greedy(rp, ci).tobytes(), "the rounds and greedy first-fit in descending key order differ"
    return (color, ncolors, rounds) + order_of(color, ncolors)


def bad_diagonal(rp, ci, va):
    """the lowest row whose diagonal entry is zero or not finite, or None"""
    for i in range(len(rp) - 1):
        for q in range(rp[i], rp[i + 1]):
            if ci[q] == i and not (va[q] != 0 and np.isfinite(va[q])):
                return i
    return None


def apply(rp, ci, va, color, r, G, dtype):
    """z = M^-1 r by the header's arithmetic: va and r values of T"""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    rp_, ci_ = [int(v) for v in rp], [int(v) for v in ci[: rp[-1]]] if n else []
    a = np.asarray(va[: rp[-1]], dtype=T).astype(np.float64).tolist() if n else []
    col = [int(c) for c in color]
    rl = np.asarray(r, dtype=T).astype(np.float64).tolist()
    rows = np.argsort(np.asarray(color, dtype=np.int64), kind="stable").tolist()          # (any order that respects the colours gives the same values)
    d = [0.0] * n
    y, z = [0.0] * n, [0.0] * n

    def part_sum(i, v, lower):
        s, e = [0.0] * G, 0
        for q in range(rp_[i], rp_[i + 1]):
            j = ci_[q]
            if j == i:
                d[i] = a[q]
            elif (col[j] < col[i]) == lower:
                s[e % G] = s[e % G] + a[q] * v[j]
                e += 1
        return butterfly(s)

    with np.errstate(all="ignore"):
        for i in rows:
            s = part_sum(i, y, True)
            y[i] = float(T(np.float64(rl[i] - s) / np.float64(d[i])))
        for i in reversed(rows):
            s = part_sum(i, z, False)
            z[i] = float(T(y[i] - float(np.float64(s) / np.float64(d[i]))))
    return np.array(z, dtype=np.float64).astype(T)


def dense_apply(n, rp, ci, va, color, r):
    """(D + U)^-1 D (D + L)^-1 r with dense fp64 matrices"""
    D, L, U = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            j = int(ci[q])
            (D if j == i else L if color[j] < color[i] else U)[i, j] = np.float64(va[q])
    return np.linalg.solve(D + U, D @ np.linalg.solve(D + L, np.asarray(r, dtype=np.float64)))


class McSgs:
    """an object: the matrix, its colouring, G"""

    def __init__(self, rp, ci, va, dtype, G=None, color=None):
        self.rp, self.ci, self.T = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.dtype(dtype).type
        self.va = np.asarray(va, dtype=dtype)
        n = len(rp) - 1
        self.color = coloring(rp, ci)[0] if color is None else color
        self.G = default_lanes(n, int(rp[-1])) if G is None else int(G)

    def apply(self, r, rhs_is_fp64=False):
        assert not rhs_is_fp64
        return apply(self.rp, self.ci, self.va, self.color, r, self.G, self.T)


class McSgsPcg(IM.IluPcg):
    """cvr_pcg_device with a multicolour SGS object: ilu_model.IluPcg's recurrences with this object's apply"""


# ---- the cases the CPU and the GPU tests share ----
def _csr(n, cols_of, vals_of):
    rp, ci, va = [0], [], []
    for i in range(n):
        c = sorted(set(cols_of[i]) | {i})
        ci += c
        va += [vals_of(i, j) for j in c]
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=np.float64)


def _symmetric(n, pairs, rng, zero_share=0.0):
    """a matrix on the symmetric closure of `pairs` with nonsymmetric values: off-diagonals uniform in (-1, 1) (a share of them stored zeros), the
    diagonal 1 + the row's sum of |off-diagonals| + U(0, 1)"""
    cols = [set() for _ in range(n)]
    for i, j in pairs:
        if i != j:
            cols[i].add(j)
            cols[j].add(i)
    n, _, rp, ci, va = _csr(n, cols, lambda i, j: 0.0)
    off = rng.uniform(-1.0, 1.0, size=len(ci))
    off[rng.random(len(ci)) < zero_share] = 0.0
    rows = np.repeat(np.arange(n), np.diff(rp))
    isd = rows == ci
    off[isd] = 0.0
    rowsum = np.bincount(rows, weights=np.abs(off), minlength=n)
    va = off.copy()
    va[isd] = 1.0 + rowsum + rng.random(n)
    return n, n, rp, ci, va


def _irr_sym_3000():
    """power-law row lengths 0 .. 48, some rows with the diagonal alone, some stored zeros"""
    n, rng = 3000, np.random.default_rng(20261020)
    pairs = []
    for i in range(n):
        if rng.random() < 0.1:
            continue
        k = min(48, int(rng.pareto(1.0)) + 1)          # (each pair lengthens two rows; the closure is capped below)
        pairs += [(i, int(j)) for j in np.where(rng.random(k) < 0.5, (i + 1 + rng.integers(0, 8, size=k)) % n, rng.integers(0, n, size=k))]
    deg = np.zeros(n, dtype=np.int64)
    kept = []
    for i, j in pairs:
        if i != j and deg[i] < 48 and deg[j] < 48 and (i, j) not in kept[-64:] and (j, i) not in kept[-64:]:
            kept.append((i, j))
            deg[i] += 1
            deg[j] += 1
    return _symmetric(n, kept, rng, zero_share=0.05)


def _clique_70():
    """300 rows that hold one dense 70 x 70 block (rows 40, 43, .. of a band): at least 70 colours"""
    n, rng = 300, np.random.default_rng(70)
    block = [40 + 3 * k for k in range(70)]
    pairs = [(i, i + 1) for i in range(n - 1)] + [(a, b) for a in block for b in block if a < b]
    return _symmetric(n, pairs, rng)


def _star_2000():
    """row and column 0 full, the rest a band"""
    n, rng = 2000, np.random.default_rng(2000)
    pairs = [(0, j) for j in range(1, n)] + [(i, i + d) for i in range(1, n) for d in (1, 2) if i + d < n]
    return _symmetric(n, pairs, rng)


def tie_pairs(n):
    """the pairs (i, j), i < j < n, whose keys agree in their 31 hash bits"""
    h = (hash32(np.arange(n)) >> np.uint64(1)).astype(np.int64)
    order = np.argsort(h, kind="stable")
    same = np.flatnonzero(h[order][1:] == h[order][:-1])
    return [(int(min(order[k], order[k + 1])), int(max(order[k], order[k + 1]))) for k in same]


def _ties_62291():
    """a band long enough that rows with equal 31 hash bits exist, each such pair connected: only the index bits of the key decide between them"""
    n, rng = 62291, np.random.default_rng(62291)
    ties = tie_pairs(n)
    assert ties, "no two rows below 62291 share their 31 hash bits"
    return _symmetric(n, [(i, i + 1) for i in range(n - 1)] + ties, rng)


REGULAR = [f"{k}-{n}" for k in ("spd", "nonsym") for n in (1, 2, 63, 64, 65, 1025)] + ["laplacian-3", "laplacian-24", "laplacian-40"]
IRREGULAR = ["irr-sym-3000", "clique-70", "star-2000", "grid-513", "ties-62291"]
CASES = REGULAR + IRREGULAR
LARGE = ("grid-513", "ties-62291")          # the cases the preconditioner's export-and-apply tests leave to the colouring's


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(n, rp, ci, va) of a named case in fp64, read-only and shared"""
    kind, _, size = name.partition("-")
    if kind in ("spd", "nonsym"):
        n, _, rp, ci, va = KM.banded(kind, int(size), np.float64)
    elif kind == "laplacian":
        n, _, rp, ci, va = synth.laplacian_2d(int(size))
    elif kind == "grid":
        n, _, rp, ci, va = synth.laplacian_2d(int(size))          # 513^2 rows: more than one grid of 1024 x 256 threads
    else:
        n, _, rp, ci, va = {"irr-sym-3000": _irr_sym_3000, "clique-70": _clique_70, "star-2000": _star_2000, "ties-62291": _ties_62291}[name]()
    for a in (rp, ci, va):
        a.setflags(write=False)
    return n, rp, ci, va


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, rp, ci, va, color, ncolors, rounds, perm, color_ptr) of a named case: coloured once, nobody writes to the arrays"""
    n, rp, ci, va = matrix(name)
    out = coloring(rp, ci)
    for a in (out[0], out[3], out[4]):
        a.setflags(write=False)
    return (n, rp, ci, va) + out


def values(name, dtype):
    """the case's values in T"""
    return matrix(name)[3].astype(dtype)
