"""The contract of the sparse matrix-matrix product C = A B (include/cvr_amd.h: cvr_spgemm_*) in plain numpy and Python: the only definition of
the bits, and the seeded case generators its tests share.

C(i, j) exists iff some position p of A's row i and some position q of B's row col_A[p] have col_B[q] = j.  Its value is acc = +0;
acc = T(acc + T(a[p] * b[q])) over those (p, q) in ascending p (B's rows hold no duplicates, so q is unique for each p).  Rows ascending in column."""
import numpy as np

from cvr_amd import synth

GROUP_LIMIT, BLOCK_LIMIT, LANES = 32, 4096, 8          # cvr_spgemm.h


class Csr:
    def __init__(self, nrows, ncols, rp, ci, va):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.rp = np.ascontiguousarray(rp, dtype=np.int64)
        self.ci = np.ascontiguousarray(ci, dtype=np.int32)
        self.va = np.ascontiguousarray(va)

    def astype(self, dtype):
        return Csr(self.nrows, self.ncols, self.rp, self.ci, self.va.astype(dtype))

    def dense(self):
        """fp64, duplicates summed"""
        d = np.zeros((self.nrows, self.ncols))
        for i in range(self.nrows):
            for p in range(self.rp[i], self.rp[i + 1]):
                d[i, self.ci[p]] += float(self.va[p])
        return d


def first_unsorted_row(b):
    for r in range(b.nrows):
        c = b.ci[b.rp[r]: b.rp[r + 1]]
        if len(c) > 1 and (np.diff(c.astype(np.int64)) <= 0).any():
            return r
    return None


def products(a, b):
    """products[i] of the bound pass"""
    blen = np.diff(b.rp)
    return np.array([int(blen[a.ci[a.rp[i]: a.rp[i + 1]]].sum()) for i in range(a.nrows)], dtype=np.int64)


def row_classes(prod, group_limit=GROUP_LIMIT, block_limit=BLOCK_LIMIT):
    """(empty, group, block, spill) row counts"""
    prod = np.asarray(prod)
    return (int((prod == 0).sum()), int(((prod > 0) & (prod < group_limit)).sum()), int(((prod >= group_limit) & (prod < block_limit)).sum()),
            int((prod >= block_limit).sum()))


def spgemm(a, b):
    """C as a Csr of a's dtype, with .terms (the number of terms of every entry) and .absum (the sum of |a| |b| over them, fp64)"""
    assert a.ncols == b.nrows and a.va.dtype == b.va.dtype and first_unsorted_row(b) is None
    T = a.va.dtype.type
    rp, ci, va, terms, absum = [0], [], [], [], []
    with np.errstate(all="ignore"):
        for i in range(a.nrows):
            acc, cnt, ab = {}, {}, {}
            for p in range(a.rp[i], a.rp[i + 1]):
                k = a.ci[p]
                x = a.va[p]
                for q in range(b.rp[k], b.rp[k + 1]):
                    j = int(b.ci[q])
                    t = T(x * b.va[q])
                    acc[j] = T(acc.get(j, T(0)) + t)
                    cnt[j] = cnt.get(j, 0) + 1
                    ab[j] = ab.get(j, 0.0) + abs(float(x)) * abs(float(b.va[q]))
            for j in sorted(acc):
                ci.append(j)
                va.append(acc[j])
                terms.append(cnt[j])
                absum.append(ab[j])
            rp.append(len(ci))
    c = Csr(a.nrows, b.ncols, rp, np.array(ci, dtype=np.int32), np.array(va, dtype=a.va.dtype))
    c.terms, c.absum = np.array(terms, dtype=np.int64), np.array(absum, dtype=np.float64)
    return c


# ---- cases ----
def _values(n, seed, dtype):
    """seeded values in +-[0.5, 1.5) with a few more bits than fp32 holds"""
    r = np.random.default_rng(seed)
    return ((r.random(n) + 0.5) * r.choice([-1.0, 1.0], n)).astype(dtype)


def banded(n, dtype, seed=1):
    rows = [[j for j in (i - 3, i - 1, i, i + 1, i + 2) if 0 <= j < n] for i in range(n)]
    return from_rows(n, n, rows, dtype, seed)


def from_rows(nrows, ncols, rows, dtype, seed=1):
    rp = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    ci = np.array([j for r in rows for j in r], dtype=np.int32)
    return Csr(nrows, ncols, rp, ci, _values(len(ci), seed, dtype))


def laplacian(m, dtype):
    n, _, rp, ci, va = synth.laplacian_2d(m)
    return Csr(n, n, rp, ci, np.asarray(va).astype(dtype))


def random_csr(nrows, ncols, per_row, dtype, seed, sort=True, duplicates=False):
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(nrows):
        k = int(r.integers(0, per_row + 1))
        c = r.choice(ncols, size=min(k, ncols), replace=False).tolist()
        if duplicates and c:
            c = c + [c[0]] + c[:2]
            r.shuffle(c)
        rows.append(sorted(c) if sort else c)
    return from_rows(nrows, ncols, rows, dtype, seed + 1)


def limit_pair(nproducts, distinct, dtype):
    """one row of A with `nproducts` products: distinct=True: all on different columns (a full table's worth); False: all on 3 columns"""
    if distinct:
        # A's row points at rows of B of 16 columns each (the last one shorter), all disjoint
        nb = (nproducts + 15) // 16
        rows_b = [list(range(16 * r, min(16 * r + 16, nproducts))) for r in range(nb)]
        a = from_rows(2, nb, [list(range(nb)), []], dtype, 3)
        return a, from_rows(nb, max(nproducts, 1), rows_b, dtype, 4)
    nb = (nproducts + 2) // 3
    rows_b = [[5, 70000, 70001][: min(3, nproducts - 3 * r)] for r in range(nb)]
    a = from_rows(2, nb, [list(range(nb)), []], dtype, 5)
    return a, from_rows(nb, 70002, rows_b, dtype, 6)


HASH_MULTIPLIER = 2654435761          # cvr_spgemm.hip, row_in_table: the home slot of column j in a table of 2^L slots is the top L bits of
HASH_INVERSE = pow(HASH_MULTIPLIER, -1, 1 << 32)          # uint32(j * HASH_MULTIPLIER); the multiplier is odd, so it has an inverse modulo 2^32
BLOCK_TABLE_LOG2 = 13                # the largest LDS table: 8192 slots


def home_slot(j, log2_slots):
    return ((int(j) * HASH_MULTIPLIER) & 0xFFFFFFFF) >> (32 - log2_slots)


def table_log2(nproducts, lo=6, hi=BLOCK_TABLE_LOG2):
    """the table of a row of that many products: the smallest power of two >= twice the products, at least 64 slots"""
    return min(hi, max(lo, (2 * int(nproducts) - 1).bit_length()))


def colliding_columns(ndistinct, end):
    """the `ndistinct` smallest columns whose home slot in the 8192-slot table is one given slot -- the last one (end: every probe chain wraps around
    the table) or slot 2730 -- and which therefore share their home slot in every smaller table too (its index is a prefix of the same bits)"""
    slot = (1 << BLOCK_TABLE_LOG2) - 1 if end else 2730
    h = (np.uint64(slot) << np.uint64(32 - BLOCK_TABLE_LOG2)) + np.arange(1 << (32 - BLOCK_TABLE_LOG2), dtype=np.uint64)
    j = np.sort((h * np.uint64(HASH_INVERSE)) & np.uint64(0xFFFFFFFF))[:ndistinct]
    assert len(j) == ndistinct and j[-1] < 2 ** 31 - 2
    return [int(x) for x in j]


def collision_pair(ndistinct, dtype, end=False):
    """a row whose `ndistinct` distinct columns all have ONE home slot in its table, whatever the table's size (64 .. 8192 slots): every insertion
    walks the whole probe chain, and the lanes of a step contend for the chain's end.  Each column is met once or twice.  end: the shared slot is the
    table's last, so the chain wraps to slot 0"""
    cols = colliding_columns(ndistinct, end)
    rows_b = [cols[r::4] for r in range(4)]
    a = from_rows(3, 4, [[0, 1, 2, 3, 1, 0], [], [2]], dtype, 7)
    return a, from_rows(4, cols[-1] + 1, rows_b, dtype, 8)


def cases(dtype):
    """name -> (A, B): the list the host and the GPU tests run"""
    out = {}
    for n in (1, 2, 63, 64, 65, 1025):
        a = banded(n, dtype)
        out[f"banded-{n}"] = (a, a)
    for m in (3, 24):
        a = laplacian(m, dtype)
        out[f"laplacian-{m}"] = (a, a)
    out["rect-7x130x5"] = (random_csr(7, 130, 40, dtype, 11, sort=False), random_csr(130, 5, 5, dtype, 12))
    out["duplicates"] = (random_csr(70, 90, 9, dtype, 13, sort=False, duplicates=True), random_csr(90, 80, 7, dtype, 14))
    a = random_csr(40, 40, 6, dtype, 15)
    keep = [[] if i % 3 == 0 else a.ci[a.rp[i]: a.rp[i + 1]].tolist() for i in range(40)]
    out["a-empty-rows"] = (from_rows(40, 40, keep, dtype, 16), random_csr(40, 33, 6, dtype, 17))
    b = random_csr(40, 33, 6, dtype, 18)
    keep = [[] if i % 2 == 0 else b.ci[b.rp[i]: b.rp[i + 1]].tolist() for i in range(40)]
    out["b-empty-rows"] = (random_csr(25, 40, 8, dtype, 19), from_rows(40, 33, keep, dtype, 20))
    out["nnz-a-0"] = (from_rows(5, 6, [[]] * 5, dtype), random_csr(6, 7, 4, dtype, 21))
    out["nnz-b-0"] = (random_csr(5, 6, 4, dtype, 22), from_rows(6, 7, [[]] * 6, dtype))
    out["m-0"] = (from_rows(0, 6, [], dtype), random_csr(6, 7, 4, dtype, 23))
    out["dense-row"] = (from_rows(3, 48, [[0], list(range(48)), [47, 1]], dtype, 24), from_rows(48, 100, [list(range(100))] * 48, dtype, 25))
    return out


CASE_NAMES = list(cases(np.float32))
COLLISIONS = [20, 40, 80, 170, 340, 680, 1360, 2700]          # 1.5 times as many products: a table of 64, 128, .., 8192 slots
COLLISION_NAMES = [f"collisions-{d}{e}" for d in COLLISIONS for e in ("", "-end")]
PLAN_CASES = ["laplacian-24", "duplicates", "collisions-340", "collisions-340-end", "mixed-3000"]          # rerun under lowered limits
MIXED_PRODUCTS = [0, 5, 40, 100, 0, 12, 70]


def mixed(dtype, m=3000, seed=31):
    """A of m rows whose products cycle through MIXED_PRODUCTS: a period of 7 divides no thread's range of ceil(m / 1024) = 3 consecutive rows in
    the bin and scan kernels, so every boundary between two classes falls inside some thread's range.  B: 150 rows of 5 entries and 50 rows of one,
    on 300 columns, so that a row of A meets columns more than once.  Under the default limits the classes are empty, group (5, 12) and block (40,
    70, 100); under 8:64 all four: group (5), block (12, 40), spill (70, 100)"""
    r = np.random.default_rng(seed)
    rows_b = [sorted(r.choice(300, size=5 if k < 150 else 1, replace=False).tolist()) for k in range(200)]
    rows_a = []
    for i in range(m):
        p = MIXED_PRODUCTS[i % 7]
        rows_a.append(sorted(r.choice(150, size=p // 5, replace=False).tolist()) + sorted((150 + r.choice(50, size=p % 5, replace=False)).tolist()))
    return from_rows(m, 200, rows_a, dtype, seed + 1), from_rows(200, 300, rows_b, dtype, seed + 2)


def named(name, dtype):
    if name == "mixed-3000":
        return mixed(dtype)
    if name.startswith("collisions-"):
        return collision_pair(int(name.split("-")[1]), dtype, end=name.endswith("-end"))
    return cases(dtype)[name]
