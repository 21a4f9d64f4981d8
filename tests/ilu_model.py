"""The ILU(0) preconditioner (cvr_precond_ilu0) and the solvers that take it in numpy, written from the text of include/cvr_amd.h (not from the
kernels), beside krylov_model.py, gmres_model.py and precond_model.py, whose recurrences, sums, trajectories and comparison it uses.

What the header fixes and this file does, in the header's order:
  * the levels (`levels`): row i of L has level 0 without an entry left of the diagonal, else 1 + the largest level among those columns; U the same
    from the last row backwards over the entries right of the diagonal;
  * the launch plan (`plan`): a level of at least `wide` rows is a launch of its own, a run of consecutive narrower levels is one launch;
  * the factorisation (`factor`): on an fp64 copy, row after row, for each k < i of the row in column order a_ik = a_ik / a_kk, then
    a_ij = a_ij - a_ik * a_kj for every j > k of row k that row i has, each operation rounded on its own; rounded once to T at the end;
  * the apply (`apply`): lane l of a row's G lanes adds double(f_ij) * double(v_j) over the entries l, l + G, .. of the row's part of the triangle
    from +0, left to right; the lanes by the xor butterfly G/2 .. 1 (`butterfly`); y_i = T(double(r_i) - s), z_i = T((double(y_i) - s) / double(u_ii));
  * the solvers: cvr_cg_device's, cvr_bicgstab_device's and cvr_gmres_device's recurrences with this apply where they have T(minv * r); GMRES forms x
    from the fp64 combination u by the same two sweeps with u where L's sweep has double(r): x = T(double(x) + double(zu)).
The arithmetic is Python's float (IEEE fp64, one rounding per operation, never fused) in the apply and numpy's fp64 scalars in the factorisation."""
import functools

import numpy as np

import krylov_model as KM
from gmres_model import GmresModel
from krylov_model import _f64

DEFAULT_WIDE = 512          # include/cvr_amd.h: wide_threshold without CVR_DEBUG=ilu_wide


def diagonal_positions(rp, ci):
    """where each row's diagonal lies; the header's three structure rules are asserted"""
    n = len(rp) - 1
    d = np.zeros(n, dtype=np.int64)
    for i in range(n):
        cols = np.asarray(ci[rp[i]: rp[i + 1]], dtype=np.int64)
        assert (np.diff(cols) > 0).all(), f"row {i}: columns not strictly increasing"
        at = np.flatnonzero(cols == i)
        assert len(at) == 1, f"row {i}: no diagonal entry"
        d[i] = rp[i] + at[0]
    return d


def levels(rp, ci):
    """(lower_level, upper_level, n_lower, n_upper)"""
    n = len(rp) - 1
    d = diagonal_positions(rp, ci)
    lo, up = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        cols = ci[rp[i]: d[i]]
        lo[i] = 0 if len(cols) == 0 else 1 + max(lo[c] for c in cols)
    for i in range(n - 1, -1, -1):
        cols = ci[d[i] + 1: rp[i + 1]]
        up[i] = 0 if len(cols) == 0 else 1 + max(up[c] for c in cols)
    return lo, up, (int(lo.max()) + 1 if n else 0), (int(up.max()) + 1 if n else 0)


def widths(level, nlevels):
    return np.bincount(np.asarray(level, dtype=np.int64), minlength=nlevels)[:nlevels] if nlevels else np.zeros(0, dtype=np.int64)


def plan(level, nlevels, wide=DEFAULT_WIDE):
    """the launches of one sweep: [(first level, number of levels, merged)]"""
    out = []
    for l, w in enumerate(widths(level, nlevels).tolist()):
        if w >= wide:
            out.append((l, 1, False))
        elif out and out[-1][2] and out[-1][0] + out[-1][1] == l:
            out[-1] = (out[-1][0], out[-1][1] + 1, True)
        else:
            out.append((l, 1, True))
    return out


def default_lanes(n, nnz):
    """G: the power of two from ceil((nnz - n) / (2 n)) up, 1 .. 64"""
    mean = -(-(nnz - n) // (2 * n)) if n > 0 else 0
    G = 1
    while G < mean and G < 64:
        G <<= 1
    return G


def butterfly(s):
    """s: G fp64 values (G a power of two) -> what every lane holds behind s += s[lane ^ o] for o = G/2 .. 1"""
    s = list(s)
    o = len(s) >> 1
    while o > 0:
        s = [s[l] + s[l ^ o] for l in range(len(s))]
        o >>= 1
    return s[0]


def factor(rp, ci, va, dtype):
    """(the factors in T in the CSR's positions, the lowest row whose pivot is zero or not finite or None)"""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    d = diagonal_positions(rp, ci)
    a = np.asarray(va[: rp[-1]], dtype=T).astype(np.float64)
    bad = None
    with np.errstate(all="ignore"):
        for i in range(n):
            where = {int(ci[q]): q for q in range(rp[i], rp[i + 1])}
            for q in range(rp[i], d[i]):
                k = int(ci[q])
                a[q] = a[q] / a[d[k]]
                for pk in range(d[k] + 1, rp[k + 1]):
                    pi = where.get(int(ci[pk]))
                    if pi is not None:
                        a[pi] = a[pi] - a[q] * a[pk]
            if bad is None and not (a[d[i]] != 0 and np.isfinite(a[d[i]])):
                bad = i
    return a.astype(T), bad


def _sweep(rp, ci, d, f, rhs, G, T, upper):
    n = len(rp) - 1
    v = [0.0] * n
    for i in (range(n - 1, -1, -1) if upper else range(n)):          # (any order that respects the levels gives the same values)
        beg, end = (d[i] + 1, rp[i + 1]) if upper else (rp[i], d[i])
        s = [0.0] * G
        for e, q in enumerate(range(beg, end)):
            s[e % G] = s[e % G] + f[q] * v[ci[q]]
        t = rhs[i] - butterfly(s)
        if upper:
            t = t / f[d[i]]
        v[i] = float(T(t))
    return v


def apply(rp, ci, f, r, G, dtype, rhs_is_fp64=False):
    """z = U^-1 L^-1 r by the header's arithmetic: f the exported factors (T), r n values of T -- or of fp64, used as they are (rhs_is_fp64: GMRES's u)"""
    T = np.dtype(dtype).type
    rp_, ci_ = [int(v) for v in rp], [int(v) for v in ci[: rp[-1]]]
    d = [int(v) for v in diagonal_positions(rp, ci)]
    fl = np.asarray(f, dtype=T).astype(np.float64).tolist()
    rl = (np.asarray(r, dtype=np.float64) if rhs_is_fp64 else np.asarray(r, dtype=T).astype(np.float64)).tolist()
    with np.errstate(all="ignore"):
        y = _sweep(rp_, ci_, d, fl, rl, G, T, False)
        z = _sweep(rp_, ci_, d, fl, y, G, T, True)
    return np.array(z, dtype=np.float64).astype(T)


class Ilu:
    """an object: the pattern, the factors as exported, G"""

    def __init__(self, rp, ci, f, G, dtype):
        self.rp, self.ci, self.f, self.G, self.T = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(f), int(G), np.dtype(dtype).type

    @classmethod
    def of(cls, rp, ci, va, dtype, G=None):
        f, bad = factor(rp, ci, va, dtype)
        assert bad is None, bad
        n = len(rp) - 1
        return cls(rp, ci, f, default_lanes(n, int(rp[-1])) if G is None else G, dtype)

    def apply(self, r, rhs_is_fp64=False):
        return apply(self.rp, self.ci, self.f, r, self.G, self.T, rhs_is_fp64)


class _Object:
    def set_object(self, ilu):
        self.ilu = ilu

    def scale(self, minv, r):
        """z: the apply in place of T(minv * r)"""
        return self.ilu.apply(r)


class IluPcg(_Object, KM.CgModel):
    """cvr_pcg_device with an ILU(0) object"""

    def __init__(self, product, dtype, ilu, sums="tree"):
        KM.CgModel.__init__(self, product, dtype, sums)
        self.set_object(ilu)

    def start(self, b, x0, minv):
        b, x, _, r = super().start(b, x0, None)
        return b, x, self, r          # (a preconditioner is present: r.z is a sum of its own)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


class IluBicgstab(_Object, KM.BicgstabModel):
    """cvr_pbicgstab_device with an ILU(0) object: p^ = M^-1 p, s^ = M^-1 s"""

    def __init__(self, product, dtype, ilu, sums="tree"):
        KM.BicgstabModel.__init__(self, product, dtype, sums)
        self.set_object(ilu)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


class IluGmres(_Object, GmresModel):
    """cvr_pgmres_device with an ILU(0) object: z_j = M^-1 v_j, and x from the fp64 u through the same two sweeps"""

    def __init__(self, product, dtype, ilu, sums="tree", restart=30):
        GmresModel.__init__(self, product, dtype, sums, restart)
        self.set_object(ilu)

    def form_x(self, x, minv, R, g, V, q):
        if q == 0:
            return x
        u = self.combination(self.back_substitute(R, g, q), V[:q])
        return self.rnd(_f64(x) + _f64(self.ilu.apply(u, rhs_is_fp64=True)))

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def wide_matrix(dtype, n=4097):
    """two levels in L: the first (n + 1) // 2 rows are diagonal only, each later row has two columns in the first half plus the diagonal"""
    half = (n + 1) // 2
    rp, ci, va = [0], [], []
    rng = np.random.default_rng(20261019)
    for i in range(n):
        if i >= half:
            a, b = sorted(((i * 7) % half, (i * 13 + 5) % half))
            if a == b:
                b = (a + 1) % half
                a, b = sorted((a, b))
            ci += [a, b]
            va += [rng.uniform(-0.5, 0.5) / 2, rng.uniform(-0.5, 0.5) / 2]
        ci.append(i)
        va.append(1.0 + rng.random())
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


def transpose(n, rp, ci, va):
    """the CSR of A^T, the columns of a row ascending"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[: rp[-1]], dtype=np.int64)
    order = np.lexsort((rows, cols))
    rpt = np.zeros(n + 1, dtype=np.int64)
    rpt[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return n, n, rpt, rows[order].astype(np.int32), np.asarray(va[: rp[-1]])[order]


def _irregular_triangle(n, rng, kmax, near, shallow):
    """per row i the ascending columns left of the diagonal: about one row in six has none, the others draw k in [1, min(i, kmax)] columns, each one of
    the `near` columns just left of i or uniform in [0, i) (a coin decides; a column drawn twice counts once).  shallow > 0: that share of the rows
    with columns draws them uniformly among the earlier rows that have none instead -- rows of level 1"""
    rows, roots = [np.zeros(0, dtype=np.int64)], [0]
    for i in range(1, n):
        if rng.random() < 1.0 / 6.0:
            rows.append(np.zeros(0, dtype=np.int64))
            roots.append(i)
            continue
        k = int(rng.integers(1, min(i, kmax) + 1))
        if shallow > 0 and rng.random() < shallow:
            rows.append(np.unique(rng.choice(roots, size=k)).astype(np.int64))
            continue
        close = i - 1 - rng.integers(0, min(near, i), size=k)
        far = rng.integers(0, i, size=k)
        rows.append(np.unique(np.where(rng.random(k) < 0.5, close, far)).astype(np.int64))
    return rows


def irregular(n, seed, sym, kmax, dtype, near=8, shallow=0.0):
    """(n, n, row_ptr, col_idx, vals) of an irregular matrix that ILU(0) factors without a bad pivot: rows of unrelated lengths (0 .. kmax entries in a
    triangle), level-0 rows scattered through the matrix, neighbouring and far columns mixed.  sym: the upper triangle mirrors the lower one, pattern and
    values; else it is drawn on its own in the same way from the last row back (row i's columns right of the diagonal among i + 1 .. i + near or uniform
    in (i, n)).  Off-diagonal values uniform in (-1, 1), the diagonal 1 + the sum of the row's |off-diagonals| + U(0, 1): strictly row dominant.
    shallow: the share of rows of level 1 (_irregular_triangle); 0 but for irr-nonsym-2500, where a level of 512 rows behind a narrower level 0 is
    wanted: with columns uniform in [0, i) a level behind level 0 holds less than level 0's share times the rest, never a fifth of the rows.
    Everything comes from np.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    lower = _irregular_triangle(n, rng, kmax, near, shallow)
    lower_vals = [rng.uniform(-1.0, 1.0, size=len(c)) for c in lower]
    upper, upper_vals = [[] for _ in range(n)], [[] for _ in range(n)]
    if sym:
        for i in range(n):
            for c, v in zip(lower[i].tolist(), lower_vals[i].tolist()):          # (rows ascending: every upper row comes out ascending)
                upper[c].append(i)
                upper_vals[c].append(v)
    else:
        mirrored = _irregular_triangle(n, rng, kmax, near, shallow)
        for i in range(n):
            upper[i] = (n - 1 - mirrored[n - 1 - i])[::-1].tolist()
            upper_vals[i] = rng.uniform(-1.0, 1.0, size=len(upper[i])).tolist()
    rp, ci, va = [0], [], []
    for i in range(n):
        off = lower_vals[i].tolist() + list(upper_vals[i])
        ci += lower[i].tolist() + [i] + list(upper[i])
        va += lower_vals[i].tolist() + [1.0 + float(np.abs(off).sum()) + rng.random()] + list(upper_vals[i])
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


# name -> (n, seed, sym, kmax, near, shallow): the irregular cases of tests/test_ilu_model_host.py (which holds each to its conditions) and of
# tests/test_gpu_ilu0_irregular.py
IRREGULAR = {
    "irr-spd-700": (700, 700, True, 6, 8, 0.0),
    "irr-nonsym-700": (700, 701, False, 6, 8, 0.0),
    "irr-dense-spd-320": (320, 320, True, 190, 8, 0.0),
    "irr-dense-nonsym-320": (320, 321, False, 320, 8, 0.0),
    "irr-nonsym-2500": (2500, 2500, False, 3, 8, 0.3),
}


@functools.lru_cache(maxsize=None)
def irregular_case(name, prec):
    """(n, rp, ci, va, f, lo, up, nlo, nup, threshold) of a named case in "fp64" or "fp32": the matrix, the model's factors (no bad pivot), its levels and
    width_threshold -- computed once and shared, nobody writes to them"""
    dtype = np.float64 if prec == "fp64" else np.float32
    n, seed, sym, kmax, near, shallow = IRREGULAR[name]
    n, _, rp, ci, va = irregular(n, seed, sym, kmax, dtype, near, shallow)
    f, bad = factor(rp, ci, va, dtype)
    assert bad is None, (name, prec, bad)
    for a in (rp, ci, va, f):
        a.setflags(write=False)
    return (n, rp, ci, va, f) + levels(rp, ci) + (width_threshold(rp, ci),)


def width_threshold(rp, ci):
    """a wide_threshold from the matrix's own level widths, max(2, the median width over both sweeps): about half of the levels are wide, half merged"""
    lo, up, nlo, nup = levels(rp, ci)
    return max(2, int(np.median(np.concatenate([widths(lo, nlo), widths(up, nup)]))))


def dense_lu(n, rp, ci, f):
    """(L, U) dense in fp64 from exported factors"""
    L, U = np.eye(n), np.zeros((n, n))
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            (L if ci[q] < i else U)[i, ci[q]] = np.float64(f[q])
    return L, U
