"""The aggregation AMG preconditioner (cvr_precond_amg, cvr_amg_setup_host) and cvr_pcg_device with it in numpy, written from the text of
include/cvr_amd.h (not from the library's code), beside krylov_model.py, whose recurrence, sums, trajectories and comparison it uses.

What the header fixes and this file does, in the header's order:
  * the smoother diagonal (`smoother_diagonal`): d_i = the sum of |a_ij| in column order from +0, dinv_i = T(1 / d_i); a diagonal entry that is not
    finite or not > 0 is reported as (level, lowest such row);
  * the strength test (`strong_entries`): j != i, a_ij != 0 and a_ij * a_ij >= ((s * s) * a_ii) * a_jj;
  * the three passes of the aggregation (`aggregate`);
  * the coarse operator (`coarse_operator`): entry (I, J) is the sum from +0 of a_ij over the rows of I ascending, each row's entries in column
    order, rounded to T once; the rows come out sorted; the next level reads the rounded values;
  * the stopping rule and the coarsest level (`setup`): n <= coarse_size, max_levels levels, or a stall n_next > 0.8 * n; with n <= MAX_COARSE the
    explicit inverse of the dense matrix (`dense_inverse`), else 2 * sweeps smoother sweeps from zero;
  * the cycle (`cycle`) through one product callback x -> T(A_l x) per level -- on the GPU cvr_spmv_device of handles made from the exported
    levels, on the CPU the CSR loop rounded to T.
The arithmetic is IEEE fp64 with one rounding per operation (numpy's element-wise ufuncs never fuse); sums whose order matters run term by term."""
import math

import numpy as np

import krylov_model as KM
from cvr_amd import synth

MAX_LEVELS = 16          # CVR_AMG_MAX_LEVELS
MAX_COARSE = 256         # CVR_AMG_MAX_COARSE
DEFAULTS = dict(max_levels=16, coarse_size=64, sweeps=1, strength=0.08, coarse_scale=1.0)


def _f64(a):
    return np.asarray(a).astype(np.float64)


def segment_sums(v, starts, lengths):
    """s_k = +0 + v[starts_k] + v[starts_k + 1] + ..., left to right in fp64, for every segment at once"""
    s = np.zeros(len(starts), dtype=np.float64)
    for t in range(int(lengths.max()) if len(lengths) else 0):
        on = lengths > t
        s[on] = s[on] + v[starts[on] + t]
    return s


class Level:
    def __init__(self, n, rp, ci, va):
        self.n, self.rp, self.ci, self.va = n, rp, ci, va
        self.nnz = int(rp[n])
        self.dinv = self.agg = None
        self.nc = 0

    def rows(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rp))

    def diagonal(self):
        rows = self.rows()
        d = np.zeros(self.n, dtype=np.float64)
        at = np.flatnonzero(self.ci[: self.nnz] == rows)
        assert len(at) == self.n, "a diagonal entry in every row"
        d[rows[at]] = _f64(self.va[at])
        return d


class Hierarchy:
    def __init__(self, opts, dtype):
        self.opts, self.T = dict(opts), np.dtype(dtype).type
        self.levels, self.winv, self.bad = [], None, None          # bad: (level, row, what) of a failed set-up

    @property
    def coarse_direct(self):
        return self.winv is not None

    def operator_complexity(self):
        nnz0 = self.levels[0].nnz
        return float(sum(l.nnz for l in self.levels)) / float(nnz0) if nnz0 else 0.0

    def products_per_apply(self):
        s, L = self.opts["sweeps"], len(self.levels)
        return 2 * s * (L - 1) + (0 if self.coarse_direct else 2 * s - 1)


def check_structure(rp, ci):
    n = len(rp) - 1
    for i in range(n):
        cols = np.asarray(ci[rp[i]: rp[i + 1]], dtype=np.int64)
        assert (np.diff(cols) > 0).all(), f"row {i}: columns not strictly increasing"
        assert (cols == i).sum() == 1, f"row {i}: no diagonal entry"


def smoother_diagonal(lv, T):
    """(dinv in T, None) or (None, the lowest row whose diagonal entry is not finite or not > 0)"""
    d = lv.diagonal()
    bad = np.flatnonzero(~((d > 0) & np.isfinite(d)))
    if len(bad):
        return None, int(bad[0])
    s = segment_sums(np.abs(_f64(lv.va[: lv.nnz])), lv.rp[:-1], np.diff(lv.rp))
    return (1.0 / s).astype(T), None


def strong_entries(lv, strength):
    rows, cols, a, d = lv.rows(), lv.ci[: lv.nnz].astype(np.int64), _f64(lv.va[: lv.nnz]), lv.diagonal()
    return (cols != rows) & (a != 0) & (a * a >= ((strength * strength) * d[rows]) * d[cols])


def aggregate(lv, strength):
    """(agg[n], the number of aggregates)"""
    n, rp = lv.n, lv.rp
    strong = strong_entries(lv, strength)
    cols, mag = lv.ci[: lv.nnz].astype(np.int64), np.abs(_f64(lv.va[: lv.nnz]))
    nb = [cols[rp[i]: rp[i + 1]][strong[rp[i]: rp[i + 1]]] for i in range(n)]
    agg, nc = np.full(n, -1, dtype=np.int64), 0
    for i in range(n):          # pass 1
        if agg[i] < 0 and (agg[nb[i]] < 0).all():
            agg[i] = nc
            agg[nb[i]] = nc
            nc += 1
    first = agg.copy()
    for i in range(n):          # pass 2
        if agg[i] < 0:
            js = nb[i]
            ok = first[js] >= 0
            if ok.any():
                m = mag[rp[i]: rp[i + 1]][strong[rp[i]: rp[i + 1]]][ok]
                agg[i] = first[js[ok][int(np.argmax(m))]]          # (argmax: the first of equal ones, so the lowest j)
    for i in range(n):          # pass 3
        if agg[i] < 0:
            agg[i] = nc
            js = nb[i]
            agg[js[agg[js] < 0]] = nc
            nc += 1
    return agg.astype(np.int32), nc


def members(agg, nc):
    """(mrp[nc + 1], mem[n]): the rows of every aggregate, ascending"""
    mem = np.argsort(agg, kind="stable").astype(np.int32)
    mrp = np.zeros(nc + 1, dtype=np.int64)
    mrp[1:] = np.cumsum(np.bincount(agg, minlength=nc))
    return mrp, mem


def coarse_operator(lv, agg, nc, T):
    rows, cols, a = lv.rows(), lv.ci[: lv.nnz].astype(np.int64), _f64(lv.va[: lv.nnz])
    key = agg[rows].astype(np.int64) * nc + agg[cols]
    order = np.argsort(key, kind="stable")          # within a pair: the rows ascending, each row's entries in column order
    key, a = key[order], a[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, dtype=np.int64)
    lengths = np.diff(np.r_[starts, len(key)])
    vals = segment_sums(a, starts, lengths).astype(T)
    I, J = key[starts] // nc, key[starts] % nc
    rp = np.zeros(nc + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(I, minlength=nc))
    return Level(nc, rp, J.astype(np.int32), vals)


def dense_inverse(lv, T):
    """(W in T, None) or (None, the pivot that is not finite or not > 0): right-looking LDL^T of the lower triangle, L^-1 by columns, then
    W_ij = W_ji = T(sum over k = i .. n-1 ascending of (Linv_ki / d_k) * Linv_kj) for j <= i"""
    n = lv.n
    S = np.zeros((n, n), dtype=np.float64)
    rows = lv.rows()
    S[rows, lv.ci[: lv.nnz]] = _f64(lv.va[: lv.nnz])
    L, d = np.zeros((n, n)), np.zeros(n)
    for k in range(n):
        d[k] = S[k, k]
        if not (d[k] > 0 and math.isfinite(d[k])):
            return None, k
        L[k + 1:, k] = S[k + 1:, k] / d[k]
        S[k + 1:, k + 1:] = S[k + 1:, k + 1:] - np.outer(L[k + 1:, k], S[k + 1:, k])          # (only a >= b is read again)
    Y = np.eye(n)
    for k in range(n):
        Y[k + 1:, : k + 1] = Y[k + 1:, : k + 1] - np.outer(L[k + 1:, k], Y[k, : k + 1])
    W = np.zeros((n, n))
    for k in range(n):
        W[: k + 1, : k + 1] = W[: k + 1, : k + 1] + np.outer(Y[k, : k + 1] / d[k], Y[k, : k + 1])
    W = np.tril(W)
    W = W + np.tril(W, -1).T
    return W.astype(T), None


def setup(rp, ci, va, dtype, **kw):
    """the Hierarchy of a square CSR matrix; options as cvr_amg_options (DEFAULTS)"""
    opts = dict(DEFAULTS, **kw)
    T = np.dtype(dtype).type
    H = Hierarchy(opts, T)
    n = len(rp) - 1
    check_structure(rp, ci)
    nnz = int(rp[n])
    lv = Level(n, np.asarray(rp, dtype=np.int64).copy(), np.asarray(ci[:nnz], dtype=np.int32).copy(), np.asarray(va[:nnz], dtype=T).copy())
    with np.errstate(all="ignore"):
        while True:
            lv.dinv, bad = smoother_diagonal(lv, T)
            if bad is not None:
                H.bad = (len(H.levels), bad, "diagonal")
                return H
            H.levels.append(lv)
            if lv.n <= opts["coarse_size"] or len(H.levels) == opts["max_levels"]:
                break
            agg, nc = aggregate(lv, opts["strength"])
            if nc > 0.8 * lv.n:          # a stall: this level is the last
                break
            lv.agg, lv.nc = agg, nc
            lv = coarse_operator(lv, agg, nc, T)
        last = H.levels[-1]
        if last.n <= MAX_COARSE:
            H.winv, bad = dense_inverse(last, T)
            if bad is not None:
                H.bad = (len(H.levels) - 1, bad, "pivot")
    return H


# ---- the cycle ----
def smooth_first(lv, r, T):
    return (_f64(lv.dinv) * _f64(r)).astype(T)


def smooth_more(lv, z, r, q, T):
    return (_f64(z) + _f64(lv.dinv) * (_f64(r) - _f64(q))).astype(T)


def dense_apply(W, r, T):
    """z_i = T(t_0 + t_1 + ...), t_j = double(W_ij) * double(r_j), left to right from t_0"""
    W, r = _f64(W), _f64(r)
    if len(r) == 0:
        return np.zeros(0, dtype=T)
    s = W[:, 0] * r[0]
    for j in range(1, len(r)):
        s = s + W[:, j] * r[j]
    return s.astype(T)


def cycle(H, products, r, l=0):
    """z of level l for the right-hand side r (T values); products[l]: x -> T(A_l x)"""
    T, lv, sweeps = H.T, H.levels[l], H.opts["sweeps"]
    r = np.asarray(r, dtype=T)
    last = l == len(H.levels) - 1
    if last and H.coarse_direct:
        return dense_apply(H.winv, r, T)
    z = smooth_first(lv, r, T)
    for _ in range((2 * sweeps if last else sweeps) - 1):
        z = smooth_more(lv, z, r, products[l](z), T)
    if last:
        return z
    q = products[l](z)
    mrp, mem = members(lv.agg, lv.nc)
    rc = segment_sums((_f64(r) - _f64(q))[mem], mrp[:-1], np.diff(mrp)).astype(T)
    zc = cycle(H, products, rc, l + 1)
    z = (_f64(z) + H.opts["coarse_scale"] * _f64(zc)[lv.agg]).astype(T)
    for _ in range(sweeps):
        z = smooth_more(lv, z, r, products[l](z), T)
    return z


def apply(H, products, r):
    with np.errstate(all="ignore"):
        return cycle(H, products, r, 0)


# ---- products on the CPU, for the host tests ----
def csr_product(n, rp, ci, va, dtype):
    """x -> T(A x), every row summed left to right in fp64"""
    T = np.dtype(dtype).type
    rp, ci, v = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), _f64(va)

    def product(x):
        return segment_sums(v[: rp[-1]] * _f64(x)[ci[: rp[-1]]], rp[:-1], np.diff(rp)).astype(T)

    return product


def cpu_products(H):
    return [csr_product(l.n, l.rp, l.ci, l.va, H.T) for l in H.levels]


def dense(n, rp, ci, va):
    A = np.zeros((n, n))
    for i in range(n):
        A[i, ci[rp[i]: rp[i + 1]]] = _f64(va[rp[i]: rp[i + 1]])
    return A


def prolongator(lv):
    P = np.zeros((lv.n, lv.nc))
    P[np.arange(lv.n), lv.agg] = 1.0
    return P


class AmgPcg(KM.CgModel):
    """cvr_pcg_device with an AMG object: cvr_cg_device's recurrence with z = the cycle's"""

    def __init__(self, product, dtype, H, products, sums="tree"):
        super().__init__(product, dtype, sums)
        self.H, self.products = H, products

    def scale(self, minv, r):
        """z: the apply in place of T(minv * r)"""
        return apply(self.H, self.products, r)

    def start(self, b, x0, minv):
        b, x, _, r = super().start(b, x0, None)
        return b, x, self, r          # (a preconditioner is present: r.z is a sum of its own)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def _csr_of_dense(A, dtype):
    n = len(A)
    rp, ci, va = [0], [], []
    for i in range(n):
        for j in np.flatnonzero((A[i] != 0) | (np.arange(n) == i)):
            ci.append(int(j))
            va.append(A[i, j])
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


def singletons(dtype, n=90):
    """a chain -1, 2.5, -1 in which every third row holds its diagonal alone (and nothing points at it): singletons among coupled rows"""
    A = np.zeros((n, n))
    for i in range(n):
        A[i, i] = 2.5 + 0.01 * (i % 7)
        if i % 3 != 2 and i + 1 < n and (i + 1) % 3 != 2:
            A[i, i + 1] = A[i + 1, i] = -1.0
    return _csr_of_dense(A, dtype)


def two_blocks(dtype):
    """the 9 x 9 Laplacian (81 rows) and a chain of 40 rows, not connected"""
    n1, _, rp, ci, va = synth.laplacian_2d(9)
    n = n1 + 40
    A = np.zeros((n, n))
    A[:n1, :n1] = dense(n1, rp, ci, va)
    for i in range(n1, n):
        A[i, i] = 2.0
        if i + 1 < n:
            A[i, i + 1] = A[i + 1, i] = -1.0
    return _csr_of_dense(A, dtype)


def diagonal(dtype, n=300):
    d = 1.0 + np.arange(n) % 5
    return n, n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), d.astype(dtype)


def matrix(name, dtype):
    """(n, n, row_ptr, col_idx, vals) by name: spd-<n> (krylov_model.banded), laplacian-<m>, singletons, blocks, diagonal"""
    kind, _, size = name.partition("-")
    if kind == "spd":
        return KM.banded("spd", int(size), dtype)
    if kind == "laplacian":
        return synth.laplacian_2d(int(size), dtype)
    return {"singletons": singletons, "blocks": two_blocks, "diagonal": diagonal}[kind](dtype)


# (name, options): the shapes of the issue, then the two options that cut the hierarchy short
CASES = [(f"spd-{n}", {}) for n in (1, 2, 64, 65, 1025)] + [(f"laplacian-{m}", {}) for m in (3, 24, 40)] + [
    ("singletons", {}), ("blocks", {}), ("diagonal", {}), ("laplacian-24", dict(max_levels=1)), ("laplacian-24", dict(coarse_size=1)),
    ("laplacian-24", dict(sweeps=2, coarse_scale=1.5)), ("spd-1025", dict(strength=0.0, max_levels=2, sweeps=2))]


def case_id(c):
    return c[0] + "".join(f",{k}={v}" for k, v in c[1].items())


def from_export(info, levels, dtype):
    """the Hierarchy of exported levels (capi.AmgInfo and capi.AmgLevel objects): what a caller needs to carry out the cycle himself"""
    H = Hierarchy(dict(max_levels=info.max_levels, coarse_size=info.coarse_size, sweeps=info.sweeps, strength=info.strength, coarse_scale=info.coarse_scale), dtype)
    for e in levels:
        lv = Level(e.n, e.rp, e.ci, e.va)
        lv.dinv, lv.agg = e.dinv, e.agg
        lv.nc = int(e.agg.max()) + 1 if e.agg is not None and len(e.agg) else 0
        H.levels.append(lv)
    H.winv = levels[-1].winv if info.coarse_direct else None
    return H


def same_hierarchy(H, info, levels):
    """"" when the exported levels are the model's byte for byte, else what differs first"""
    if (info.levels, bool(info.coarse_direct)) != (len(H.levels), H.coarse_direct):
        return f"levels / coarse_direct = {(info.levels, info.coarse_direct)}, model {(len(H.levels), H.coarse_direct)}"
    for l, (m, g) in enumerate(zip(H.levels, levels)):
        if (info.n[l], info.nnz[l]) != (m.n, m.nnz):
            return f"level {l}: n / nnz = {(info.n[l], info.nnz[l])}, model {(m.n, m.nnz)}"
        if not (np.array_equal(m.rp, g.rp) and np.array_equal(m.ci, g.ci) and g.ci.dtype == np.int32):
            return f"level {l}: the pattern differs"
        for name in ("va", "dinv"):
            a, b = getattr(m, name), getattr(g, name)
            if a.dtype != b.dtype or a.tobytes() != b.tobytes():
                return f"level {l}: {name} differs"
        if (m.agg is None) != (g.agg is None) or (m.agg is not None and not np.array_equal(m.agg, g.agg)):
            return f"level {l}: agg differs"
    if H.coarse_direct and (H.winv.dtype != levels[-1].winv.dtype or H.winv.tobytes() != levels[-1].winv.tobytes()):
        return "winv differs"
    if any(info.n[len(H.levels):]) or any(info.nnz[len(H.levels):]) or any(info.reserved):
        return "words behind the levels are not 0"
    if info.operator_complexity != H.operator_complexity():
        return f"operator_complexity = {info.operator_complexity!r}, model {H.operator_complexity()!r}"
    return ""
