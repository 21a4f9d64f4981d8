"""The FSAI preconditioner (cvr_precond_fsai, cvr_fsai_factor_host) and cvr_pcg_device with it in numpy, written from the text of include/cvr_amd.h (not
from the kernels), beside krylov_model.py, whose recurrence, sums, trajectories and comparison it uses.

What the header fixes and this file does, in the header's order:
  * the pattern (`pattern`): row i keeps its columns <= i, of more than MAX_ROW the MAX_ROW nearest the diagonal; such a row is a truncated one;
  * the small matrix (`small_matrix`): S[a][b] for b <= a is the entry (p_a, p_b) of A, +0 when row p_a has no column p_b;
  * the right-looking LDL^T (`ldlt`): d_k = S[k][k], bad unless finite and > 0; l_ak = S[a][k] / d_k; S[a][b] = S[a][b] - l_ak * S[b][k] for
    k < b <= a -- ascending k, one product and one subtraction each;
  * the back substitution by columns (`back_substitute`): w_(m-1) = 1, the others +0; for b = m-1 .. 1, for a < b: w_a = w_a - l_ba * w_b;
  * the outputs (`factor`): Wa = T(w_a), Wb = T(w_a / d_(m-1));
  * the apply (`apply`): z = Wb^T (Wa r) through two product callbacks x -> T(M x) -- on the GPU cvr_spmv_device of handles made from the exported
    arrays, on the CPU the CSR loop rounded to T.
The arithmetic is Python's float (IEEE fp64, one rounding per operation, never fused)."""
import math

import numpy as np

import krylov_model as KM
from cvr_amd import synth

MAX_ROW = 32          # CVR_FSAI_MAX_ROW


def pattern(rp, ci):
    """(W's row_ptr, W's col_idx, src, max_row, truncated_rows): src[i] is where row i's first kept entry lies in A's arrays.  The header's structure
    rules are asserted."""
    n = len(rp) - 1
    wrp, src = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    max_row = truncated = 0
    for i in range(n):
        cols = np.asarray(ci[rp[i]: rp[i + 1]], dtype=np.int64)
        assert (np.diff(cols) > 0).all(), f"row {i}: columns not strictly increasing"
        at = np.flatnonzero(cols == i)
        assert len(at) == 1, f"row {i}: no diagonal entry"
        m = int(at[0]) + 1
        if m > MAX_ROW:
            m, truncated = MAX_ROW, truncated + 1
        max_row = max(max_row, m)
        src[i] = rp[i] + at[0] - m + 1
        wrp[i + 1] = wrp[i] + m
    wci = np.concatenate([np.asarray(ci[src[i]: src[i] + wrp[i + 1] - wrp[i]], dtype=np.int32) for i in range(n)]) if n else np.zeros(0, dtype=np.int32)
    return wrp, wci.astype(np.int32), src, max_row, truncated


def lanes(max_row):
    """G: the power of two from the largest m up, 4 .. 64"""
    G = 4
    while G < max_row and G < 64:
        G <<= 1
    return G


def small_matrix(rows, p):
    """S as a list of lists (lower triangle; the rest 0.0): rows[r] = {column: fp64 value} of A"""
    m = len(p)
    return [[rows[p[a]].get(p[b], 0.0) if b <= a else 0.0 for b in range(m)] for a in range(m)]


def usable_pivot(d):
    return d > 0 and math.isfinite(d)


def ldlt(S):
    """(l as a list of lists with l[a][k] for a > k, d_(m-1)), or None at a bad pivot"""
    m = len(S)
    l = [[0.0] * m for _ in range(m)]
    d = 0.0
    for k in range(m):
        d = S[k][k]
        if not usable_pivot(d):
            return None
        for a in range(k + 1, m):
            l[a][k] = S[a][k] / d
        for a in range(k + 1, m):
            for b in range(k + 1, a + 1):
                S[a][b] = S[a][b] - l[a][k] * S[b][k]
    return l, d


def back_substitute(l):
    m = len(l)
    w = [0.0] * m
    w[m - 1] = 1.0
    for b in range(m - 1, 0, -1):
        for a in range(b):
            w[a] = w[a] - l[b][a] * w[b]
    return w


def factor(rp, ci, va, dtype):
    """(W's row_ptr, W's col_idx, Wa, Wb in T, the lowest row with a bad pivot or None): the rows from a bad one on stay 0"""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    wrp, wci, src, _, _ = pattern(rp, ci)
    a64 = np.asarray(va[: rp[-1]], dtype=T).astype(np.float64).tolist() if n else []
    cil = [int(c) for c in ci[: rp[-1]]] if n else []
    rows = [dict(zip(cil[rp[i]: rp[i + 1]], a64[rp[i]: rp[i + 1]])) for i in range(n)]
    wa, wb = np.zeros(int(wrp[n]), dtype=np.float64), np.zeros(int(wrp[n]), dtype=np.float64)
    bad = None
    with np.errstate(all="ignore"):
        for i in range(n):
            p = [int(c) for c in wci[wrp[i]: wrp[i + 1]]]
            out = ldlt(small_matrix(rows, p))
            if out is None:
                bad = i
                break
            l, dl = out
            w = back_substitute(l)
            wa[wrp[i]: wrp[i + 1]] = w
            wb[wrp[i]: wrp[i + 1]] = [x / dl for x in w]
        return wrp, wci, wa.astype(T), wb.astype(T), bad


def apply(product_a, product_bt, r):
    """z = Wb^T (Wa r): product_a is x -> T(Wa x), product_bt is x -> T(Wb^T x)"""
    return product_bt(product_a(r))


# ---- products on the CPU, for the host tests ----
def csr_product(n, rp, ci, va, dtype):
    """x -> T(A x), rows summed in fp64 (numpy's reduceat; every row has an entry)"""
    T = np.dtype(dtype).type
    rp, ci, v = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(va).astype(np.float64)

    def product(x):
        x = np.asarray(x).astype(np.float64)
        return np.add.reduceat(v * x[ci], rp[:-1]).astype(T) if n else np.zeros(0, dtype=T)

    return product


def transpose_csr(n, rp, ci, va):
    """the CSR of the transpose, the columns of a row ascending"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[: rp[-1]], dtype=np.int64)
    order = np.lexsort((rows, cols))
    rpt = np.zeros(n + 1, dtype=np.int64)
    rpt[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return rpt, rows[order].astype(np.int32), np.asarray(va[: rp[-1]])[order]


def cpu_products(n, wrp, wci, wa, wb, dtype):
    """(product_a, product_bt) of exported arrays"""
    trp, tci, tvb = transpose_csr(n, wrp, wci, wb)
    return csr_product(n, wrp, wci, wa, dtype), csr_product(n, trp, tci, tvb, dtype)


def dense(n, rp, ci, va):
    A = np.zeros((n, n))
    for i in range(n):
        A[i, ci[rp[i]: rp[i + 1]]] = np.asarray(va[rp[i]: rp[i + 1]], dtype=np.float64)
    return A


class FsaiPcg(KM.CgModel):
    """cvr_pcg_device with an FSAI object: cvr_cg_device's recurrence with z = Wb^T (Wa r)"""

    def __init__(self, product, dtype, product_a, product_bt, sums="tree"):
        super().__init__(product, dtype, sums)
        self.product_a, self.product_bt = product_a, product_bt

    def scale(self, minv, r):
        """z: the apply in place of T(minv * r)"""
        return apply(self.product_a, self.product_bt, r)

    def start(self, b, x0, minv):
        b, x, _, r = super().start(b, x0, None)
        return b, x, self, r          # (a preconditioner is present: r.z is a sum of its own)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def _full_csr(A, dtype):
    n = len(A)
    rp = np.arange(n + 1, dtype=np.int64) * n
    ci = np.tile(np.arange(n, dtype=np.int32), n)
    return n, n, rp, ci, A.reshape(-1).astype(dtype)


def dense_spd(n, dtype, seed=0):
    """B B^T / n + I with B standard normal, every entry stored"""
    B = np.random.default_rng(20261020 + seed + n).standard_normal((n, n))
    return _full_csr(B @ B.T / n + np.eye(n), dtype)


def arrow(n, dtype):
    """SPD: a diagonal in [2, 3), and a last row and column of entries in (-0.1, 0.1); the last row is full"""
    rng = np.random.default_rng(20261020 + n)
    d, v = 2.0 + rng.random(n), rng.uniform(-0.1, 0.1, n - 1)
    rp, ci, va = [0], [], []
    for i in range(n - 1):
        ci += [i, n - 1]
        va += [d[i], v[i]]
        rp.append(len(ci))
    ci += list(range(n))
    va += list(v) + [d[n - 1]]
    rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


def matrix(name, dtype):
    """(n, n, row_ptr, col_idx, vals) by name: spd-<n> (krylov_model.banded), laplacian-<m>, dense-<n> or arrow-<n>"""
    kind, _, size = name.partition("-")
    if kind == "spd":
        return KM.banded("spd", int(size), dtype)
    if kind == "laplacian":
        return synth.laplacian_2d(int(size), dtype)
    if kind == "dense":
        return dense_spd(int(size), dtype)
    assert kind == "arrow", name
    return arrow(int(size), dtype)


MATRICES = [f"spd-{n}" for n in (1, 2, 63, 64, 65, 1025)] + ["laplacian-3", "laplacian-24", "dense-8", "dense-32", "dense-40", "arrow-100"]
