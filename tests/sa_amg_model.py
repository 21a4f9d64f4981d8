"""Smoothed-aggregation AMG (cvr_precond_amg_smoothed, cvr_amg_smoothed_setup_host) in numpy, written from the text of include/cvr_amd.h (not from
the library's code), on top of amg_model.py -- whose smoother diagonal, strength test, aggregation, stopping and stall rules, dense inverse and
smoothing steps it uses unchanged -- and of spgemm_model.spgemm, the only definition of a product's bits.

What the header adds and this file does, per level above the coarsest:
  1. T as a CSR: row_ptr = 0 .. n, col_idx = agg, vals = 1                                      (`tentative`)
  2. G = A T by the SpGEMM contract
  3. P on G's pattern: w_i = omega * double(dinv_i); p_ij = T([j == agg_i] - w_i * double(g_ij))   (`smooth_prolongator`)
  4. R = P^T, a stable transpose                                                                (`transpose`)
  5. A_next = R (A P), two products by the SpGEMM contract
and the cycle with 3'. t = T(r - q), r_next = R t and 5'. e = P z_next, z = T(z + coarse_scale * e), through product callbacks for A_l, P_l, R_l."""
import numpy as np

import amg_model as AM
import krylov_model as KM
import spgemm_model as SM

DEFAULT_OMEGA = 4.0 / 3.0
_f64 = AM._f64


def used_omega(omega):
    """0.0: the default; else finite with 0 < omega < 2"""
    if omega == 0.0:
        return DEFAULT_OMEGA
    assert 0 < omega < 2, omega
    return float(omega)


def tentative(lv, T):
    return SM.Csr(lv.n, lv.nc, np.arange(lv.n + 1, dtype=np.int64), lv.agg.astype(np.int32), np.ones(lv.n, dtype=T))


def smooth_prolongator(G, agg, dinv, omega, T):
    rows = np.repeat(np.arange(G.nrows, dtype=np.int64), np.diff(G.rp))
    w = omega * _f64(dinv)          # one rounding
    wg = w[rows] * _f64(G.va)          # one rounding
    own = (G.ci.astype(np.int64) == agg.astype(np.int64)[rows]).astype(np.float64)
    return SM.Csr(G.nrows, G.ncols, G.rp, G.ci, (own - wg).astype(T))


def transpose(P):
    """row J: P's entries of column J in ascending row of P"""
    rows = np.repeat(np.arange(P.nrows, dtype=np.int64), np.diff(P.rp))
    order = np.argsort(P.ci, kind="stable")
    rp = np.zeros(P.ncols + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(P.ci, minlength=P.ncols))
    return SM.Csr(P.ncols, P.nrows, rp, rows[order].astype(np.int32), P.va[order])


def coarsen(lv, omega, T):
    """(P, R, the next Level) of a level whose dinv, agg and nc are set"""
    A = SM.Csr(lv.n, lv.n, lv.rp, lv.ci, lv.va)
    P = smooth_prolongator(SM.spgemm(A, tentative(lv, T)), lv.agg, lv.dinv, omega, T)
    R = transpose(P)
    C = SM.spgemm(R, SM.spgemm(A, P))
    return P, R, AM.Level(lv.nc, C.rp, C.ci, C.va)


class Hierarchy(AM.Hierarchy):
    def __init__(self, opts, dtype, omega):
        super().__init__(opts, dtype)
        self.omega, self.P, self.R = omega, [], []

    def products_per_apply(self):
        s, L = self.opts["sweeps"], len(self.levels)
        return (2 * s + 2) * (L - 1) + (0 if self.coarse_direct else 2 * s - 1)


def setup(rp, ci, va, dtype, omega=0.0, **kw):
    """amg_model.setup with step `coarsen` in place of coarse_operator"""
    opts = dict(AM.DEFAULTS, **kw)
    T = np.dtype(dtype).type
    H = Hierarchy(opts, T, used_omega(omega))
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
            agg, nc = AM.aggregate(lv, opts["strength"])
            if nc > 0.8 * lv.n:
                break
            lv.agg, lv.nc = agg, nc
            P, R, lv = coarsen(lv, H.omega, T)
            H.P.append(P)
            H.R.append(R)
        last = H.levels[-1]
        if last.n <= AM.MAX_COARSE:
            H.winv, bad = AM.dense_inverse(last, T)
            if bad is not None:
                H.bad = (len(H.levels) - 1, bad, "pivot")
    return H


# ---- the cycle ----
def cycle(H, A, P, R, r, l=0):
    """z of level l; A[l], P[l], R[l]: x -> T(A_l x), T(P_l x), T(R_l x)"""
    T, lv, sweeps = H.T, H.levels[l], H.opts["sweeps"]
    r = np.asarray(r, dtype=T)
    last = l == len(H.levels) - 1
    if last and H.coarse_direct:
        return AM.dense_apply(H.winv, r, T)
    z = AM.smooth_first(lv, r, T)
    for _ in range((2 * sweeps if last else sweeps) - 1):
        z = AM.smooth_more(lv, z, r, A[l](z), T)
    if last:
        return z
    t = (_f64(r) - _f64(A[l](z))).astype(T)
    zc = cycle(H, A, P, R, R[l](t), l + 1)
    z = (_f64(z) + H.opts["coarse_scale"] * _f64(P[l](zc))).astype(T)
    for _ in range(sweeps):
        z = AM.smooth_more(lv, z, r, A[l](z), T)
    return z


def apply(H, A, P, R, r):
    with np.errstate(all="ignore"):
        return cycle(H, A, P, R, r, 0)


def cpu_products(H):
    """(A, P, R) product lists on the CPU: the CSR loop in fp64 rounded to T"""
    return (AM.cpu_products(H), [AM.csr_product(p.nrows, p.rp, p.ci, p.va, H.T) for p in H.P], [AM.csr_product(r.nrows, r.rp, r.ci, r.va, H.T) for r in H.R])


class SaAmgPcg(AM.AmgPcg):
    """cvr_pcg_device with a smoothed AMG object"""

    def __init__(self, product, dtype, H, A, P, R, sums="tree"):
        super().__init__(product, dtype, H, A, sums)
        self.P, self.R = P, R

    def scale(self, minv, r):
        return apply(self.H, self.products, self.P, self.R, r)


# ---- comparison with what the library exports ----
def from_export(info, sinfo, levels, prolongators, dtype):
    """the Hierarchy of exported levels and prolongators (capi.AmgInfo, AmgSmoothedInfo, AmgLevel and AmgProlongator objects)"""
    H = Hierarchy(dict(max_levels=info.max_levels, coarse_size=info.coarse_size, sweeps=info.sweeps, strength=info.strength, coarse_scale=info.coarse_scale), dtype, sinfo.omega)
    base = AM.from_export(info, levels, dtype)
    H.levels, H.winv = base.levels, base.winv
    H.P = [SM.Csr(p.n, p.nc, p.rp, p.ci, p.va) for p in prolongators]
    H.R = [transpose(p) for p in H.P]
    return H


def same_hierarchy(H, info, sinfo, levels, prolongators):
    """"" when levels and prolongators are the model's byte for byte and both infos fit, else what differs first"""
    what = AM.same_hierarchy(H, info, levels)
    if what:
        return what
    if (sinfo.smoothed, sinfo.omega, sinfo.products_per_apply) != (1, H.omega, H.products_per_apply()):
        return f"smoothed / omega / products_per_apply = {(sinfo.smoothed, sinfo.omega, sinfo.products_per_apply)}, model {(1, H.omega, H.products_per_apply())}"
    if len(prolongators) != len(H.P):
        return f"{len(prolongators)} prolongators, model {len(H.P)}"
    for l, (m, g) in enumerate(zip(H.P, prolongators)):
        if (sinfo.p_nnz[l], g.n, g.nc) != (len(m.ci), m.nrows, m.ncols):
            return f"P_{l}: p_nnz / n / nc = {(sinfo.p_nnz[l], g.n, g.nc)}, model {(len(m.ci), m.nrows, m.ncols)}"
        if not (np.array_equal(m.rp, g.rp) and np.array_equal(m.ci, g.ci) and g.ci.dtype == np.int32):
            return f"P_{l}: the pattern differs"
        if m.va.dtype != g.va.dtype or m.va.tobytes() != g.va.tobytes():
            return f"P_{l}: the values differ"
    if any(sinfo.p_nnz[len(H.P):]) or any(sinfo.reserved):
        return "words behind the prolongators are not 0"
    return ""


def zero_entry(dtype, n=120):
    """a chain -1, 3, -1 with a stored 0.0 two columns off the diagonal in every fifth row: structural zeros whose entries must stay in G and P"""
    rp, ci, va = [0], [], []
    for i in range(n):
        for j, v in ((i - 2, 0.0 if i % 5 == 0 else None), (i - 1, -1.0), (i, 3.0), (i + 1, -1.0), (i + 2, 0.0 if i % 5 == 3 else None)):
            if 0 <= j < n and v is not None:
                ci.append(j)
                va.append(v)
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va).astype(dtype)


def matrix(name, dtype):
    return zero_entry(dtype) if name == "zero-entry" else AM.matrix(name, dtype)


_CACHE = {}


def cached_setup(name, dtype, omega=0.0, **options):
    """the model's hierarchy of a named case, computed once per process (the Python SpGEMM is slow); nobody writes into it"""
    key = (name, np.dtype(dtype).name, omega, tuple(sorted(options.items())))
    if key not in _CACHE:
        n, _, rp, ci, va = matrix(name, dtype)
        _CACHE[key] = setup(rp, ci, va, dtype, omega, **options)
    return _CACHE[key]


def pcg_steps(m, rtol=1e-8, max_iters=400):
    """steps of the model's PCG on the m x m Laplacian in fp64 with krylov_model's right-hand side and stop rule: (smoothed, the Hierarchy)"""
    n = m * m
    H = cached_setup(f"laplacian-{m}", np.float64)
    A, P, R = cpu_products(H)
    b = KM.inputs(n, np.float64)[0]
    last = SaAmgPcg(A[0], np.float64, H, A, P, R).run(b, None, rtol=rtol, max_iters=max_iters).last
    assert last.terminal and last.status == KM.CONVERGED
    return last.iterations, H
