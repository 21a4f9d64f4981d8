"""The thick-restart Golub-Kahan-Lanczos recurrence of cvr_svds_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the
model the singular-value tests compare the device with, bit for bit.  The conventions are tests/krylov_model.py's and tests/lanczos_model.py's: every
stored vector is rounded to the handles' type T once, scalars are fp64, a sum's terms are `double(a_i) * double(b_i)` added in the documented tree
(krylov_model.tree_sum), and the matrix enters through two callbacks, `product` (x -> T(A x)) and `product_t` (y -> T(A^T y)).  The projected matrix is
taken apart by the library's own cvr_svd_host (capi.svd_host), an ingredient exactly as the products are: tests/test_svds_host.py holds it to LAPACK
on its own.

One method per operation of the header, so that a mutant (tests/test_svds_model_host.py) is the model with one method replaced."""
import numpy as np

from cvr_amd import capi
from krylov_model import _f64, _Model

CONVERGED, MAX_RESTARTS, BREAKDOWN, INVARIANT = 0, 1, 2, 3          # CVR_EIG_* of include/cvr_amd.h
EPS23 = 3.666852862501036e-11          # the header's literal


def default_ncv(nrows, ncols, nev):
    return min(min(nrows, ncols), max(2 * nev + 1, 20), 64)


class SvdEntry:
    """what the device returns: svals (the count returned, descending), U (nrows x count) and V (ncols x count), and the result's fields"""

    def __init__(self, svals, U, V, nconv, status, restarts, spmv_count, max_estimate, **scalars):
        self.svals, self.U, self.V = np.asarray(svals, dtype=np.float64), U, V
        self.nconv, self.status, self.restarts, self.spmv_count = int(nconv), int(status), int(restarts), int(spmv_count)
        self.max_estimate = np.float64(max_estimate)
        self.scalars = scalars

    def __repr__(self):
        return (f"SvdEntry(svals={self.svals!r}, nconv={self.nconv}, status={self.status}, restarts={self.restarts}, spmv_count={self.spmv_count}, "
                f"max_estimate={self.max_estimate!r})")


def _block_difference(name, g, w):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    if g.dtype != w.dtype or g.shape != w.shape:
        return f"{name} is {g.dtype}{g.shape}, model {w.dtype}{w.shape}"
    if g.tobytes() != w.tobytes():
        d = np.argwhere((g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,))).any(axis=-1))
        i, c = (int(v) for v in d[0])
        return f"{name} differs in {len(d)} of {g.size} values, first at row {i} of column {c}: {g[i, c]!r}, model {w[i, c]!r}"
    return ""


def compare(got, want, vectors=True):
    """the one comparison of a result with a model entry: svals bit for bit, U and V byte for byte, nconv, status, restarts, spmv_count equal,
    max_estimate equal as bits.  `vectors`: True, False, or "U" / "V" for one block alone.  Returns "" when they agree, else what differs."""
    bad = []
    for name in ("nconv", "status", "restarts", "spmv_count"):
        if getattr(got, name) != getattr(want, name):
            bad.append(f"{name} = {getattr(got, name)}, model {getattr(want, name)}")
    if np.float64(got.max_estimate).tobytes() != np.float64(want.max_estimate).tobytes():
        bad.append(f"max_estimate = {got.max_estimate!r}, model {want.max_estimate!r}")
    gs, ws = np.ascontiguousarray(got.svals, dtype=np.float64), np.ascontiguousarray(want.svals, dtype=np.float64)
    if gs.shape != ws.shape or gs.tobytes() != ws.tobytes():
        bad.append(f"svals = {gs!r}, model {ws!r}")
    for name in ("U", "V"):
        if vectors is True or vectors == name:
            msg = _block_difference(name, getattr(got, name), getattr(want, name))
            if msg:
                bad.append(msg)
    return "; ".join(bad)


class SvdsModel(_Model):
    """cvr_svds_device"""

    def __init__(self, product, product_t, dtype, sums="tree"):
        super().__init__(product, dtype, sums)
        self.product_t = product_t

    # ---- the single operations of the header ----
    def coefficients(self, B, w):
        """c_i = b_i . w for every column, all on the same w"""
        return np.array([self.dot("b.w", b, w) for b in B])

    def subtract(self, B, c, w):
        """t = double(w); t = t - c_0 double(b_0); ...; w = T(t)"""
        t = _f64(w)
        for ci, b in zip(c, B):
            t = t - ci * _f64(b)
        return self.rnd(t)

    def passes(self, B, w):
        """classical Gram-Schmidt against the columns B, twice: (w behind pass 1, w behind pass 2, the coefficients of the two passes)"""
        h = self.coefficients(B, w)
        w1 = self.subtract(B, h, w)
        d = self.coefficients(B, w1)
        return w1, self.subtract(B, d, w1), h, d

    def first_sum(self, w0, w1):
        """ww1: of w behind pass 1"""
        return self.dot("w.w", w1, w1)

    def norm_entry(self, ww, h, d):
        """alpha_j / beta_(j+1) = sqrt(ww): the norm, not a coefficient"""
        return np.sqrt(ww)

    def closed(self, ww1, ww):
        """the half is closed: the second pass halved the norm once more (a zero norm included)"""
        return bool(ww <= 0.25 * ww1)

    def normalise(self, w, by):
        return self.rnd(_f64(w) / by)

    def left_columns(self, U, j):
        """the left half of step j works against u_0 .. u_(j-1)"""
        return U[:j]

    def right_columns(self, V, j):
        """the right half of step j works against v_0 .. v_j"""
        return V[:j + 1]

    def spike(self, beta_m, Q, kk):
        """s_c = beta_m * Q[m-1, c] of the kept triplets"""
        return np.array([beta_m * Q[-1, c] for c in range(kk)])

    def projected(self, p, q, k, sigma, spike, alpha, beta):
        """the p x q matrix: the kept values with their spike in column k, upper bidiagonal beyond"""
        B = np.zeros((p, q))
        for c in range(min(k, p)):
            B[c, c] = sigma[c]
            if k < q:
                B[c, k] = spike[c]
        for j in range(k, p):
            B[j, j] = alpha[j]
            if j + 1 < q:
                B[j, j + 1] = beta[j + 1]
        return B

    def small_svd(self, B):
        return capi.svd_host(B)

    def select(self, p, count):
        """the `count` leading triplets, descending"""
        return list(range(count))

    def estimate(self, beta_m, Q, P, p, c):
        """e_c = |beta_m * Q[p-1, c]|"""
        return abs(beta_m * Q[p - 1, c])

    def keep(self, nev, nconv, m):
        """k = nev + min(nconv, (m - nev) / 2)"""
        return nev + min(nconv, (m - nev) // 2)

    def restart_sum(self, s, B):
        """u = +0; u = u + S[l, c] * double(b_l), l ascending; T(u)"""
        u = np.zeros(len(B[0]))
        for sl, b in zip(s, B):
            u = u + sl * _f64(b)
        return self.rnd(u)

    def carry(self, V, m):
        """the new v_k: the old v_m"""
        return V[m]

    # ---- the run ----
    def run(self, v0, nrows, nev=1, ncv=0, tol=1e-8, max_restarts=100):
        with np.errstate(all="ignore"):
            return self._run(np.ascontiguousarray(v0, dtype=self.T), int(nrows), int(nev), int(ncv), np.float64(tol), int(max_restarts))

    def _run(self, v0, nr, nev, ncv, tol, max_restarts):
        nc = len(v0)
        m = ncv if ncv else default_ncv(nr, nc, nev)
        assert nev >= 1 and nev + 2 <= m <= min(nr, nc, 64), (nr, nc, nev, m)
        noU, noV = np.zeros((nr, 0), dtype=self.T), np.zeros((nc, 0), dtype=self.T)
        self.history = []          # history[r]: what the same call returns with max_restarts = r (the last entry: for every larger one, when it is final)
        s = self.dot("v0.v0", v0, v0)
        # (the steps are enqueued before the start's stop is known: the first cycle counts in any case)
        if not (s > 0 and np.isfinite(s)):
            return SvdEntry([], noU, noV, 0, BREAKDOWN, 0, 2 * m, 0.0, s=s)
        V, U = [self.normalise(v0, np.sqrt(s))], []
        k, restarts, spmvs = 0, 0, 0
        sigma, spike = np.zeros(0), np.zeros(0)
        while True:
            alpha, beta = np.zeros(m), np.zeros(m + 1)
            spmvs += 2 * (m - k)          # a whole cycle is enqueued, whatever ends it
            p, q, closed = m, m, False
            for j in range(k, m):
                w0 = self.product(V[j])
                w1, w, h, d = self.passes(self.left_columns(U, j), w0)
                ww1, ww = self.first_sum(w0, w1), self.dot("w.w", w, w)
                if not (np.isfinite(ww1) and np.isfinite(ww)):
                    return SvdEntry([], noU, noV, 0, BREAKDOWN, restarts, spmvs, 0.0, ww=ww, j=j, half="left")
                alpha[j] = self.norm_entry(ww, h, d)
                if self.closed(ww1, ww):
                    p, q, closed = j, j + 1, True
                    break
                U.append(self.normalise(w, alpha[j]))
                z0 = self.product_t(U[j])
                z1, z, h, d = self.passes(self.right_columns(V, j), z0)
                zz1, zz = self.first_sum(z0, z1), self.dot("z.z", z, z)
                if not (np.isfinite(zz1) and np.isfinite(zz)):
                    return SvdEntry([], noU, noV, 0, BREAKDOWN, restarts, spmvs, 0.0, zz=zz, j=j, half="right")
                beta[j + 1] = self.norm_entry(zz, h, d)
                if self.closed(zz1, zz):
                    p, q, closed = j + 1, j + 1, True
                    break
                V.append(self.normalise(z, beta[j + 1]))
            if p == 0:          # A v_0 = 0: nothing to return
                entry = SvdEntry([], noU, noV, 0, INVARIANT, restarts, spmvs, 0.0, p=0)
                self.history.append(entry)
                return entry
            sv, Q, P = self.small_svd(self.projected(p, q, k, sigma, spike, alpha, beta))
            want = min(nev, p)
            sel = self.select(p, want)
            bq = 0.0 if closed else beta[m]
            est = np.array([self.estimate(bq, Q, P, p, c) for c in sel])
            scale = np.maximum(EPS23, sv[sel])
            nconv = int(np.count_nonzero(est <= tol * scale))
            worst = float(np.max(est / scale))
            done = closed or nconv == nev
            # what the call returns when it ends here (for max_restarts = restarts, or for good)
            status = (CONVERGED if p >= nev else INVARIANT) if closed else CONVERGED if done else MAX_RESTARTS
            Uo = np.stack([self.restart_sum(Q[:, c], U[:p]) for c in sel], axis=1)
            Vo = np.stack([self.restart_sum(P[:, c], V[:q]) for c in sel], axis=1)
            entry = SvdEntry(sv[sel], Uo, Vo, want if closed else nconv, status, restarts, spmvs, worst, sv=sv, Q=Q, P=P, beta=beta, alpha=alpha, est=est, p=p, q=q)
            self.history.append(entry)
            if done or restarts == max_restarts:
                return entry
            kk = self.keep(nev, nconv, m)
            sigma, spike = sv[:kk], self.spike(beta[m], Q, kk)
            U = [self.restart_sum(Q[:, c], U[:m]) for c in range(kk)]
            V = [self.restart_sum(P[:, c], V[:m]) for c in range(kk)] + [self.carry(V, m)]
            k = kk
            restarts += 1


def svds_model(product, product_t, v0, nrows, nev=1, ncv=0, tol=1e-8, max_restarts=100, dtype=np.float64, sums="tree"):
    return SvdsModel(product, product_t, dtype, sums).run(v0, nrows, nev, ncv, tol, max_restarts)


# ---- the cases the CPU and the GPU tests share ----
def band_rect(nrows, ncols, dtype, half_band=2, seed=0):
    """(nrows, ncols, row_ptr, col_idx, vals) of a random band around the stretched diagonal i -> i * ncols / nrows, entries in [-1, 1): nonsymmetric,
    of full rank in practice, every row with an entry"""
    rng = np.random.default_rng(20261021 + seed + 3 * nrows + ncols)
    rp, ci, va = [0], [], []
    for i in range(nrows):
        c = (i * ncols) // nrows
        for j in range(max(0, c - half_band), min(ncols, c + half_band + 1)):
            ci.append(j)
            va.append(float(dtype(rng.random() * 2 - 1)))
        rp.append(len(ci))
    return nrows, ncols, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def random_sparse(nrows, ncols, dtype, per_row=4, seed=0):
    """per_row distinct random columns in every row, entries standard normal"""
    rng = np.random.default_rng(20261021 + seed + 5 * nrows + ncols)
    rp, ci, va = [0], [], []
    for _ in range(nrows):
        cols = np.sort(rng.choice(ncols, size=min(per_row, ncols), replace=False))
        ci.extend(int(c) for c in cols)
        va.extend(float(dtype(v)) for v in rng.standard_normal(len(cols)))
        rp.append(len(ci))
    return nrows, ncols, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def from_dense(A, dtype):
    """the CSR of the non-zero entries of a dense matrix"""
    A = np.asarray(A)
    rp, ci, va = [0], [], []
    for i in range(A.shape[0]):
        for j in np.nonzero(A[i])[0]:
            ci.append(int(j))
            va.append(A[i, j])
        rp.append(len(ci))
    return A.shape[0], A.shape[1], np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def transpose_csr(nrows, ncols, rp, ci, va):
    """the CSR of A^T, columns ascending within a row"""
    rows = np.repeat(np.arange(nrows), np.diff(rp))
    order = np.lexsort((rows, ci))
    rpt = np.zeros(ncols + 1, dtype=np.int64)
    np.add.at(rpt, np.asarray(ci, dtype=np.int64) + 1, 1)
    return ncols, nrows, np.cumsum(rpt), rows[order].astype(np.int32), np.asarray(va)[order]


def dense_of(nrows, ncols, rp, ci, va):
    A = np.zeros((nrows, ncols))
    for i in range(nrows):
        for p in range(rp[i], rp[i + 1]):
            A[i, ci[p]] += float(va[p])
    return A


def dense_products(A, dtype):
    """(x -> T(A x), y -> T(A^T y)) in fp64 (the CPU tests' products)"""
    A = np.asarray(A, dtype=np.float64)
    return (lambda x: (A @ _f64(x)).astype(dtype)), (lambda y: (A.T @ _f64(y)).astype(dtype))


def start_vector(n, dtype, seed=0):
    return np.random.default_rng(20261021 + 7 * seed + n).standard_normal(n).astype(dtype)


# What rounding adds to a returned triplet's figures beyond its returned estimate e_c, in units of u_T * sigma_max: the largest
# (figure - e_c) / (u_T sigma_max) over |sigma - sigma_ref|, ||A v - sigma u|| and ||A^T u - sigma v|| and over the cases of
# tests/test_svds_model_host.py; residual_allowance allows 4 times that.  Measured: fp64 15.7 (||A v - sigma u|| of the third triplet of the
# 171 x 300 band at nev = 3, 4.22e-15 against an estimate of 1.16e-16: that residual is pure rounding, which the estimate does not cover); fp32 1.50
# (the same residual on the 300 x 171 band at nev = 6, 2.51e-07).
RESIDUAL_K = {"float64": 15.7, "float32": 1.5}

def residual_allowance(dtype, sigma_max):
    return 4 * RESIDUAL_K[np.dtype(dtype).name] * float(np.finfo(dtype).eps) / 2 * sigma_max
