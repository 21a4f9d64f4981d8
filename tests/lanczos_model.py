"""The thick-restart Lanczos recurrence of cvr_eigsh_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the
eigensolver tests compare the device with, bit for bit.  The conventions are tests/krylov_model.py's: every stored vector is rounded to the handle's
type T once, scalars are fp64, a sum's terms are `double(a_i) * double(b_i)` added in the documented tree (krylov_model.tree_sum), and the matrix enters
through `product` (x -> T(A x)).  The projected problem is solved by the library's own cvr_sym_eig_host (capi.sym_eig_host), an ingredient exactly as
the product is: tests/test_lanczos_model_host.py holds it to LAPACK on its own.

One method per operation of the header, so that a mutant (tests/test_lanczos_model_host.py) is the model with one method replaced."""
import numpy as np

from cvr_amd import capi
from krylov_model import _f64, _Model

CONVERGED, MAX_RESTARTS, BREAKDOWN, INVARIANT = 0, 1, 2, 3          # CVR_EIG_* of include/cvr_amd.h
LARGEST, SMALLEST = 0, 1
EPS23 = 3.666852862501036e-11          # the header's literal


def default_ncv(n, nev):
    return min(n, max(2 * nev + 1, 20), 64)


class EigEntry:
    """what the device returns: evals (the count returned, ascending), evecs (n x count, column c the vector of evals[c]), and the result's fields"""

    def __init__(self, evals, evecs, nconv, status, restarts, spmv_count, max_estimate, **scalars):
        self.evals, self.evecs = np.asarray(evals, dtype=np.float64), evecs
        self.nconv, self.status, self.restarts, self.spmv_count = int(nconv), int(status), int(restarts), int(spmv_count)
        self.max_estimate = np.float64(max_estimate)
        self.scalars = scalars

    def __repr__(self):
        return (f"EigEntry(evals={self.evals!r}, nconv={self.nconv}, status={self.status}, restarts={self.restarts}, spmv_count={self.spmv_count}, "
                f"max_estimate={self.max_estimate!r})")


def compare(got, want, vectors=True):
    """the one comparison of a result with a model entry: evals bit for bit, evecs byte for byte, nconv, status, restarts, spmv_count equal,
    max_estimate equal as bits.  Returns "" when they agree, else what differs."""
    bad = []
    for name in ("nconv", "status", "restarts", "spmv_count"):
        if getattr(got, name) != getattr(want, name):
            bad.append(f"{name} = {getattr(got, name)}, model {getattr(want, name)}")
    if np.float64(got.max_estimate).tobytes() != np.float64(want.max_estimate).tobytes():
        bad.append(f"max_estimate = {got.max_estimate!r}, model {want.max_estimate!r}")
    ge, we = np.ascontiguousarray(got.evals, dtype=np.float64), np.ascontiguousarray(want.evals, dtype=np.float64)
    if ge.shape != we.shape or ge.tobytes() != we.tobytes():
        bad.append(f"evals = {ge!r}, model {we!r}")
    if vectors:
        gv, wv = np.ascontiguousarray(got.evecs), np.ascontiguousarray(want.evecs)
        if gv.dtype != wv.dtype or gv.shape != wv.shape:
            bad.append(f"evecs is {gv.dtype}{gv.shape}, model {wv.dtype}{wv.shape}")
        elif gv.tobytes() != wv.tobytes():
            d = np.argwhere((gv.view(np.uint8).reshape(gv.shape + (-1,)) != wv.view(np.uint8).reshape(wv.shape + (-1,))).any(axis=-1))
            i, c = (int(v) for v in d[0])
            bad.append(f"evecs differ in {len(d)} of {gv.size} values, first at row {i} of column {c}: {gv[i, c]!r}, model {wv[i, c]!r}")
    return "; ".join(bad)


class LanczosModel(_Model):
    """cvr_eigsh_device"""

    def __init__(self, product, dtype, sums="tree"):
        super().__init__(product, dtype, sums)

    # ---- the single operations of the header ----
    def coefficients(self, V, w):
        """c_i = v_i . w for every column, all on the same w"""
        return np.array([self.dot("v.w", v, w) for v in V])

    def subtract(self, V, c, w):
        """t = double(w); t = t - c_0 double(v_0); ...; w = T(t)"""
        t = _f64(w)
        for ci, v in zip(c, V):
            t = t - ci * _f64(v)
        return self.rnd(t)

    def alpha(self, h, d, j):
        """alpha_j = h_j + d_j"""
        return h[j] + d[j]

    def beta_sum(self, w_new, w_old):
        """ww: of the new w"""
        return self.dot("w.w", w_new, w_new)

    def closed(self, ww1, ww):
        """the space is closed: the second pass halved the norm once more (beta == 0 included)"""
        return bool(ww <= 0.25 * ww1)

    def normalise(self, w, by):
        return self.rnd(_f64(w) / by)

    def arrow(self, beta_m, S, sel):
        """s_c = beta_m * S[m-1, c] of the kept pairs"""
        return np.array([beta_m * S[-1, c] for c in sel])

    def projected(self, q, k, theta, arrow, alpha, beta):
        """the q x q matrix (its lower triangle): the kept values with their arrow in row k, the tridiagonal beyond"""
        P = np.zeros((q, q))
        for c in range(k):
            P[c, c] = theta[c]
            P[k, c] = arrow[c]
        for j in range(k, q):
            P[j, j] = alpha[j]
            if j + 1 < q:
                P[j + 1, j] = beta[j + 1]
        return P

    def small_eig(self, P):
        return capi.sym_eig_host(P)

    def select(self, which, q, count):
        """the `count` pairs at the wanted end, ascending"""
        return list(range(q - count, q)) if which == LARGEST else list(range(count))

    def estimate(self, beta_q, S, q, c):
        """e_c = |beta_q * S[q-1, c]|"""
        return abs(beta_q * S[q - 1, c])

    def keep(self, nev, nconv, m):
        """k = nev + min(nconv, (m - nev) / 2)"""
        return nev + min(nconv, (m - nev) // 2)

    def restart_sum(self, s, V):
        """u = +0; u = u + S[l, c] * double(v_l), l ascending; T(u)"""
        u = np.zeros(len(V[0]))
        for sl, v in zip(s, V):
            u = u + sl * _f64(v)
        return self.rnd(u)

    def carry(self, V, m):
        """the new v_k: the old v_m"""
        return V[m]

    # ---- the run ----
    def run(self, v0, nev=1, which=LARGEST, ncv=0, tol=1e-8, max_restarts=100):
        with np.errstate(all="ignore"):
            return self._run(np.ascontiguousarray(v0, dtype=self.T), int(nev), which, int(ncv), np.float64(tol), int(max_restarts))

    def _run(self, v0, nev, which, ncv, tol, max_restarts):
        n = len(v0)
        m = ncv if ncv else default_ncv(n, nev)
        assert nev >= 1 and nev + 2 <= m <= min(n, 64), (n, nev, m)
        none = np.zeros((n, 0), dtype=self.T)
        self.history = []          # history[r]: what the same call returns with max_restarts = r (the last entry: for every larger one, when it is final)
        s = self.dot("v0.v0", v0, v0)
        # (the steps are enqueued before the start's stop is known: the first cycle counts in any case)
        if not (s > 0 and np.isfinite(s)):
            return EigEntry([], none, 0, BREAKDOWN, 0, m, 0.0, s=s)
        V = [self.normalise(v0, np.sqrt(s))]
        k, restarts, spmvs = 0, 0, 0
        theta, arrow = np.zeros(0), np.zeros(0)
        while True:
            alpha, beta = np.zeros(m), np.zeros(m + 1)
            spmvs += m - k          # a whole cycle is enqueued, whatever ends it
            q, closed = m, False
            for j in range(k, m):
                w0 = self.product(V[j])
                h = self.coefficients(V, w0)
                w1 = self.subtract(V, h, w0)
                d = self.coefficients(V, w1)
                w = self.subtract(V, d, w1)
                alpha[j] = self.alpha(h, d, j)
                ww1, ww = self.dot("w.w", w1, w1), self.beta_sum(w, w1)
                beta[j + 1] = np.sqrt(ww)
                if not (np.isfinite(ww1) and np.isfinite(ww) and np.isfinite(alpha[j])):
                    return EigEntry([], none, 0, BREAKDOWN, restarts, spmvs, 0.0, ww=ww, alpha=alpha[j], j=j)
                if self.closed(ww1, ww):
                    q, closed = j + 1, True
                    break
                V.append(self.normalise(w, beta[j + 1]))
            th, S = self.small_eig(self.projected(q, k, theta, arrow, alpha, beta))
            want = min(nev, q)
            sel = self.select(which, q, want)
            bq = 0.0 if closed else beta[q]
            est = np.array([self.estimate(bq, S, q, c) for c in sel])
            scale = np.maximum(EPS23, np.abs(th[sel]))
            nconv = int(np.count_nonzero(est <= tol * scale))
            worst = float(np.max(est / scale))
            done = closed or nconv == nev
            # what the call returns when it ends here (for max_restarts = restarts, or for good)
            status = (CONVERGED if q >= nev else INVARIANT) if closed else CONVERGED if done else MAX_RESTARTS
            vecs = np.stack([self.restart_sum(S[:, c], V[:q]) for c in sel], axis=1)
            entry = EigEntry(th[sel], vecs, want if closed else nconv, status, restarts, spmvs, worst, theta=th, S=S, beta=beta, alpha=alpha, est=est, q=q)
            self.history.append(entry)
            if done or restarts == max_restarts:
                return entry
            kk = self.keep(nev, nconv, m)
            ksel = self.select(which, m, kk)
            theta, arrow = th[ksel], self.arrow(beta[m], S, ksel)
            V = [self.restart_sum(S[:, c], V[:m]) for c in ksel] + [self.carry(V, m)]
            k = kk
            restarts += 1


def eigsh_model(product, v0, nev=1, which=LARGEST, ncv=0, tol=1e-8, max_restarts=100, dtype=np.float64, sums="tree"):
    return LanczosModel(product, dtype, sums).run(v0, nev, which, ncv, tol, max_restarts)


# ---- the cases the CPU and the GPU tests share ----
def laplacian_1d(n, dtype):
    """(n, n, row_ptr, col_idx, vals) of tridiag(-1, 2, -1): the eigenvalues are 2 - 2 cos(k pi / (n + 1)), k = 1..n"""
    rp, ci, va = [0], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                ci.append(j)
                va.append(v)
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def laplacian_eigs(n):
    return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


def band_indefinite(n, dtype, half_band=2, seed=0):
    """a symmetric random band matrix with entries in [-1, 1): indefinite"""
    rng = np.random.default_rng(20261019 + seed + n)
    D = {}
    for i in range(n):
        for j in range(i, min(n, i + half_band + 1)):
            D[(i, j)] = D[(j, i)] = float(dtype(rng.random() * 2 - 1))
    rp, ci, va = [0], [], []
    for i in range(n):
        for j in range(max(0, i - half_band), min(n, i + half_band + 1)):
            ci.append(j)
            va.append(D[(i, j)])
        rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def diag96(dtype):
    """(n, row_ptr, col_idx, vals) of tests/golden/diag96.npz, the loader's arrays read literally: n = 97 with an empty first row"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diag96.npz"))
    return int(z["dims"][1]) + 1, z["csr_rowptr"].astype(np.int64), z["csr_col"].astype(np.int32), z["csr_val"].astype(dtype)


def residual_allowance(dtype, anorm1):
    """what rounding adds to a returned pair's true residual beyond the estimate: 4 * RESIDUAL_K * u_T * ||A||_1 (tests/test_lanczos_model_host.py
    measures RESIDUAL_K over its cases)"""
    return 4 * RESIDUAL_K[np.dtype(dtype).name] * float(np.finfo(dtype).eps) / 2 * anorm1


# the largest (||A v - theta v|| - tol max(eps23, |theta|)) / (u_T ||A||_1) over the cases of tests/test_lanczos_model_host.py: fp64: none above its
# estimate's bound (the nearest stays 646 u ||A||_1 below it); fp32: 1.72
RESIDUAL_K = {"float64": 0.0, "float32": 1.72}


def dense_of(n, rp, ci, va):
    A = np.zeros((n, n))
    for i in range(n):
        for p in range(rp[i], rp[i + 1]):
            A[i, ci[p]] += float(va[p])
    return A


def csr_product(n, rp, ci, va, dtype):
    """x -> T(A x) with every row's terms added in CSR order in fp64 (the CPU tests' product)"""
    A = dense_of(n, rp, ci, va)

    def product(x):
        return (A @ _f64(x)).astype(dtype)
    return product


def start_vector(n, dtype, seed=0):
    return np.random.default_rng(20261019 + 7 * seed + n).standard_normal(n).astype(dtype)
