"""The recurrence of cvr_lsqr_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the LSQR tests compare
the device with, value by value.  The conventions are tests/krylov_model.py's: every stored vector rounded to T once, every scalar fp64, every sum the
documented tree (`krylov_model.tree_sum`) over double(a_i) * double(b_i), a Trajectory whose steps[k] is what the device must return for
max_iters = k, and `compare` as the one comparison (here with cvr_lsqr_info beside it: `compare` below).

The matrix enters through two callbacks, `product` x -> T(A x) on n values and `product_t` y -> T(A^T y) on m values: on the GPU the two handles' own
cvr_spmv_device, on the CPU the oracle's CSR loop rounded to T.

The model is a class whose methods are the single operations of the header, so that a mutant (tests/test_lsqr_model_host.py) is the model with one
method replaced."""
import numpy as np

import krylov_model as KM
from krylov_model import BREAKDOWN, CONVERGED, MAX_ITERS, _f64


class Info:
    """cvr_lsqr_info in the model's terms"""

    def __init__(self, arnorm, anorm, stop_test):
        self.arnorm, self.anorm, self.stop_test = np.float64(arnorm), np.float64(anorm), int(stop_test)

    def __repr__(self):
        return f"Info(arnorm={self.arnorm!r}, anorm={self.anorm!r}, stop_test={self.stop_test})"


def compare(got, got_info, step):
    """krylov_model.compare, and cvr_lsqr_info against the entry's: arnorm and anorm equal as bits, stop_test equal.  "" when they agree."""
    bad = [KM.compare(got, step)] if KM.compare(got, step) else []
    want = step.scalars["info"]
    if got_info.stop_test != want.stop_test:
        bad.append(f"stop_test = {got_info.stop_test}, model {want.stop_test}")
    for name in ("arnorm", "anorm"):
        g, m = getattr(got_info, name), getattr(want, name)
        if KM._bits(g) != KM._bits(m):
            bad.append(f"{name} = {g!r}, model {m!r}")
    return "; ".join(bad)


def _finite(*v):
    return all(np.isfinite(a) for a in v)


class LsqrModel:
    """cvr_lsqr_device"""

    def __init__(self, product, product_t, dtype, sums="tree"):
        assert sums in ("tree", "exact"), sums
        self.product, self.product_t, self.T, self.sums, self.pack = product, product_t, np.dtype(dtype).type, sums, KM.pack_of(dtype)

    # ---- the single operations of the header ----
    def dot(self, name, a, b):
        t = _f64(a) * _f64(b)
        return KM.tree_sum(t, self.pack) if self.sums == "tree" else KM.exact_sum(t)

    def norm(self, name, a):
        """sqrt of the sum called `name` ("b.b", "u.u", "v.v")"""
        return np.sqrt(self.dot(name, a, a))

    def rnd(self, v):
        return np.asarray(v).astype(self.T)

    def start_u(self, b, x):
        """u^ = b - A x0: what the scaled product with alpha = -1, beta = 1 stores"""
        return self.rnd(_f64(b) - _f64(self.product(x)))

    def first_v(self, p, beta):
        return self.rnd(_f64(p) / beta)

    def next_u(self, q, u, alpha, beta):
        """u^ = T(double(q) - (alpha / beta) * double(u^)): u stays unnormalised"""
        return self.rnd(_f64(q) - (alpha / beta) * _f64(u))

    def next_v(self, p, v, beta):
        return self.rnd(_f64(p) / beta - beta * _f64(v))

    def normalise(self, vh, alpha):
        return self.rnd(_f64(vh) / alpha)

    def anorm2(self, anorm2, alpha, beta, damp):
        return anorm2 + ((alpha * alpha + beta * beta) + damp * damp)

    def damp_rotation(self, rhobar, phibar, damp):
        """(rhobar1, psi, phibar)"""
        if damp > 0:
            rhobar1 = np.sqrt(rhobar * rhobar + damp * damp)
            return rhobar1, (damp / rhobar1) * phibar, (rhobar / rhobar1) * phibar
        return rhobar, np.float64(0.0), phibar

    def rotation(self, rhobar1, beta, alpha, phibar):
        """(rho, theta, rhobar, phi, phibar, s)"""
        rho = np.sqrt(rhobar1 * rhobar1 + beta * beta)
        c, s = rhobar1 / rho, beta / rho
        return rho, s * alpha, self.new_rhobar(c, alpha), c * phibar, s * phibar, s

    def new_rhobar(self, c, alpha):
        return -c * alpha

    def update_x(self, x, t1, w):
        return self.rnd(_f64(x) + t1 * _f64(w))

    def update_w(self, v, t2, w):
        return self.rnd(_f64(v) - t2 * _f64(w))

    def arnorm(self, alpha, s, phi):
        return alpha * np.abs(s * phi)

    def test1(self, rnorm, rtol, bnorm):
        return bool(rnorm <= np.float64(rtol) * bnorm)

    def test2(self, arnorm, rtol, anorm, rnorm):
        return bool(arnorm <= (np.float64(rtol) * anorm) * rnorm)

    def run(self, b, x0=None, damp=0.0, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, np.float64(damp), rtol, max_iters)

    def _run(self, b, x0, damp, rtol, max_iters):
        tr = KM.Trajectory()
        b = np.ascontiguousarray(b, dtype=self.T)
        probe = self.product_t(np.zeros(len(b), dtype=self.T))
        n = len(probe)
        x = np.zeros(n, dtype=self.T) if x0 is None else np.array(x0, dtype=self.T)
        u = self.start_u(b, x)
        bb = self.dot("b.b", b, b)
        bnorm, beta = np.sqrt(bb), self.norm("u.u", u)
        if bb == 0:
            return tr.add(np.zeros(n, dtype=self.T), 0, CONVERGED, 0.0, bnorm, terminal=True, info=Info(0.0, 0.0, 0))
        if not _finite(beta):
            return tr.add(x, 0, BREAKDOWN, beta, bnorm, terminal=True, info=Info(0.0, 0.0, 0))
        if self.test1(beta, rtol, bnorm):
            return tr.add(x, 0, CONVERGED, beta, bnorm, terminal=True, info=Info(0.0, 0.0, 1))
        vh = self.first_v(self.product_t(u), beta)
        alpha = self.norm("v.v", vh)
        if not _finite(alpha):
            return tr.add(x, 0, BREAKDOWN, beta, bnorm, terminal=True, info=Info(alpha * beta, 0.0, 0))
        if alpha == 0:
            return tr.add(x, 0, CONVERGED, beta, bnorm, terminal=True, info=Info(alpha * beta, 0.0, 2))
        v = self.normalise(vh, alpha)
        w = v.copy()
        rhobar, phibar, anorm2, psi2, rnorm = alpha, beta, np.float64(0.0), np.float64(0.0), beta
        info = Info(alpha * beta, 0.0, 0)
        tr.add(x, 0, MAX_ITERS, rnorm, bnorm, info=info, alpha=alpha, beta=beta)
        for k in range(max_iters):
            u = self.next_u(self.product(v), u, alpha, beta)
            beta1 = self.norm("u.u", u)
            alpha1 = np.float64(0.0)
            if beta1 != 0 and _finite(beta1):
                vh = self.next_v(self.product_t(u), v, beta1)
                alpha1 = self.norm("v.v", vh)
            anorm2 = self.anorm2(anorm2, alpha, beta1, damp)
            rhobar1, psi, phibar1 = self.damp_rotation(rhobar, phibar, damp)
            rho, theta, rhobar_n, phi, phibar_n, s = self.rotation(rhobar1, beta1, alpha1, phibar1)
            t1, t2 = phi / rho, theta / rho
            if not _finite(beta1, alpha1, rho, t1) or rho == 0:          # found before x is touched: everything stays at the last iterate's
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, info=info)
            x = self.update_x(x, t1, w)
            psi2 = psi2 + psi * psi
            rnorm, arnorm, anorm = np.sqrt(phibar_n * phibar_n + psi2), self.arnorm(alpha1, s, phi), np.sqrt(anorm2)
            test = 0
            if _finite(rnorm, arnorm, anorm):
                test = 1 if self.test1(rnorm, rtol, bnorm) else 2 if self.test2(arnorm, rtol, anorm, rnorm) else 0
            info = Info(arnorm, anorm, test)
            sc = dict(info=info, alpha=alpha1, beta=beta1, rho=rho, phi=phi, theta=theta)
            if test:
                return tr.add(x, k + 1, CONVERGED, rnorm, bnorm, terminal=True, **sc)
            v = self.normalise(vh, alpha1)
            w = self.update_w(v, t2, w)
            alpha, beta, rhobar, phibar = alpha1, beta1, rhobar_n, phibar_n
            tr.add(x, k + 1, MAX_ITERS, rnorm, bnorm, **sc)
        return tr


def lsqr_model(product, product_t, b, x0=None, damp=0.0, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return LsqrModel(product, product_t, dtype, sums).run(b, x0, damp, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def transpose_csr(m, n, rp, ci, va):
    """(n, m, row_ptr, col_idx, vals) of A^T, columns of a row ascending"""
    rows = np.repeat(np.arange(m), np.diff(rp))
    order = np.lexsort((rows, ci))
    rpt = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rpt, np.asarray(ci, dtype=np.int64) + 1, 1)
    return n, m, np.cumsum(rpt), rows[order].astype(np.int32), np.asarray(va)[order]


def rect_sparse(m, n, dtype, seed=0, per_row=3):
    """(m, n, row_ptr, col_idx, vals): a diagonal-like entry (row i: column i * n // m when m >= n, else column i; value in [1, 2)) plus up to
    `per_row` random entries in [-0.5, 0.5) per row, sorted columns without duplicates: full rank min(m, n), moderately conditioned"""
    rng = np.random.default_rng(20261019 + seed + 1000 * m + n)
    rp, ci, va = [0], [], []
    for i in range(m):
        d = i * n // m if m >= n else i
        cols = {int(c): float(rng.random() - 0.5) for c in rng.integers(0, n, per_row)}
        cols[d] = 1.0 + float(rng.random())
        for c in sorted(cols):
            ci.append(c)
            va.append(cols[c])
        rp.append(len(ci))
    return m, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def rect_long(dtype, m=701, n=449, long_rows=(348, 349, 350, 351), long_cols=(221, 222, 223), seed=0):
    """(m, n, row_ptr, col_idx, vals): rect_sparse(m, n) plus four neighbouring rows of 300 and three neighbouring columns of 400 further entries of size
    <= 0.02 (sorted columns, no duplicates).  Each is longer than a quarter of a chunk of 16 steps (256 of 1024 slots) and the neighbours together
    are longer than a chunk, so the plain layout of A and of A^T cuts at least one of them over chunks; the added part has a Frobenius norm of
    about 1 beside singular values of A in about [1, 2.5]: still well conditioned (tests/test_lsqr_model_host.py)"""
    _, _, rp, ci, va = rect_sparse(m, n, np.float64)
    rng = np.random.default_rng(20261020 + seed)
    rows = [dict(zip(ci[rp[i]:rp[i + 1]].tolist(), va[rp[i]:rp[i + 1]].tolist())) for i in range(m)]
    for r in long_rows:
        for c in rng.choice(n, size=300, replace=False):
            rows[r].setdefault(int(c), float(rng.random() * 0.04 - 0.02))
    for c in long_cols:
        for r in rng.choice(m, size=400, replace=False):
            rows[int(r)].setdefault(int(c), float(rng.random() * 0.04 - 0.02))
    rp2 = np.zeros(m + 1, dtype=np.int64)
    rp2[1:] = np.cumsum([len(r) for r in rows])
    ci2 = np.array([c for r in rows for c in sorted(r)], dtype=np.int32)
    va2 = np.array([r[c] for r in rows for c in sorted(r)], dtype=dtype)
    return m, n, rp2, ci2, va2


def two_per_row(m, n, dtype):
    """(m, n, row_ptr, col_idx, vals) for m >= n: row i holds its diagonal-like entry at column i % n (value 1 + (i % 7) / 8) and its neighbour
    (i + 1) % n (value -0.25); with n == 1 the diagonal-like entry alone"""
    i = np.arange(m, dtype=np.int64)
    if n == 1:
        return m, n, np.arange(m + 1, dtype=np.int64), np.zeros(m, dtype=np.int32), (1 + (i % 7) / 8).astype(dtype)
    c0, c1 = i % n, (i + 1) % n
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    ci = np.stack([lo, hi], axis=1).reshape(-1).astype(np.int32)
    d, o = 1 + (i % 7) / 8, np.full(m, -0.25)
    va = np.stack([np.where(lo == c0, d, o), np.where(lo == c0, o, d)], axis=1).reshape(-1).astype(dtype)
    return m, n, np.arange(0, 2 * m + 1, 2, dtype=np.int64), ci, va


def dense_of(m, n, rp, ci, va):
    A = np.zeros((m, n))
    A[np.repeat(np.arange(m), np.diff(rp)), ci] = va
    return A


def inputs(m, n, rp, ci, va, dtype, consistent, seed=0):
    """(b, a random start vector in [-1, 1)): b = A x* rounded to T for a random x* (consistent; fp rounding of b aside) or that plus a random
    vector of the same size (inconsistent)"""
    rng = np.random.default_rng(20261019 + seed + 7 * m + n)
    xs = rng.standard_normal(n)
    b = dense_of(m, n, rp, ci, va) @ xs if m * n <= 1 << 22 else None
    if b is None:
        b = np.zeros(m)
        np.add.at(b, np.repeat(np.arange(m), np.diff(rp)), _f64(va) * xs[ci])
    if not consistent:
        b = b + rng.standard_normal(m) * max(1.0, float(np.abs(b).mean()))
    return b.astype(dtype), (rng.random(n) * 2 - 1).astype(dtype)
