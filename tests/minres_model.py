"""The recurrence of cvr_minres_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the MINRES tests compare
the device with, value by value.  The conventions are tests/krylov_model.py's: every stored vector rounded to T once, every scalar fp64, every sum the
documented tree (`krylov_model.tree_sum`) over double(a_i) * double(b_i), a Trajectory whose steps[k] is what the device must return for
max_iters = k, and `compare` as the one comparison (here with cvr_minres_info beside it: `compare` below).

The matrix enters through `product`, a callback x -> T(A x) on arrays of n values: on the GPU the handle's own cvr_spmv_device, on the CPU the oracle's
CSR loop rounded to T.  The shift is the model's own arithmetic.

The model is krylov_model._Model with the single operations of the header as methods, so that a mutant (tests/test_minres_model_host.py) is the model
with one method replaced."""
import numpy as np

import krylov_model as KM
from krylov_model import BREAKDOWN, CONVERGED, MAX_ITERS, _f64

DBL_MAX = np.finfo(np.float64).max


class Info:
    """cvr_minres_info in the model's terms"""

    def __init__(self, anorm, acond):
        self.anorm, self.acond = np.float64(anorm), np.float64(acond)

    def __repr__(self):
        return f"Info(anorm={self.anorm!r}, acond={self.acond!r})"


def compare(got, got_info, step):
    """krylov_model.compare, and cvr_minres_info against the entry's: anorm and acond equal as bits.  "" when they agree."""
    bad = [KM.compare(got, step)] if KM.compare(got, step) else []
    want = step.scalars["info"]
    for name in ("anorm", "acond"):
        g, m = getattr(got_info, name), getattr(want, name)
        if KM._bits(g) != KM._bits(m):
            bad.append(f"{name} = {g!r}, model {m!r}")
    return "; ".join(bad)


class MinresModel(KM._Model):
    """cvr_minres_device"""

    # ---- the single operations of the header ----
    def b_norm(self, b, m):
        """the norm the residual is measured in: sqrt(b . T(minv b)); sqrt(b . b) without a preconditioner"""
        return np.sqrt(self.dot("b.b", b, b) if m is None else self.dot("b.Mb", b, self.scale(m, b)))

    def beta_of(self, r2, z):
        """r2 . z: its root is beta"""
        return self.dot("r.z", r2, z)

    def first_cs(self):
        return np.float64(-1.0)

    def start_r(self, r, x, shift):
        """the scaled product's r = b - A x0 made the residual of A - shift I: T(double(r) + shift * double(x0)); r itself when shift == 0"""
        return r if shift == 0 else self.rnd(_f64(r) + shift * _f64(x))

    def y_prime(self, q, v, r1, shift, beta, oldb, k):
        t = _f64(q)
        if shift != 0:
            t = t - shift * _f64(v)
        if k > 0:
            t = t - (beta / oldb) * _f64(r1)
        return self.rnd(t)

    def next_r(self, yp, alfa, beta, r2):
        return self.rnd(_f64(yp) - (alfa / beta) * _f64(r2))

    def rotate_r(self, r1, r2, y):
        """(r1, r2) after the step"""
        return r2, y

    def tnorm2(self, tnorm2, alfa, oldb, betan):
        return tnorm2 + ((alfa * alfa + oldb * oldb) + betan * betan)

    def rotation_in(self, cs, sn, dbar, epsln, alfa, betan):
        """(oldeps, delta, gbar, epsln, dbar)"""
        return epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa, sn * betan, -cs * betan

    def rotation_out(self, gbar, betan, phibar):
        """(gamma, cs, sn, phi, phibar)"""
        gamma = np.sqrt(gbar * gbar + betan * betan)
        cs, sn = self.new_cs(gbar, gamma), betan / gamma
        return gamma, cs, sn, cs * phibar, sn * phibar

    def new_cs(self, gbar, gamma):
        return gbar / gamma

    def new_w(self, v, oldeps, w1, delta, w2, gamma):
        return self.rnd(((_f64(v) - oldeps * _f64(w1)) - delta * _f64(w2)) / gamma)

    def update_x(self, x, phi, w):
        return self.rnd(_f64(x) + phi * _f64(w))

    def next_v(self, z, betan):
        return self.rnd(_f64(z) / betan)

    def stop_norm(self, bnorm, b):
        """what rnorm is compared with, times rtol"""
        return bnorm

    def run(self, b, x0=None, minv=None, shift=0.0, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, minv, np.float64(shift), rtol, max_iters)

    def _run(self, b, x0, minv, shift, rtol, max_iters):
        tr = KM.Trajectory()
        b, x, m, r2 = self.start(b, x0, minv)
        r2 = self.start_r(r2, x, shift)
        z = self.scale(m, r2)
        bb, bnorm, rz = self.dot("b.b", b, b), self.b_norm(b, m), self.beta_of(r2, z)
        beta = np.sqrt(rz)
        none = Info(0.0, 0.0)
        if bb == 0:
            return tr.add(np.zeros(len(b), dtype=self.T), 0, CONVERGED, 0.0, bnorm, terminal=True, info=none)
        if not (rz >= 0 and np.isfinite(rz)):
            return tr.add(x, 0, BREAKDOWN, beta, bnorm, terminal=True, info=none)
        if beta <= np.float64(rtol) * self.stop_norm(bnorm, b):
            return tr.add(x, 0, CONVERGED, beta, bnorm, terminal=True, info=none)
        v = self.next_v(z, beta)
        r1 = None
        w1 = w2 = np.zeros(len(b), dtype=self.T)
        zero = np.float64(0.0)
        oldb, dbar, epsln, phibar, cs, sn, tnorm2, gmax, gmin, rnorm = zero, zero, zero, beta, self.first_cs(), zero, zero, zero, np.float64(DBL_MAX), beta
        info = none
        tr.add(x, 0, MAX_ITERS, rnorm, bnorm, info=info, beta=beta)
        for k in range(max_iters):
            q = self.product(v)
            yp = self.y_prime(q, v, r1, shift, beta, oldb, k)
            alfa = self.dot("v.y", v, yp)
            y = self.next_r(yp, alfa, beta, r2)
            r1, r2 = self.rotate_r(r1, r2, y)
            z = self.scale(m, r2)
            rz = self.beta_of(r2, z)
            betan = np.sqrt(rz)
            tnorm2_n = self.tnorm2(tnorm2, alfa, oldb, betan)
            oldeps, delta, gbar, epsln_n, dbar_n = self.rotation_in(cs, sn, dbar, epsln, alfa, betan)
            gamma, cs_n, sn_n, phi, phibar_n = self.rotation_out(gbar, betan, phibar)
            if not (np.isfinite(alfa) and rz >= 0 and np.isfinite(rz) and KM._usable(gamma) and np.isfinite(phi / gamma)):
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, info=info)          # found before x is touched
            w = self.new_w(v, oldeps, w1, delta, w2, gamma)
            x = self.update_x(x, phi, w)
            w1, w2 = w2, w
            gmax, gmin = np.maximum(gmax, gamma), np.minimum(gmin, gamma)
            tnorm2, epsln, dbar, cs, sn, phibar = tnorm2_n, epsln_n, dbar_n, cs_n, sn_n, phibar_n
            rnorm = phibar
            info = Info(np.sqrt(tnorm2), gmax / gmin)
            sc = dict(info=info, alfa=alfa, beta=betan, gamma=gamma, phi=phi, delta=delta, oldeps=oldeps)
            if np.isfinite(rnorm) and rnorm <= np.float64(rtol) * self.stop_norm(bnorm, b):
                return tr.add(x, k + 1, CONVERGED, rnorm, bnorm, terminal=True, **sc)
            v = self.next_v(z, betan)
            oldb, beta = beta, betan
            tr.add(x, k + 1, MAX_ITERS, rnorm, bnorm, **sc)
        return tr


def minres_model(product, b, x0=None, minv=None, shift=0.0, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return MinresModel(product, dtype, sums).run(b, x0, minv, shift, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def kkt(n1, n2, dtype):
    """(n, n, row_ptr, col_idx, vals) of [[K, B^T], [B, 0]], n = n1 + n2: K = krylov_model.banded("spd", n1) (spectrum in [0.5, 1.5]), B of n2 <= n1 / 2
    rows with B[i, 2i] = 1 and B[i, 2i + 1] = 0.5 (orthogonal rows of norm sqrt(1.25)).  By Rusten and Winther (SIAM J. Matrix Anal. Appl. 13, 1992)
    the spectrum lies in [-0.90, -0.59] u [0.5, 2.10]: truly indefinite and well conditioned."""
    assert 2 * n2 <= n1, (n1, n2)
    _, _, rp, ci, va = KM.banded("spd", n1, dtype)
    rows = []
    for i in range(n1):
        cols = {int(c): va[j] for j, c in zip(range(rp[i], rp[i + 1]), ci[rp[i]:rp[i + 1]])}
        if i < 2 * n2:
            cols[n1 + i // 2] = 1.0 if i % 2 == 0 else 0.5
        rows.append(cols)
    for i in range(n2):
        rows.append({2 * i: 1.0, 2 * i + 1: 0.5})
    n = n1 + n2
    rpn = np.zeros(n + 1, dtype=np.int64)
    cin, van = [], []
    for i, cols in enumerate(rows):
        for c in sorted(cols):
            cin.append(c)
            van.append(cols[c])
        rpn[i + 1] = len(cin)
    return n, n, rpn, np.array(cin, dtype=np.int32), np.array(van, dtype=dtype)


def banded_indefinite(n, dtype):
    """(n, n, row_ptr, col_idx, vals): krylov_model.banded("spd", n) with 2 taken from the diagonal of every odd row.  That matrix is I + E with
    ||E||_2 <= 0.5 (its spectrum lies in [0.5, 1.5]), this one J + E with J = diag(1, -1, 1, ...): symmetric, its spectrum inside
    [-1.5, -0.5] and [0.5, 1.5] (Weyl), about half of it on either side"""
    n, _, rp, ci, va = KM.banded("spd", n, np.float64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    va = va.copy()
    va[(rows == ci) & (rows % 2 == 1)] -= 2.0
    return n, n, rp, ci, va.astype(dtype)


def dense_of(n, rp, ci, va):
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    return A


def singular_kkt(n1, n2, dtype):
    """(n, row_ptr, col_idx, vals, b): kkt(n1, n2) with one empty row and column appended (n = n1 + n2 + 1, rank n - 1) and a b that is zero there:
    a singular consistent system"""
    n, _, rp, ci, va = kkt(n1, n2, dtype)
    b, _, _ = KM.inputs(n, dtype)
    return n + 1, np.concatenate([rp, rp[-1:]]), ci, va, np.concatenate([b, np.zeros(1, dtype=dtype)])


def shifted_inputs(n, dtype):
    """krylov_model.inputs for banded("spd", n) - 2 I; at n = 1 with b = 2, where (alfa / beta) * r2 is exact and step 0 ends with beta' == 0"""
    b, x0, minv = KM.inputs(n, dtype)
    if n == 1:
        b = np.array([2.0], dtype=dtype)
    return b, x0, minv


# The steps the model takes on the CPU to rtol = 1e-10 (fp64) / 1e-5 (fp32) on kkt(n1, n2) with krylov_model.inputs, the larger of the zero and the
# random start, by (n1, n2, precision, minv): seen with the tree sums and pinned as upper limits (tests/test_minres_model_host.py).
KKT_STEPS = {(40, 20, "fp64", False): 38, (40, 20, "fp64", True): 62, (200, 100, "fp64", False): 38, (200, 100, "fp64", True): 100,
             (40, 20, "fp32", False): 20, (40, 20, "fp32", True): 42, (200, 100, "fp32", False): 20, (200, 100, "fp32", True): 55}

# | residual_norm - ||b - (A - shift I) x||_M^-1 | <= GAP * eps(T) * (||A - shift I||_2 ||x||_2 + ||b||_2) at every entry of a trajectory.  The Lanczos
# vectors lose orthogonality in finite precision, so no bound is derived: the largest ratio seen with exact sums over the cases of
# tests/test_minres_model_host.py is 0.872 (kkt(200, 100), fp64, with minv, from the zero start); 4 times that is allowed.
GAP = 4 * 0.872


def residual_gap(dtype, a_norm2, x, b):
    return GAP * float(np.finfo(dtype).eps) * (a_norm2 * float(np.linalg.norm(_f64(x))) + float(np.linalg.norm(_f64(b))))
