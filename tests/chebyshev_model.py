"""The Chebyshev polynomial preconditioner (cvr_precond_chebyshev), cvr_pcg_device with it and cvr_chebyshev_bounds in numpy, written from the text of
include/cvr_amd.h (not from the kernels), beside krylov_model.py, whose sums, trajectories and comparison it uses, and power_model.py, whose loop the
bounds run.

What the header fixes and this file does: the scalars are fp64 and computed once (`Cheb.coefficients`: theta, delta, sigma, rho_k, a[k], b[k], every
operation rounded on its own); every stored vector is rounded to the handle's type T once -- step 0 is `d = T(c0 * double(r))`, `z = d`, step k >= 1 is
`q = A z`, `d = T(a[k] * double(d) + b[k] * (double(r) - double(q)))`, `z = T(double(z) + double(d))` (numpy's ufuncs never fuse).  The matrix enters
through `product`, a callback x -> T(A x): on the GPU the handle's own cvr_spmv_device, on the CPU the CSR loop rounded to T.

`Cheb` is a class whose methods are the single operations of the header, so that a mutant (tests/test_chebyshev_model_host.py) is the model with one
method replaced.  `ChebPcg` is cvr_cg_device's model whose z is that apply."""
import numpy as np

import krylov_model as KM
import power_model as PW

MAX_DEGREE = 16          # CVR_CHEBYSHEV_MAX_DEGREE
LMAX_FACTOR = 1.1        # CVR_CHEBYSHEV_LMAX_FACTOR


def _f64(a):
    return np.asarray(a).astype(np.float64)


class Cheb:
    """z = p_degree(A) r for bounds lmin < lmax, in T"""

    def __init__(self, degree, lmin, lmax, dtype):
        assert 1 <= degree <= MAX_DEGREE and 0 < lmin < lmax
        self.degree, self.lmin, self.lmax, self.T = int(degree), np.float64(lmin), np.float64(lmax), np.dtype(dtype).type
        self.a, self.b = self.coefficients()

    # ---- the single operations of the header ----
    def next_rho(self, sigma, rho):
        return np.float64(1.0) / (np.float64(2.0) * sigma - rho)

    def carry(self, rho_old, rho_new):
        """rho_(k-1) of the next k"""
        return rho_new

    def pair(self, rho_new, rho_old, delta):
        """(a[k], b[k])"""
        return rho_new * rho_old, np.float64(2.0) * rho_new / delta

    def coefficients(self):
        theta = (self.lmax + self.lmin) / np.float64(2.0)
        delta = (self.lmax - self.lmin) / np.float64(2.0)
        sigma = theta / delta
        rho = np.float64(1.0) / sigma
        a, b = np.zeros(self.degree), np.zeros(self.degree)
        a[0], b[0] = 0.0, np.float64(1.0) / theta
        for k in range(1, self.degree):
            new = self.next_rho(sigma, rho)
            a[k], b[k] = self.pair(new, rho, delta)
            rho = self.carry(rho, new)
        return a, b

    def rnd(self, v):
        return np.asarray(v).astype(self.T)

    def first(self, r):
        """d of step 0"""
        return self.rnd(self.b[0] * _f64(r))

    def residual(self, r, q):
        return _f64(r) - _f64(q)

    def direction(self, k, d, r, q):
        return self.rnd(self.a[k] * _f64(d) + self.b[k] * self.residual(r, q))

    def accumulate(self, z, d):
        return self.rnd(_f64(z) + _f64(d))

    def apply(self, product, r):
        r = np.ascontiguousarray(r, dtype=self.T)
        with np.errstate(all="ignore"):
            d = self.first(r)
            z = d.copy()
            for k in range(1, self.degree):
                q = product(z)
                d = self.direction(k, d, r, q)
                z = self.accumulate(z, d)
        return z


def apply(product, r, degree, lmin, lmax, dtype):
    return Cheb(degree, lmin, lmax, dtype).apply(product, r)


class ChebPcg(KM.CgModel):
    """cvr_pcg_device with a Chebyshev object: cvr_cg_device's recurrence with z = p_d(A) r.  `cheb`: a Cheb (or a mutant of it); `inner`: the product of
    the object's handle where it is not the solve's."""

    def __init__(self, product, dtype, cheb, sums="tree", inner=None):
        super().__init__(product, dtype, sums)
        self.cheb, self.inner = cheb, inner or product

    def scale(self, minv, r):
        """z: the apply in place of T(minv * r)"""
        return self.cheb.apply(self.inner, r)

    def start(self, b, x0, minv):
        b, x, _, r = super().start(b, x0, None)
        return b, x, self, r          # (a preconditioner is present: r.z is a sum of its own)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


# ---- cvr_chebyshev_bounds ----
def start_vector(n, dtype):
    """x_i = T(1 + double(uint32(i * 2654435761)) * 2^-32)"""
    u = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (1.0 + u.astype(np.float64) * 2.0 ** -32).astype(dtype)


def bounds(product, n, dtype, power_iters=20, eig_ratio=30.0, power_model=None):
    """(lmin, lmax, lambda): cvr_power_iteration's model from the start vector (`power_model`: the handle's PowerModel where its sums are not the dense
    tree's), lmax = 1.1 * lambda, lmin = lmax / eig_ratio"""
    m = power_model or PW.PowerModel(product, dtype)
    lam = m.run(start_vector(n, dtype), power_iters).lam
    lmax = np.float64(LMAX_FACTOR) * lam
    return lmax / np.float64(eig_ratio), lmax, lam


# ---- the closed form ----
def closed_form(A, r, degree, lmin, lmax):
    """p(A) r in fp64 through A's eigenvectors: the residual polynomial of `degree` Chebyshev steps from z = 0 is
    T_degree((theta - lambda) / delta) / T_degree(sigma), so p(lambda) = (1 - that) / lambda"""
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    lam, Q = np.linalg.eigh(A)
    c = np.zeros(degree + 1)
    c[degree] = 1.0
    T = np.polynomial.chebyshev.chebval
    p = (1.0 - T((theta - lam) / delta, c) / T(theta / delta, c)) / lam
    return Q @ (p * (Q.T @ r))


def closed_form_bound(n, degree, lmin, lmax, rnorm):
    """||model - closed form||_2 <= this, in fp64 (eps = 2^-53 per operation), for a spectrum inside [lmin, lmax].  Every iterate is z_k = p_k(A) r
    with |p_k| <= 2 / lmin on the spectrum, so ||z_k|| <= 2 R, ||d_k|| = ||z_k - z_(k-1)|| <= 4 R with R = ||r|| / lmin; |a[k]| < 1 (rho < 1) and
    |b[k]| < 2 / delta; ||A|| <= lmax.  A step rounds d with at most (n + 4) eps relative to |a| |d| + |b| (|r| + |A| |z|) (a row of q = A z is a sum
    of n terms) and z with eps relative to |z| + |d|: a local error of at most
        e = eps * ((n + 4) * (4 R + (2 / delta) * (||r|| + 2 lmax R)) + 6 R).
    An error put into z at one step is carried on by the homogeneous recurrence, whose solutions are Chebyshev polynomials of the second kind over
    those of the first at sigma: bounded by degree + 1 on the spectrum.  `degree` steps: degree * (degree + 1) * e."""
    eps = 2.0 ** -53
    delta = (lmax - lmin) / 2
    R = rnorm / lmin
    e = eps * ((n + 4) * (4 * R + (2 / delta) * (rnorm + 2 * lmax * R)) + 6 * R)
    return degree * (degree + 1) * e
