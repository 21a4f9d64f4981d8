"""The numpy model of the Chebyshev polynomial preconditioner (tests/chebyshev_model.py) on the CPU: that its coefficient recurrence is the polynomial
it claims to be, that it does what it is for on the 5-point Laplacian with the estimated bounds, that degree 1 is cvr_cg_device's model with a constant
diagonal, and that the trajectory comparison the GPU tests use rejects the classical mistakes of the recurrence within 3 steps."""
import numpy as np
import pytest

import chebyshev_model as CM
import krylov_model as KM
import precond_model as PM
from cvr_amd import synth


def _dense_spd(n=12, lo=1.0, hi=10.0, seed=3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.linspace(lo, hi, n)
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 8, 16])
def test_recurrence_is_the_closed_form(degree):
    """dense 12 x 12 SPD, spectrum in [1, 10], bounds = the extreme eigenvalues widened by 1 %: the model in fp64 against p(A) r through the
    eigenvectors, within closed_form_bound (the recurrence's rounding) plus the same for the eigen-decomposition's side (n eps ||A|| on lambda and Q:
    covered by doubling)"""
    n = 12
    A = _dense_spd(n)
    ev = np.linalg.eigvalsh(A)
    lmin, lmax = ev[0] * 0.99, ev[-1] * 1.01
    r = np.random.default_rng(degree).standard_normal(n)
    z = CM.apply(lambda x: A @ np.asarray(x, dtype=np.float64), r, degree, lmin, lmax, np.float64)
    ref = CM.closed_form(A, r, degree, lmin, lmax)
    err, bound = np.linalg.norm(z - ref), 2 * CM.closed_form_bound(n, degree, lmin, lmax, np.linalg.norm(r))
    print(f"degree {degree}: |model - closed form| = {err:.3g}, bound {bound:.3g}, |z| = {np.linalg.norm(z):.3g}")
    assert err <= bound
    assert bound <= 1e-9 * np.linalg.norm(ref)          # (the bound is a rounding bound: a wrong coefficient is off by a factor, not by 1e-9)


def test_coefficients():
    c = CM.Cheb(3, 1.0, 3.0, np.float64)          # theta = 2, delta = 1, sigma = 2, rho_0 = 1/2, rho_1 = 1 / (4 - 1/2) = 2/7, rho_2 = 1 / (4 - 2/7) = 7/26
    assert c.a[0] == 0 and c.b[0] == 0.5
    assert c.a[1] == np.float64(1.0) / np.float64(3.5) * 0.5 and c.b[1] == 2 * (np.float64(1.0) / np.float64(3.5)) / 1.0
    r1 = np.float64(1.0) / np.float64(3.5)
    r2 = np.float64(1.0) / (np.float64(4.0) - r1)
    assert c.a[2] == r2 * r1 and c.b[2] == 2 * r2
    assert abs(r2 - 7 / 26) < 1e-16


def _laplacian(m, dtype=np.float64):
    n, _, rp, ci, va = synth.laplacian_2d(m, dtype)
    return n, rp, ci, va, PM.host_product(n, rp, ci, va, dtype)


def test_laplacian_generator():
    n, _, rp, ci, va = synth.laplacian_2d(5)
    A = PM.dense_of(n, rp, ci, va)
    assert np.array_equal(A, A.T) and np.array_equal(np.diag(A), np.full(n, 4.0)) and A.sum() == 4 * 5          # (only the boundary rows do not sum to 0)
    k = np.arange(1, 6)
    want = np.sort((4 - 2 * np.cos(k * np.pi / 6))[:, None] - 2 * np.cos(k * np.pi / 6)[None, :], axis=None)
    assert np.allclose(np.linalg.eigvalsh(A), want, atol=1e-12)


def test_degree_4_with_estimated_bounds_beats_plain_cg_on_the_laplacian():
    """24 x 24 grid, rtol 1e-8, bounds from the model of cvr_chebyshev_bounds (20 power steps, ratio 30); a plain-fp64 run gave 22 steps against 76"""
    n, rp, ci, va, prod = _laplacian(24)
    lmin, lmax, lam = CM.bounds(prod, n, np.float64, 20, 30.0)
    true_max = 8 * np.cos(np.pi / 50) ** 2
    assert lam <= true_max * (1 + 1e-12) and lmax > true_max, (lam, lmax, true_max)          # the Rayleigh quotient is a lower bound, the margin covers it here
    b = synth.x_rand(n)
    pre = CM.ChebPcg(prod, np.float64, CM.Cheb(4, lmin, lmax, np.float64)).run(b, None, rtol=1e-8, max_iters=400)
    plain = KM.CgModel(prod, np.float64).run(b, None, None, rtol=1e-8, max_iters=400)
    print(f"Chebyshev degree 4: {pre.last.iterations} steps, plain CG: {plain.last.iterations} steps; lambda = {lam:.6g} of {true_max:.6g}")
    assert pre.last.terminal and pre.last.status == KM.CONVERGED
    assert plain.last.terminal and plain.last.status == KM.CONVERGED
    assert pre.last.iterations < plain.last.iterations
    y = PM.dense_of(n, rp, ci, va) @ pre.last.x
    assert np.linalg.norm(b - y) <= 2e-8 * np.linalg.norm(b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degree_one_is_the_diagonal_model(dtype):
    """z = T(c0 * double(r)) is T(double(minv) * double(r)) with minv = T(c0): in fp64 for every c0, in fp32 where c0 is an fp32 value (1 / theta = 0.5)"""
    n, _, rp, ci, va = KM.banded("spd", 250, dtype)
    prod = PM.host_product(n, rp, ci, va, dtype)
    b, x0, _ = KM.inputs(n, dtype)
    lmin, lmax = (0.45, 1.6) if dtype == np.float64 else (0.5, 3.5)
    cheb = CM.Cheb(1, lmin, lmax, dtype)
    minv = np.full(n, cheb.b[0], dtype=dtype)
    assert np.float64(minv[0]) == cheb.b[0]
    got = CM.ChebPcg(prod, dtype, cheb).run(b, x0, rtol=0.0, max_iters=5)
    ref = KM.CgModel(prod, dtype).run(b, x0, minv, rtol=0.0, max_iters=5)
    assert len(got.steps) == len(ref.steps) == 6
    for k, (s, t) in enumerate(zip(got.steps, ref.steps)):
        assert KM.compare(s, t) == "", (k, KM.compare(s, t))


def test_start_vector():
    x = CM.start_vector(5, np.float64)
    assert x[0] == 1.0 and x[1] == 1.0 + 2654435761 / 2.0 ** 32 and x[2] == 1.0 + ((2 * 2654435761) % 2 ** 32) / 2.0 ** 32
    assert ((x >= 1) & (x < 2)).all()
    assert CM.start_vector(70000, np.float32).dtype == np.float32


# ---- the mutants ----
class _RhoNotUpdated(CM.Cheb):
    def carry(self, rho_old, rho_new):
        return rho_old


class _SignFlipped(CM.Cheb):
    def residual(self, r, q):
        return CM._f64(q) - CM._f64(r)


class _NotAccumulated(CM.Cheb):
    def accumulate(self, z, d):
        return d


class _Swapped(CM.Cheb):
    def pair(self, rho_new, rho_old, delta):
        a, b = super().pair(rho_new, rho_old, delta)
        return b, a


def _rejected(good, bad):
    for k in range(min(len(good.steps), len(bad.steps))):
        msg = KM.compare(bad.steps[k], good.steps[k])
        if msg:
            return k, msg
    return None


@pytest.mark.parametrize("mutant", [_RhoNotUpdated, _SignFlipped, _NotAccumulated, _Swapped], ids=lambda m: m.__name__.strip("_"))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_compare_rejects_the_mutant_within_three_steps(mutant, dtype):
    """degree 4 (rho_1 is first read by k = 2) on the 24 x 24 Laplacian"""
    n, rp, ci, va, prod = _laplacian(24, dtype)
    lmin, lmax = 0.3, 8.8
    b = synth.x_rand(n).astype(dtype)
    good = CM.ChebPcg(prod, dtype, CM.Cheb(4, lmin, lmax, dtype)).run(b, None, rtol=0.0, max_iters=3)
    bad = CM.ChebPcg(prod, dtype, mutant(4, lmin, lmax, dtype)).run(b, None, rtol=0.0, max_iters=3)
    hit = _rejected(good, bad)
    assert hit is not None and hit[0] <= 3, hit
    print(mutant.__name__, "rejected at step", *hit)
    # ... and the apply alone differs too
    r = KM.inputs(n, dtype)[0]
    assert CM.Cheb(4, lmin, lmax, dtype).apply(prod, r).tobytes() != mutant(4, lmin, lmax, dtype).apply(prod, r).tobytes()
