"""The numpy model of cvr_svds_device (tests/svds_model.py) on the CPU, with products formed in fp64 from the dense matrix and rounded to T.

Leading triplets: random sparse matrices of 200 x 120 and 120 x 200 and a random band of 300 x 171 and 171 x 300 (both orientations of each), nev = 1,
3, 6, the default ncv, tol = 1e-8 in fp64 and 1e-4 in fp32 (TOL; the model converges on every case within MAX_RESTARTS, which the test checks
first).  Three figures per triplet, all formed in fp64 against numpy.linalg.svd: |sigma - sigma_ref|, ||A v - sigma u||_2 and ||A^T u - sigma v||_2.
Each is at most the triplet's own returned estimate e_c = |beta_m Q[m-1, c]| (the entry's `est`; max_estimate is the largest
e_c / max(eps23, sigma_c), which the test checks) plus a rounding allowance K u_T sigma_max -- not the convergence threshold tol max(eps23, sigma),
under which rounding would be invisible.  K is not derived: the largest (figure - e_c) / (u_T sigma_max) measured over exactly these cases is
svds_model.RESIDUAL_K, fp64 15.7 and fp32 1.50 (both ||A v - sigma u||, which is pure rounding and which the estimate, standing for
||A^T u - sigma v||, does not cover; the largest for ||A^T u - sigma v|| itself is 14.1 in fp64 and 1.45 in fp32, for sigma 12.8 in fp64), and
svds_model.residual_allowance allows 4 times that.  The
vectors are orthonormal within 2 (m + 1) u_T per cycle and triplet, as reasoned in tests/test_lanczos_model_host.py.

Closure: a left half closed at step 2 (v0 with a component in the null space: 2 exact triplets from a 2 x 3 projected matrix), a right half closed
at steps 0 and 2, fewer triplets than nev (CVR_EIG_INVARIANT), a zero matrix and a v0 in the null space (nothing returned), v0 = 0 and NaN.

Twelve mutants: svds_model.compare rejects each wrong recurrence at a size of 40 x 30 (the one that changes only the fp64 accumulation order of
the restart sum shows in fp64 alone: the rounding to fp32 drops the bits it changes)."""
import numpy as np
import pytest

import svds_model as SM

TOL = {np.float64: 1e-8, np.float32: 1e-4}
MAX_RESTARTS = 400


def _systems(dtype):
    for nr, nc in ((200, 120), (120, 200)):
        yield f"random{nr}x{nc}", SM.random_sparse(nr, nc, dtype)
    for nr, nc in ((300, 171), (171, 300)):
        yield f"band{nr}x{nc}", SM.band_rect(nr, nc, dtype)


_RUNS = {}


def _runs(dtype):
    """every (system, nev) once per type: (name, A, reference values, entry)"""
    if dtype not in _RUNS:
        out = []
        for name, (nr, nc, rp, ci, va) in _systems(dtype):
            A = SM.dense_of(nr, nc, rp, ci, va)
            ref = np.linalg.svd(A, compute_uv=False)
            mul, mul_t = SM.dense_products(A, dtype)
            for nev in (1, 3, 6):
                e = SM.svds_model(mul, mul_t, SM.start_vector(nc, dtype), nr, nev, 0, TOL[dtype], MAX_RESTARTS, dtype)
                out.append(((name, nev), A, ref[:nev], e))
        _RUNS[dtype] = out
    return _RUNS[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_model_finds_the_leading_triplets(dtype):
    u = float(np.finfo(dtype).eps) / 2
    worst_k = 0.0
    for ctx, A, ref, e in _runs(dtype):
        nev = ctx[1]
        assert e.status == SM.CONVERGED and e.nconv == nev and e.restarts < MAX_RESTARTS, (ctx, e)
        assert e.max_estimate <= TOL[dtype]
        assert (np.diff(e.svals) <= 0).all()
        bound = e.scalars["est"]          # the returned estimates e_c, one per triplet (max_estimate is the largest e_c / max(eps23, sigma_c))
        assert (bound <= TOL[dtype] * np.maximum(SM.EPS23, e.svals)).all() and e.max_estimate == (bound / np.maximum(SM.EPS23, e.svals)).max()
        U, V = e.U.astype(np.float64), e.V.astype(np.float64)
        figures = (np.abs(e.svals - ref), np.linalg.norm(A @ V - U * e.svals, axis=0), np.linalg.norm(A.T @ U - V * e.svals, axis=0))
        allow = SM.residual_allowance(dtype, ref[0])
        for what, f in zip(("sigma", "A v - sigma u", "A^T u - sigma v"), figures):
            k = ((f - bound) / (u * ref[0])).max()
            worst_k = max(worst_k, k)
            print(f"{ctx} {np.dtype(dtype).name} {what}: figure {f.max():.3g}, estimates {bound.min():.3g} .. {bound.max():.3g}, K {k:.3g}, restarts {e.restarts}")
            assert (f <= bound + allow).all(), (ctx, what, f, bound, allow)
        # orthonormal: see tests/test_lanczos_model_host.py -- 2 (m + 1) u per cycle and triplet, for either block
        m = e.scalars["Q"].shape[0]
        for B in (U, V):
            orth = np.linalg.norm(B.T @ B - np.eye(nev))
            assert orth <= 2 * (m + 1) * u * (e.restarts + 1) * nev, (ctx, orth, e.restarts)
    print(f"{np.dtype(dtype).name}: the largest K measured {worst_k:.3g}, recorded {SM.RESIDUAL_K[np.dtype(dtype).name]}")
    assert worst_k <= 4 * SM.RESIDUAL_K[np.dtype(dtype).name]


# ---- closure
def _diag_case(dtype):
    """A (6 x 7) with A[i, i] = d_i and an empty last column: A^T A = diag(d^2, 0)"""
    d = np.array([3.0, 1.0, 2.5, 0.5, 4.0, 1.5])
    A = np.zeros((6, 7))
    A[np.arange(6), np.arange(6)] = d
    return A, d


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_closed_halves_and_breakdowns(dtype):
    A, d = _diag_case(dtype)
    mul, mul_t = SM.dense_products(A, dtype)
    run = lambda v0, nev, ncv=5: SM.svds_model(mul, mul_t, np.asarray(v0, dtype=dtype), 6, nev, ncv, 1e-8, 5, dtype)          # noqa: E731
    rtol = 1e-6 if dtype == np.float32 else 1e-13
    # v0 = e_4: the right half closes at step 0 with the exact triplet
    e = run(np.eye(7)[4], 1)
    assert (e.status, e.nconv, e.restarts, e.max_estimate, e.spmv_count) == (SM.CONVERGED, 1, 0, 0.0, 10) and e.svals.tolist() == [4.0], e
    assert e.U[:, 0].tolist() == np.eye(6)[4].tolist() and e.V[:, 0].tolist() == np.eye(7)[4].tolist() and (e.scalars["p"], e.scalars["q"]) == (1, 1)
    # three entries with distinct d: the right half closes at step 2 with 3 columns; nev = 2: converged, nev = 4: fewer than wanted
    v = np.zeros(7)
    v[[0, 2, 3]] = (1.0, 2.0, -1.5)
    e = run(v, 2)
    assert (e.status, e.nconv, e.scalars["p"], e.scalars["q"]) == (SM.CONVERGED, 2, 3, 3) and np.allclose(e.svals, [3.0, 2.5], rtol=rtol, atol=0), e
    e = run(v, 4, 6)
    assert (e.status, e.nconv, e.restarts, e.U.shape, e.V.shape) == (SM.INVARIANT, 3, 0, (6, 3), (7, 3)) and np.allclose(e.svals, [3.0, 2.5, 0.5], rtol=rtol, atol=0), e
    # two such entries and a component in the null space: the right space has 3 dimensions, the left one 2 -- the left half closes at step 2, the
    # projected matrix is 2 x 3 and its 2 triplets are exact
    v = np.zeros(7)
    v[[1, 4, 6]] = (1.0, -2.0, 0.7)
    e = run(v, 2)
    assert (e.status, e.nconv, e.scalars["p"], e.scalars["q"], e.max_estimate) == (SM.CONVERGED, 2, 2, 3, 0.0) and np.allclose(e.svals, [4.0, 1.0], rtol=rtol, atol=0), e
    U, V = e.U.astype(np.float64), e.V.astype(np.float64)
    assert np.abs(A @ V - U * e.svals).max() <= 64 * np.finfo(dtype).eps and np.abs(A.T @ U - V * e.svals).max() <= 64 * np.finfo(dtype).eps
    e = run(v, 3)
    assert (e.status, e.nconv, len(e.svals), e.U.shape, e.V.shape) == (SM.INVARIANT, 2, 2, (6, 2), (7, 2)), e
    # v0 in the null space, and a zero matrix: the left half closes at step 0 and nothing is returned
    e = run(np.eye(7)[6], 1)
    assert (e.status, e.nconv, len(e.svals), e.U.shape, e.V.shape, e.max_estimate, e.spmv_count) == (SM.INVARIANT, 0, 0, (6, 0), (7, 0), 0.0, 10), e
    zmul, zmul_t = SM.dense_products(np.zeros((6, 7)), dtype)
    e = SM.svds_model(zmul, zmul_t, np.ones(7, dtype=dtype), 6, 2, 5, 1e-8, 5, dtype)
    assert (e.status, e.nconv, len(e.svals)) == (SM.INVARIANT, 0, 0), e
    # v0 = 0 and a NaN in v0: breakdown, nothing returned
    for bad in (np.zeros(7), np.where(np.arange(7) == 3, np.nan, 1.0)):
        e = run(bad, 2)
        assert (e.status, e.nconv, len(e.svals), e.U.shape, e.V.shape, e.spmv_count, e.restarts) == (SM.BREAKDOWN, 0, 0, (6, 0), (7, 0), 10, 0), e
    # a NaN in A
    B = A.copy()
    B[2, 2] = np.nan
    nmul, nmul_t = SM.dense_products(B, dtype)
    e = SM.svds_model(nmul, nmul_t, np.ones(7, dtype=dtype), 6, 2, 5, 1e-8, 5, dtype)
    assert (e.status, e.nconv, len(e.svals)) == (SM.BREAKDOWN, 0, 0), e


# ---- mutants
class OnePass(SM.SvdsModel):
    def passes(self, B, w):
        h = self.coefficients(B, w)
        w1 = self.subtract(B, h, w)
        return w1, w1, h, np.zeros(len(h))


class CoefficientForNorm(SM.SvdsModel):
    def norm_entry(self, ww, h, d):
        return h[-1] + d[-1] if len(h) else np.sqrt(ww)


class FirstSumInFrontOfThePasses(SM.SvdsModel):
    def first_sum(self, w0, w1):
        return self.dot("w.w", w0, w0)


class CarryWrongColumn(SM.SvdsModel):
    def carry(self, V, m):
        return V[m - 1]


class NoSpike(SM.SvdsModel):
    def spike(self, beta_m, Q, kk):
        return np.zeros(kk)


class SpikeFromP(SM.SvdsModel):
    def spike(self, beta_m, Q, kk):
        return np.array([beta_m * self.last_P[-1, c] for c in range(kk)])

    def small_svd(self, B):
        s, Q, self.last_P = super().small_svd(B)
        return s, Q, self.last_P


class EstimateFromP(SM.SvdsModel):
    def estimate(self, beta_m, Q, P, p, c):
        return abs(beta_m * P[p - 1, c])


class Ascending(SM.SvdsModel):
    def select(self, p, count):
        return list(range(count))[::-1]


class KeepWithoutNconv(SM.SvdsModel):
    def keep(self, nev, nconv, m):
        return nev


class RightHalfWithoutTheNewestColumn(SM.SvdsModel):
    def right_columns(self, V, j):
        return V[:j]


class LowerBidiagonal(SM.SvdsModel):
    def projected(self, p, q, k, sigma, spike, alpha, beta):
        return super().projected(p, q, k, sigma, spike, alpha, beta).T.copy() if p == q else super().projected(p, q, k, sigma, spike, alpha, beta)


class DescendingSum(SM.SvdsModel):
    def restart_sum(self, s, B):
        u = np.zeros(len(B[0]))
        for sl, b in zip(s[::-1], B[::-1]):
            u = u + sl * SM._f64(b)
        return self.rnd(u)


MUTANTS = [OnePass, CoefficientForNorm, FirstSumInFrontOfThePasses, CarryWrongColumn, NoSpike, SpikeFromP, EstimateFromP, Ascending, KeepWithoutNconv,
           RightHalfWithoutTheNewestColumn, LowerBidiagonal, DescendingSum]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__ for m in MUTANTS])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_compare_rejects_a_wrong_recurrence(mutant, dtype):
    """band_rect(40, 30), nev = 3, ncv = 8, a loose tol so that a restart sees some of the wanted triplets converged and some not"""
    nr, nc, rp, ci, va = SM.band_rect(40, 30, dtype)
    mul, mul_t = SM.dense_products(SM.dense_of(nr, nc, rp, ci, va), dtype)
    v0, tol = SM.start_vector(nc, dtype), 1e-3
    right = SM.SvdsModel(mul, mul_t, dtype)
    want = right.run(v0, nr, 3, 8, tol, 6)
    assert want.restarts >= 2 and any(0 < h.nconv < 3 for h in right.history), [h.nconv for h in right.history]
    again = SM.SvdsModel(mul, mul_t, dtype).run(v0, nr, 3, 8, tol, 6)
    assert SM.compare(again, want) == ""
    if dtype == np.float32 and mutant is DescendingSum:
        # (the restart sum is accumulated in fp64 and rounded to T once: in fp32 another order changes bits that the rounding to T drops; fp64
        # shows it at once)
        assert SM.compare(mutant(mul, mul_t, np.float64).run(v0, nr, 3, 8, tol, 1), SM.SvdsModel(mul, mul_t, np.float64).run(v0, nr, 3, 8, tol, 1)) != ""
        return
    msg = SM.compare(mutant(mul, mul_t, dtype).run(v0, nr, 3, 8, tol, 6), want)
    assert msg != "", mutant.__name__


def test_compare_looks_at_every_field():
    nr, nc, rp, ci, va = SM.band_rect(40, 30, np.float64)
    mul, mul_t = SM.dense_products(SM.dense_of(nr, nc, rp, ci, va), np.float64)
    want = SM.svds_model(mul, mul_t, SM.start_vector(nc, np.float64), nr, 3, 8, 1e-3, 2)
    for field, value in (("nconv", want.nconv + 1), ("status", 7), ("restarts", 9), ("spmv_count", 1), ("max_estimate", np.nextafter(want.max_estimate, 1.0))):
        got = SM.SvdEntry(want.svals, want.U, want.V, want.nconv, want.status, want.restarts, want.spmv_count, want.max_estimate)
        setattr(got, field, value)
        assert field in SM.compare(got, want)
    sv = want.svals.copy()
    sv[1] = np.nextafter(sv[1], 0.0)
    assert "svals" in SM.compare(SM.SvdEntry(sv, want.U, want.V, want.nconv, want.status, want.restarts, want.spmv_count, want.max_estimate), want)
    for name in ("U", "V"):
        blocks = {"U": want.U.copy(), "V": want.V.copy()}
        blocks[name][5, 2] = np.nextafter(blocks[name][5, 2], 9.0)
        got = SM.SvdEntry(want.svals, blocks["U"], blocks["V"], want.nconv, want.status, want.restarts, want.spmv_count, want.max_estimate)
        assert name in SM.compare(got, want) and SM.compare(got, want, vectors=False) == "" and SM.compare(got, want, vectors="V" if name == "U" else "U") == ""
