"""The numpy model of cvr_eigsh_device (tests/lanczos_model.py) and the library's small eigensolver cvr_sym_eig_host on the CPU.

cvr_sym_eig_host against numpy.linalg.eigh (LAPACK) at m = 1, 2, 3, 20, 64 on random symmetric matrices, a diagonal one, repeated eigenvalues, the
arrow-plus-tridiagonal shape the solver produces, lda > m and garbage in the triangle that is not read.  Three figures per matrix -- max |w - w_ref|,
||A Z - Z W||_F and ||Z^T Z - I||_F -- each at most 8 x max(LAPACK's own figure on the same matrix, m 2^-53 ||A||_F).  The worst ratios to that
maximum measured here (x86-64, this test's matrices): 0.78 for the values, 0.70 for the residual, 0.93 for the orthogonality (all three at m = 3;
0.03, 0.22 and 0.10 at m = 64); allowed: 8.

The model with the oracle's CSR product on the 1-D Laplacian (n = 64, 257), golden/sym250_real and an indefinite random band, both ends, nev = 1, 3, 6,
tol = 1e-8 in fp64 and 1e-4 in fp32 (TOL; the model converges on every case within MAX_RESTARTS, which the test checks first): the values are
numpy.linalg.eigvalsh's within tol max(eps23, |theta|) + the allowance, the vectors orthonormal, and a pair's true residual ||A v - theta v||_2 at most
its estimate's bound tol max(eps23, |theta|) + K u_T ||A||_1.  K is not derived: the largest value measured over exactly these cases is
lanczos_model.RESIDUAL_K (fp32 1.72; fp64 0: every residual stayed below its estimate's bound, the nearest at 0.81 of it), and
lanczos_model.residual_allowance allows 4 times that.  The vectors are orthonormal within 2 (m + 1) u_T per cycle and pair (reasoned in the test).

Nine mutants: lanczos_model.compare rejects each wrong recurrence at a size of 40 (the two that change only the fp64 accumulation of the restart sum
show in fp64 alone: the rounding to fp32 drops the bits they change)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import lanczos_model as LM
import oraclelib as O
from cvr_amd import capi, synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = {np.float64: 1e-8, np.float32: 1e-4}
MAX_RESTARTS = 400


# ---- cvr_sym_eig_host
def _arrow(m, k, rng):
    """diag(theta) of k entries, the arrow in row k, tridiagonal beyond: the solver's projected matrix"""
    A = np.zeros((m, m))
    A[np.arange(m), np.arange(m)] = rng.standard_normal(m)
    if k < m:
        A[k, :k] = A[:k, k] = 1e-3 * rng.standard_normal(k)
    for j in range(k, m - 1):
        A[j + 1, j] = A[j, j + 1] = abs(rng.standard_normal())
    return A


def _matrices(m):
    rng = np.random.default_rng(20261019 + m)
    R = rng.standard_normal((m, m))
    yield "random", R + R.T
    yield "diagonal", np.diag(rng.standard_normal(m) * 3)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    yield "repeated", (Q * np.repeat([1.0, 2.0, 5.0], -(-m // 3))[:m]) @ Q.T
    yield "arrow", _arrow(m, m // 3, rng)
    yield "tridiagonal", _arrow(m, 0, rng)


def _figures(A, w, Z, w_ref):
    m = len(w)
    return np.abs(w - w_ref).max(), np.linalg.norm(A @ Z - Z * w), np.linalg.norm(Z.T @ Z - np.eye(m))


@pytest.mark.parametrize("m", [1, 2, 3, 20, 64])
def test_sym_eig_host_against_lapack(m):
    L = capi.lib()
    worst = np.zeros(3)
    for name, A in _matrices(m):
        A = (A + A.T) / 2
        w_ref, Z_ref = np.linalg.eigh(A)
        floor = m * 2.0 ** -53 * np.linalg.norm(A)
        lap = _figures(A, w_ref, Z_ref, w_ref)
        for lda in (m, m + 5):
            a = np.full((m, lda), 1e300, order="C")          # a[j, i] in C order is element (i, j) at i + j * lda; rows of garbage beyond m
            for j in range(m):
                a[j, j:m] = A[j:, j]                          # the lower triangle; the upper one keeps the garbage
            w, z = np.zeros(m), np.zeros((m, m + 2))
            assert L.cvr_sym_eig_host(m, a.ctypes.data, lda, w.ctypes.data, z.ctypes.data, m + 2) == 0, capi.last_error()
            Z = z[:, :m].T.copy()
            fig = _figures(A, w, Z, w_ref)
            for i, (f, l) in enumerate(zip(fig, lap)):
                ratio = f / max(l, floor)
                worst[i] = max(worst[i], ratio)
                assert f <= 8 * max(l, floor), (name, m, lda, i, f, l, floor)
            assert (np.diff(w) >= 0).all(), (name, w)
            for c in range(m):          # the sign rule: the first component of largest magnitude is positive
                assert Z[int(np.argmax(np.abs(Z[:, c]))), c] > 0, (name, c)
            w2, z2 = np.zeros(m), np.zeros((m, m + 2))
            assert L.cvr_sym_eig_host(m, a.ctypes.data, lda, w2.ctypes.data, z2.ctypes.data, m + 2) == 0
            assert w2.tobytes() == w.tobytes() and z2.tobytes() == z.tobytes(), "two calls differ"
            wv = capi.sym_eig_host(A, vectors=False)
            assert wv.tobytes() == w.tobytes()
    print(f"m = {m}: worst ratios to max(LAPACK, floor): values {worst[0]:.3g}, residual {worst[1]:.3g}, orthogonality {worst[2]:.3g}")


def test_sym_eig_host_ties_keep_their_order():
    w, Z = capi.sym_eig_host(np.diag([3.0, 1.0, 3.0, 1.0]))
    assert w.tolist() == [1.0, 1.0, 3.0, 3.0]
    assert [int(np.argmax(Z[:, c])) for c in range(4)] == [1, 3, 0, 2]


# ---- the model with the oracle's CSR product
def _sym250(dtype):
    z = np.load(os.path.join(GOLD, "sym250_real.npz"))
    n = int(z["dims"][1]) + 1          # (the reference loader's arrays, read literally)
    return synth.spd_from_pattern(n, z["csr_rowptr"].astype(np.int64), z["csr_col"], dtype=dtype)


def _systems(dtype):
    yield "laplacian64", LM.laplacian_1d(64, dtype), 0
    yield "laplacian257", LM.laplacian_1d(257, dtype), 40
    yield "sym250", _sym250(dtype), 0
    yield "band300", LM.band_indefinite(300, dtype), 0


def _product(rp, ci, va):
    return lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)


_RUNS = {}


def _runs(dtype):
    """every (system, end, nev) once per type: (name, A, reference values at that end, entry)"""
    if dtype not in _RUNS:
        out = []
        for name, (n, _, rp, ci, va), ncv in _systems(dtype):
            A = LM.dense_of(n, rp, ci, va)
            assert (A == A.T).all(), name
            ref = np.linalg.eigvalsh(A)
            for which in (LM.LARGEST, LM.SMALLEST):
                for nev in (1, 3, 6):
                    e = LM.eigsh_model(_product(rp, ci, va), LM.start_vector(n, dtype), nev, which, ncv, TOL[dtype], MAX_RESTARTS, dtype)
                    out.append(((name, which, nev), A, ref[-nev:] if which == LM.LARGEST else ref[:nev], e))
        _RUNS[dtype] = out
    return _RUNS[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_model_finds_the_extreme_pairs(dtype):
    u = float(np.finfo(dtype).eps) / 2
    worst_k = 0.0
    for ctx, A, ref, e in _runs(dtype):
        nev = ctx[2]
        assert e.status == LM.CONVERGED and e.nconv == nev and e.restarts < MAX_RESTARTS, (ctx, e)
        anorm1 = np.abs(A).sum(axis=0).max()
        scale = np.maximum(LM.EPS23, np.abs(e.evals))
        assert e.max_estimate <= TOL[dtype]
        V = e.evecs.astype(np.float64)
        res = np.linalg.norm(A @ V - V * e.evals, axis=0)
        k = ((res - TOL[dtype] * scale) / (u * anorm1)).max()
        worst_k = max(worst_k, k)
        allow = LM.residual_allowance(dtype, anorm1)
        assert (res <= TOL[dtype] * scale + allow).all(), (ctx, res, TOL[dtype] * scale, allow)
        assert (np.abs(e.evals - ref) <= TOL[dtype] * scale + allow).all(), (ctx, e.evals, ref)
        # orthonormal: Gram-Schmidt applied twice leaves a cycle's basis orthonormal to the order of m u, a restart's product adds (m + 1) u per column,
        # and nothing renormalises: 2 (m + 1) u per cycle and pair
        m = e.scalars["S"].shape[0]
        orth = np.linalg.norm(V.T @ V - np.eye(nev))
        assert orth <= 2 * (m + 1) * u * (e.restarts + 1) * nev, (ctx, orth, e.restarts)
        if ctx[0].startswith("laplacian"):
            exact = LM.laplacian_eigs(A.shape[0])
            want = exact[-nev:] if ctx[1] == LM.LARGEST else exact[:nev]
            assert (np.abs(e.evals - want) <= TOL[dtype] * scale + allow).all(), (ctx, e.evals, want)
    print(f"{np.dtype(dtype).name}: the largest K measured {worst_k:.3g}, recorded {LM.RESIDUAL_K[np.dtype(dtype).name]}")
    assert worst_k <= 4 * LM.RESIDUAL_K[np.dtype(dtype).name]


# ---- mutants
class AlphaFromPassOne(LM.LanczosModel):
    def alpha(self, h, d, j):
        return h[j]


class NoArrow(LM.LanczosModel):
    def arrow(self, beta_m, S, sel):
        return np.zeros(len(sel))


class KeepWithoutNconv(LM.LanczosModel):
    def keep(self, nev, nconv, m):
        return nev


class WrongEnd(LM.LanczosModel):
    def select(self, which, q, count):
        return super().select(1 - which, q, count) if count > self.nev_wanted else super().select(which, q, count)


class Descending(LM.LanczosModel):
    def restart_sum(self, s, V):
        u = np.zeros(len(V[0]))
        for sl, v in zip(s[::-1], V[::-1]):
            u = u + sl * LM._f64(v)
        return self.rnd(u)


class Fused(LM.LanczosModel):
    def restart_sum(self, s, V):
        u = [Fraction(0)] * len(V[0])
        for sl, v in zip(s, V):
            u = [Fraction(float(Fraction(float(sl)) * Fraction(float(x)) + a)) for x, a in zip(v, u)]          # one rounding per multiply-add
        return self.rnd(np.array([float(a) for a in u]))


class CarryWrongColumn(LM.LanczosModel):
    def carry(self, V, m):
        return V[m - 1]


class EstimateFromFirstRow(LM.LanczosModel):
    def estimate(self, beta_q, S, q, c):
        return abs(beta_q * S[0, c])


class BetaFromOldW(LM.LanczosModel):
    def beta_sum(self, w_new, w_old):
        return self.dot("w.w", w_old, w_old)


MUTANTS = [AlphaFromPassOne, NoArrow, KeepWithoutNconv, WrongEnd, Descending, Fused, CarryWrongColumn, EstimateFromFirstRow, BetaFromOldW]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__ for m in MUTANTS])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_compare_rejects_a_wrong_recurrence(mutant, dtype):
    """band_indefinite(40), nev = 3, ncv = 8, a loose tol so that a restart sees some of the wanted pairs converged and some not"""
    n, _, rp, ci, va = LM.band_indefinite(40, dtype)
    v0, tol = LM.start_vector(n, dtype), 1e-3
    right = LM.LanczosModel(_product(rp, ci, va), dtype)
    want = right.run(v0, 3, LM.LARGEST, 8, tol, 6)
    assert want.restarts >= 2 and any(0 < h.nconv < 3 for h in right.history), [h.nconv for h in right.history]
    again = LM.LanczosModel(_product(rp, ci, va), dtype).run(v0, 3, LM.LARGEST, 8, tol, 6)
    assert LM.compare(again, want) == ""
    if dtype == np.float32 and mutant in (Descending, Fused):
        # (the restart sum is accumulated in fp64 and rounded to T once: in fp32 another order or a fused step changes bits that the rounding to
        # T drops -- it shows once in about 2^29 values, at no size a test can afford; fp64 shows it at once)
        assert LM.compare(mutant(_product(rp, ci, va), np.float64).run(v0, 3, LM.LARGEST, 8, tol, 1),
                          LM.LanczosModel(_product(rp, ci, va), np.float64).run(v0, 3, LM.LARGEST, 8, tol, 1)) != ""
        return
    M = mutant(_product(rp, ci, va), dtype)
    M.nev_wanted = 3          # (WrongEnd: the kept pairs from the wrong end, the returned ones from the right one)
    msg = LM.compare(M.run(v0, 3, LM.LARGEST, 8, tol, 6), want)
    assert msg != "", mutant.__name__
