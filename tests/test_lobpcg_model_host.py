"""The numpy model of cvr_lobpcg_device (tests/lobpcg_model.py) on the CPU: it finds the lowest eigenpairs within the residual bound of symmetric
matrices, its block is orthonormal, the residuals it reports are those of the block it returns, the Cholesky fallback engages on a constructed case
and the solve still converges, and the checks reject three wrong recurrences.  No GPU: the product is a dense fp64 one rounded to T.

The bounds.  For a symmetric A and a unit x, an eigenvalue lies within ||A x - theta x|| of theta; numpy's eigvalsh has an error of its own of a few
eps ||A||, taken as REF_ERR = 16 eps ||A||_1.  With no locking a converged column goes on converging, so its reported residual falls below that:
the sum of the two, and of what one rounded product may hide of the true residual (below), is the bound.  Orthonormality: G = X^T X is formed in fp64 and the combination is rounded once per value, so |X^T X - I| stays at
a few eps per entry whatever n is; 64 eps.  Reported against recomputed residuals: the allowance of one rounded product (1e-12 * sum |a_ij x_j| row-wise,
in norm), the parity tests' own."""
import numpy as np
import pytest

import krylov_model as KM
import lobpcg_model as LM

DT = np.float64
EPS = float(np.finfo(DT).eps)


def _matrix(name):
    if name == "lap24":
        return LM.laplacian_grid(24, 24, DT)
    if name == "lap40x12":
        return LM.laplacian_grid(40, 12, DT)
    return LM.banded(257, DT)


_CACHE = {}


def _dense(name):
    if name not in _CACHE:
        n, _, rp, ci, va = _matrix(name)
        A = LM.dense_of(n, rp, ci, va)
        _CACHE[name] = (n, A, np.linalg.eigh(A))
    return _CACHE[name]


def _bound(e, A):
    """the reported residual, what one rounded product may hide of the true one, and the reference's own error"""
    return e.resnorms + LM.residual_allowance(np.abs(A), e.X, 1e-12) + 16 * EPS * np.abs(A).sum(axis=0).max()


def _check(e, A, lam, k):
    """"" when the entry passes the three checks, else what fails"""
    if e.status != LM.CONVERGED:
        return f"status {e.status} after {e.iterations} iterations"
    X = e.X.astype(np.float64)
    if not (np.abs(e.evals - lam[:k]) <= _bound(e, A)).all():
        return f"eigenvalues {e.evals!r} against {lam[:k]!r}, residuals {e.resnorms!r}"
    if not np.abs(X.T @ X - np.eye(k)).max() <= 64 * EPS:
        return f"X^T X - I = {np.abs(X.T @ X - np.eye(k)).max():.3g}"
    true = np.linalg.norm(A @ X - X * e.evals, axis=0)
    if not (np.abs(true - e.resnorms) <= LM.residual_allowance(np.abs(A), X, 1e-12)).all():
        return f"reported residuals {e.resnorms!r}, recomputed {true!r}"
    return ""


def test_tree_sum_many_is_tree_sum():
    rng = np.random.default_rng(3)
    for n, pack in ((1, 2), (5, 4), (513, 2), (1000, 4), (4097, 2)):
        t = rng.standard_normal((4, n))
        assert LM.tree_sum_many(t, pack).tobytes() == np.array([KM.tree_sum(r, pack) for r in t]).tobytes(), (n, pack)


@pytest.mark.parametrize("k", [1, 3, 4, 8])
@pytest.mark.parametrize("name", ["lap24", "lap40x12", "band257"])
def test_the_model_finds_the_lowest_pairs(name, k):
    n, A, (lam, _) = _dense(name)
    e = LM.lobpcg_model(LM.dense_product(A, DT), LM.start_block(n, k, DT), None, LM.SMALLEST, 1e-8, 1500)
    print(f"{name} k={k}: {e.iterations} iterations, {e.restarts_without_p} without P, max |theta - lambda| {np.abs(e.evals - lam[:k]).max():.3g}")
    assert _check(e, A, lam, k) == "", (name, k)
    assert e.spmv_count == k * (2 + e.iterations) and e.precond_applies == 0          # the pass that saw the convergence had its products enqueued


def test_the_largest_end():
    n, A, (lam, _) = _dense("lap24")
    e = LM.lobpcg_model(LM.dense_product(A, DT), LM.start_block(n, 4, DT), None, LM.LARGEST, 1e-8, 1500)
    assert e.status == LM.CONVERGED and (np.abs(e.evals - lam[-4:]) <= _bound(e, A)).all(), e


def test_the_fallback_engages_and_the_solve_converges():
    """an exact inverse as M and a start block whose first two columns are eigenvectors already: their residuals are rounding noise, their directions
    P fall into the span of X and W, the Cholesky step meets a bad pivot at 3k and the iteration goes on with S = [X W]"""
    n, A, (lam, V) = _dense("lap24")
    Ai = np.linalg.inv(A)
    X0 = LM.start_block(n, 4, DT)
    X0[:, :2] = V[:, :2]
    e = LM.lobpcg_model(LM.dense_product(A, DT), X0, lambda r: Ai @ r, LM.SMALLEST, 1e-8, 200)
    assert e.restarts_without_p >= 1, e
    assert _check(e, A, lam, 4) == "", e
    assert e.precond_applies == 4 * (1 + e.iterations)
    # the exact inverse pays: the plain solve of the same block takes several times as many iterations
    plain = LM.lobpcg_model(LM.dense_product(A, DT), X0, None, LM.SMALLEST, 1e-8, 1500)
    assert plain.status == LM.CONVERGED and 3 * e.iterations <= plain.iterations, (e.iterations, plain.iterations)


def test_max_iters_zero_is_the_rayleigh_ritz_of_the_start_block():
    n, A, (lam, _) = _dense("lap40x12")
    X0 = LM.start_block(n, 3, DT)
    e = LM.lobpcg_model(LM.dense_product(A, DT), X0, None, LM.SMALLEST, 1e-8, 0)
    assert (e.status, e.iterations, e.spmv_count) == (LM.MAX_ITERS, 0, 3)
    Q, _ = np.linalg.qr(X0)
    assert np.allclose(e.evals, np.linalg.eigvalsh(Q.T @ A @ Q), rtol=1e-12, atol=0)


@pytest.mark.parametrize("name,k", sorted(key for key in LM.FP32_TOL if key[0] in ("band63", "band64", "band65")))
def test_the_recorded_fp32_tolerances(name, k):
    """the table the GPU test takes its fp32 tolerances from is what the procedure gives: every entry of the three smallest matrices (about a
    minute together), the one the fused product moves to 1e-6 among them"""
    n, _, rp, ci, va = LM.banded(int(name[4:]), np.float32)
    assert LM.fp32_tolerance(n, rp, ci, va, k) == LM.FP32_TOL[(name, k)]


def test_fused_product_is_a_product():
    n, _, rp, ci, va = LM.banded(65, np.float32)
    x = LM.start_block(n, 1, np.float32)[:, 0]
    A = LM.dense_of(n, rp, ci, va)
    y = LM.fused_product(n, rp, ci, va)(x)
    assert y.dtype == np.float32 and (np.abs(y - A @ x.astype(np.float64)) <= 5 * 2.0 ** -24 * (np.abs(A) @ np.abs(x).astype(np.float64))).all()


class OnePass(LM.LobpcgModel):
    passes = 1


class PNotZeroed(LM.LobpcgModel):
    def p_first_row(self, k):
        return 0


class WrongTheta(LM.LobpcgModel):
    def residual_theta(self, theta, c):
        return theta[(c + 1) % len(theta)]


def _w_is_orthogonal_to_x(mutant):
    """W after step 3 is orthogonal to X to a few units of rounding, also where the apply puts most of W along X (an exact inverse: M R is
    dominated by the lowest modes, which X holds).  One pass leaves eps times the norm it removed; the second pass is what brings 64 eps."""
    n, A, (lam, _) = _dense("lap24")
    Ai = np.linalg.inv(A)
    M = mutant(LM.dense_product(A, DT), DT, lambda r: Ai @ r)
    M.run(LM.start_block(n, 4, DT), LM.SMALLEST, 1e-8, 200)
    return M.worst_xtw <= 64 * EPS, M.worst_xtw


def test_w_is_orthogonal_to_x():
    ok, worst = _w_is_orthogonal_to_x(LM.LobpcgModel)
    assert ok, worst


@pytest.mark.parametrize("mutant", [OnePass, PNotZeroed, WrongTheta])
def test_mutants_are_caught(mutant):
    """each wrong recurrence fails the checks above on at least one of the cases they run on"""
    failures = []
    ok, worst = _w_is_orthogonal_to_x(mutant)
    if not ok:
        failures.append(("X^T W", worst))
    for name, k in (("lap24", 4), ("band257", 4), ("lap40x12", 8)):
        n, A, (lam, _) = _dense(name)
        e = mutant(LM.dense_product(A, DT), DT).run(LM.start_block(n, k, DT), LM.SMALLEST, 1e-8, 1500)
        msg = _check(e, A, lam, k)
        if msg:
            failures.append((name, k, msg[:80]))
    print(mutant.__name__, failures)
    assert failures, mutant.__name__
