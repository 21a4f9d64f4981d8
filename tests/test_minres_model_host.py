"""CPU: the numpy model of cvr_minres_device (tests/minres_model.py) before it meets a GPU -- that the recurrence of include/cvr_amd.h, with its rounding
points, solves symmetric indefinite and shifted systems to the accuracy its stop test promises, that its residual norm never increases, that it beats
conjugate gradients' residual on an SPD matrix and converges where they break down, and that the comparison the GPU tests use has teeth: every mutant
below is the model with one method replaced, and `compare` must tell it from the model within three steps.

The bounds, with S = A - shift I, d = minv (1 without a preconditioner), R(x) = sqrt(sum d_i r_i^2) for r = b - S x, the norm residual_norm is measured
in:
  * |residual_norm - R(x)| <= minres_model.residual_gap at every entry.  Not derived (the Lanczos vectors lose orthogonality): the largest ratio to
    eps(T) (||S||_2 ||x|| + ||b||) measured here with exact sums is 0.872 (kkt200+100, fp64, minv), and GAP allows 4 times that
    (minres_model.GAP).
  * a converged run says residual_norm <= rtol b_norm, so R(x) <= rtol b_norm + gap; R(x) >= sqrt(min d) ||r||_2 and x - x* = S^-1 r:
    ||x - x*||_2 <= (rtol b_norm + gap) / (sqrt(min d) min |lambda(S)|).  Derived; no factor on top."""
import numpy as np
import pytest

import krylov_model as KM
import minres_model as MM
import oraclelib as O

RTOL = {np.float64: 1e-10, np.float32: 1e-5}
CASES = ["kkt40+20", "kkt200+100", "banded1-2I", "banded5-2I", "banded129-2I"]


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _product(rp, ci, va):
    return lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)


_ref_cache = {}


def _reference(name, dtype):
    """(n, product, shift, b, x0, minv, S dense, ||S||_2, min |lambda(S)|), computed once per case and left unchanged"""
    key = (name, dtype)
    if key not in _ref_cache:
        if name.startswith("kkt"):
            n1, n2 = (int(s) for s in name[3:].split("+"))
            n, _, rp, ci, va = MM.kkt(n1, n2, dtype)
            shift = 0.0
            b, x0, minv = KM.inputs(n, dtype)
        else:
            n, _, rp, ci, va = KM.banded("spd", int(name[6:].split("-")[0]), dtype)
            shift = 2.0
            b, x0, minv = MM.shifted_inputs(n, dtype)
        S = MM.dense_of(n, rp, ci, va) - shift * np.eye(n)
        ev = np.linalg.eigvalsh(S)
        _ref_cache[key] = (n, _product(rp, ci, va), shift, b, x0, minv, S, float(np.abs(ev).max()), float(np.abs(ev).min()), ev)
    return _ref_cache[key]


def _true_residual(S, b, x, d):
    r = b.astype(np.float64) - S @ x.astype(np.float64)
    return float(np.sqrt((d * r * r).sum()))


def test_generators_are_what_they_say():
    for n1, n2 in ((40, 20), (200, 100), (44, 22), (201, 100), (5, 2), (2, 1)):
        for dtype in (np.float64, np.float32):
            n, _, rp, ci, va = MM.kkt(n1, n2, dtype)
            A = MM.dense_of(n, rp, ci, va)
            assert n == n1 + n2 and va.dtype == dtype and rp[-1] == len(ci) == len(va) and np.array_equal(A, A.T)
            for r in range(n):
                assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)
            assert not A[n1:, n1:].any() and np.array_equal(A[n1:, :n1] @ A[n1:, :n1].T, 1.25 * np.eye(n2))
            if n1 >= 40:
                ev = np.linalg.eigvalsh(A)
                neg, pos = ev[ev < 0], ev[ev > 0]
                assert len(neg) == n2 and len(pos) == n1 and -0.90 <= neg.min() and neg.max() <= -0.59 and 0.5 <= pos.min() and pos.max() <= 2.10, (neg.min(), neg.max(), pos.min(), pos.max())
    for name in CASES[2:]:
        ev = _reference(name, np.float64)[9]
        assert -1.5 - 1e-12 <= ev.min() and ev.max() <= -0.5 + 1e-12, (name, ev.min(), ev.max())          # (the bounds of Gershgorin, attained at n = 5; eigvalsh's own rounding)
    assert _reference("banded1-2I", np.float64)[6].tolist() == [[-1.0]]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "minv"])
@pytest.mark.parametrize("name", CASES)
def test_model_solves_the_system_within_the_bound_of_its_stop_test(name, pre, prec):
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    n, prod, shift, b, x0, minv, S, snorm, lmin, _ = _reference(name, dtype)
    xs = np.linalg.solve(S, b.astype(np.float64))
    d = minv.astype(np.float64) if pre else np.ones(n)
    worst_gap = 0.0
    for sums in ("tree", "exact"):
        steps = []
        for start in (None, x0):
            tr = MM.minres_model(prod, b, start, minv if pre else None, shift, rtol, 400, dtype, sums)
            last = tr.last
            assert last.terminal and last.status == KM.CONVERGED and len(tr.steps) == last.iterations + 1, (name, last)
            assert last.x.dtype == dtype and last.x.shape == (n,)
            steps.append(last.iterations)
            # the residual norm of the recurrence is the true one within the gap, at every entry, and never increases
            for k, e in enumerate(tr.steps):
                gap = abs(float(e.residual_norm) - _true_residual(S, b, e.x, d))
                allowed = MM.residual_gap(dtype, snorm, e.x, b)
                if sums == "exact":
                    worst_gap = max(worst_gap, gap / (allowed / MM.GAP))
                assert gap <= allowed, (name, sums, k, gap, allowed)
                assert k == 0 or e.residual_norm <= tr.steps[k - 1].residual_norm, (name, sums, k)
            assert last.residual_norm <= rtol * last.b_norm
            bn = np.sqrt((d * b.astype(np.float64) ** 2).sum())
            assert abs(float(last.b_norm) - bn) <= 1e-6 * bn
            err = np.linalg.norm(last.x.astype(np.float64) - xs)
            bound = (rtol * float(last.b_norm) + MM.residual_gap(dtype, snorm, last.x, b)) / (np.sqrt(d.min()) * lmin)
            assert err <= bound, (name, sums, err, bound)
            # the entries before the stop are those of a run that never stops
            free = MM.minres_model(prod, b, start, minv if pre else None, shift, 0.0, min(3, last.iterations - 1), dtype, sums)
            for k in range(len(free.steps)):
                assert MM.compare(free.at(k), free.at(k).scalars["info"], tr.at(k)) == "", k
        if name.startswith("kkt") and sums == "tree":
            n1, n2 = (int(s) for s in name[3:].split("+"))
            assert max(steps) <= MM.KKT_STEPS[(n1, n2, prec, pre)] <= 400, (name, prec, pre, steps)
    print(f"{name} {prec} {'minv' if pre else 'plain'}: largest |residual_norm - true| / (eps (|S| |x| + |b|)) with exact sums = {worst_gap:.3g}")


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_beta_zero_ends_in_the_stop_test_at_rtol_zero(prec):
    """A - 2 I = (-1) with b = 2: y = 0 after step 0, beta' == 0, phibar == 0: converged although rtol = 0"""
    dtype = _dtype(prec)
    n, prod, shift, b, x0, minv, *_ = _reference("banded1-2I", dtype)
    last = MM.minres_model(prod, b, None, None, shift, 0.0, 5, dtype).last
    assert (last.status, last.iterations, last.terminal, float(last.residual_norm), last.scalars["beta"]) == (KM.CONVERGED, 1, True, 0.0, 0.0)
    assert last.x.tolist() == [-2.0]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_true_residual_is_no_larger_than_conjugate_gradients_on_an_spd_matrix(prec):
    """both iterates lie in x0 + the same Krylov space, over which MINRES minimises ||r||_2; in floating point up to the gap above"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = KM.banded("spd", 129, dtype)
    prod = _product(rp, ci, va)
    A = MM.dense_of(n, rp, ci, va)
    b, x0, _ = KM.inputs(n, dtype)
    for start in (None, x0):
        mr = MM.minres_model(prod, b, start, None, 0.0, 0.0, 10, dtype)
        cg = KM.cg_model(prod, b, start, None, 0.0, 10, dtype)
        assert len(mr.steps) == len(cg.steps) == 11
        for k in range(11):
            rm, rc = _true_residual(A, b, mr.steps[k].x, 1.0), _true_residual(A, b, cg.steps[k].x, 1.0)
            assert rm <= rc + MM.residual_gap(dtype, 1.5, mr.steps[k].x, b), (k, rm, rc)
        assert _true_residual(A, b, mr.steps[5].x, 1.0) < 0.999 * _true_residual(A, b, cg.steps[5].x, 1.0)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", CASES[:2])
def test_conjugate_gradients_fail_where_minres_converges(name, prec):
    dtype = _dtype(prec)
    n, prod, shift, b, x0, minv, *_ = _reference(name, dtype)
    cg = KM.cg_model(prod, b, None, None, RTOL[dtype], 400, dtype).last
    mr = MM.minres_model(prod, b, None, None, 0.0, RTOL[dtype], 400, dtype).last
    print(f"{name} {prec}: CG status {cg.status} after {cg.iterations} steps, MINRES status {mr.status} after {mr.iterations}")
    assert cg.status in (KM.BREAKDOWN, KM.MAX_ITERS) and mr.status == KM.CONVERGED


def test_stop_rules_of_the_start():
    dtype = np.float64
    n, prod, shift, b, x0, minv, *_ = _reference("kkt40+20", dtype)
    z = MM.minres_model(prod, np.zeros(n), x0, minv, 0.0, 1e-10).last          # b.b == 0: x = 0 whatever the start
    assert (z.status, z.iterations, z.terminal, z.residual_norm) == (KM.CONVERGED, 0, True, 0.0) and not z.x.any()
    # a start within the tolerance: x untouched
    solved = MM.minres_model(prod, b, None, None, 0.0, 1e-13, 400).last
    assert solved.status == KM.CONVERGED
    s = MM.minres_model(prod, b, solved.x, None, 0.0, 1e-10).last
    assert (s.status, s.iterations, s.terminal) == (KM.CONVERGED, 0, True) and np.array_equal(s.x, solved.x)
    # a negative entry in minv that makes r2.z negative, and a NaN in b: breakdown with x untouched
    bad = minv.copy()
    bad[:] = -bad
    q = MM.minres_model(prod, b, x0, bad, 0.0, 1e-10).last
    assert (q.status, q.iterations, q.terminal) == (KM.BREAKDOWN, 0, True) and np.array_equal(q.x, x0) and np.isnan(q.residual_norm)
    bn = b.copy()
    bn[3] = np.nan
    q = MM.minres_model(prod, bn, x0, None, 0.0, 1e-10).last
    assert (q.status, q.iterations, q.terminal) == (KM.BREAKDOWN, 0, True) and np.array_equal(q.x, x0)
    # max_iters = 0 forms the start only
    f = MM.minres_model(prod, b, x0, minv, 0.0, 0.0, 0)
    assert len(f.steps) == 1 and f.last.status == KM.MAX_ITERS and not f.last.terminal
    info = f.last.scalars["info"]
    assert (info.anorm, info.acond) == (0.0, 0.0)


def test_singular_consistent_system_converges():
    """a zero row and column with b zero there: the Krylov space never sees the null vector"""
    dtype = np.float64
    n, rp, ci, va, b = MM.singular_kkt(40, 20, dtype)
    prod = _product(rp, ci, va)
    last = MM.minres_model(prod, b, None, None, 0.0, 1e-10, 400, dtype).last
    assert last.status == KM.CONVERGED and last.x[n - 1] == 0
    A = MM.dense_of(n, rp, ci, va)
    assert np.linalg.matrix_rank(A) == n - 1
    assert _true_residual(A, b, last.x, 1.0) <= 1e-10 * float(last.b_norm) + MM.residual_gap(dtype, 2.1, last.x, b)


# ---- mutants: the model with one method replaced ----
class _CsSign(MM.MinresModel):
    def new_cs(self, gbar, gamma):
        return -gbar / gamma


class _FirstCsSign(MM.MinresModel):
    def first_cs(self):
        return np.float64(1.0)


class _EpsDeltaSwapped(MM.MinresModel):
    def new_w(self, v, oldeps, w1, delta, w2, gamma):
        return super().new_w(v, delta, w1, oldeps, w2, gamma)


class _NoShift(MM.MinresModel):
    def y_prime(self, q, v, r1, shift, beta, oldb, k):
        return super().y_prime(q, v, r1, 0.0, beta, oldb, k)


class _NoShiftAtTheStart(MM.MinresModel):
    def start_r(self, r, x, shift):
        return r


class _RNotRotated(MM.MinresModel):
    def rotate_r(self, r1, r2, y):
        return (r2 if r1 is None else r1), y


class _BetaBeforeZ(MM.MinresModel):
    def beta_of(self, r2, z):
        return self.dot("r.r", r2, r2)


class _StopOnThe2Norm(MM.MinresModel):
    def stop_norm(self, bnorm, b):
        return np.sqrt(self.dot("b.b", b, b))


def _first_difference(mutant, dtype, pre, shift, rtol=0.0, steps=3):
    n, _, rp, ci, va = KM.banded("spd", 129, dtype) if shift else MM.kkt(44, 22, dtype)
    prod = _product(rp, ci, va)
    b, x0, minv = KM.inputs(n, dtype)
    for k in range(steps + 1):
        want = MM.MinresModel(prod, dtype).run(b, x0, minv if pre else None, shift, rtol, k).at(k)
        got = mutant(prod, dtype).run(b, x0, minv if pre else None, shift, rtol, k).at(k)
        msg = MM.compare(got, got.scalars["info"], want)
        if msg:
            return k, msg
    return None, ""


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("mutant,pre,shift", [(_CsSign, False, 0.0), (_FirstCsSign, False, 0.0), (_EpsDeltaSwapped, False, 0.0), (_EpsDeltaSwapped, True, 2.0),
                                              (_NoShift, False, 2.0), (_NoShiftAtTheStart, False, 2.0), (_RNotRotated, False, 0.0), (_BetaBeforeZ, True, 0.0)],
                         ids=["cs-sign", "first-cs-sign", "oldeps-delta-swapped", "oldeps-delta-swapped-shifted", "no-shift", "no-shift-at-the-start", "r-not-rotated",
                              "beta-before-z"])
def test_compare_rejects_the_mutant_within_three_steps(mutant, pre, shift, prec):
    k, msg = _first_difference(mutant, _dtype(prec), pre, shift)
    print(f"{mutant.__name__} {prec}: rejected at max_iters = {k}: {msg}")
    assert k is not None and k <= 3, (mutant.__name__, k)


def test_compare_rejects_a_stop_test_on_the_wrong_norm():
    """an rtol between rnorm / ||b||_M^-1 and rnorm / ||b||_2 of step 2: one of the model and the mutant stops there, the other goes on"""
    dtype = np.float64
    n, _, rp, ci, va = MM.kkt(44, 22, dtype)
    prod = _product(rp, ci, va)
    b, x0, minv = KM.inputs(n, dtype)
    e = MM.MinresModel(prod, dtype).run(b, x0, minv, 0.0, 0.0, 2).at(2)
    b2 = float(np.linalg.norm(b))
    assert abs(float(e.b_norm) / b2 - 1) > 0.01
    rtol = float(e.residual_norm) / np.sqrt(float(e.b_norm) * b2)
    k, msg = _first_difference(_StopOnThe2Norm, dtype, True, 0.0, rtol)
    assert k is not None and k <= 3, (k, msg)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_system_of_the_layout_test_is_indefinite_and_converges(prec):
    """minres_model.banded_indefinite(2500), the system of test_gpu_minres.test_every_layout_against_the_model"""
    dtype = _dtype(prec)
    n, _, rp, ci, va = MM.banded_indefinite(2500, dtype)
    A = MM.dense_of(n, rp, ci, va.astype(np.float64))
    assert np.array_equal(A, A.T)
    ev = np.linalg.eigvalsh(A)
    assert (ev < -0.4).sum() == n // 2 and (ev > 0.4).sum() == n - n // 2 and np.abs(ev).max() < 1.6, (ev.min(), ev.max(), np.abs(ev).min())
    b, x0, minv = KM.inputs(n, dtype)
    for pre, start, shift in ((None, None, 0.0), (minv, x0, 0.25)):
        full = MM.MinresModel(_product(rp, ci, va), dtype).run(b, start, pre, shift, rtol=RTOL[dtype], max_iters=400)
        assert full.last.terminal and full.last.status == KM.CONVERGED and 3 < len(full.steps) < 200, (shift, full.last, len(full.steps))
