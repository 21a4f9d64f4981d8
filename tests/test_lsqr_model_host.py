"""CPU: the numpy model of cvr_lsqr_device (tests/lsqr_model.py) before it meets a GPU -- that the recurrence of include/cvr_amd.h, with its rounding
points and its unnormalised u^, solves least-squares problems of every shape to the accuracy its stop tests promise, that it takes the steps scipy's
lsqr takes, and that the comparison the GPU tests use has teeth: every mutant below is the model with one method replaced, and `compare` must tell it
from the model within two steps.

The bounds, with M = [A; damp I], x* = the solution of least norm of min ||[b; 0] - M x|| (numpy.linalg.lstsq; every run starts from x0 = 0, from
where LSQR stays in the row space of A and so converges to that one), sigma = the smallest singular value of M above max(m, n) eps sigma_max:
  * a test-1 stop says ||r|| <= rtol ||b|| for the residual r of the system it then nearly solves, so x - x* = M^+ r:  ||x - x*|| <= rtol ||b|| / sigma;
  * a test-2 stop says ||M^T r|| <= rtol ||M||_F ||r||, and x - x* = (M^T M)^+ M^T (r - r*) with M^T r* = 0:  ||x - x*|| <= rtol ||M||_F ||r_true|| / sigma^2.
No factor on top: the CPU prototype of the recurrence sat at 0.12 to 0.26 of them (DESIGN.md 5.34 has the ratios this file measures)."""
import os

import numpy as np
import pytest

import krylov_model as KM
import lsqr_model as LM
import oraclelib as O
from cvr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = {np.float64: 1e-10, np.float32: 1e-5}


def _golden_rect():
    m = capi.load_mm(os.path.join(ROOT, "tests", "golden", "mtx", "rect64x300_int.mtx"), capi.MM_STRICT)
    return m["nrows"], m["ncols"], m["row_ptr"].astype(np.int64), m["col_idx"].astype(np.int32), m["vals"]


def _matrix(name, dtype):
    if name == "301x67":
        return LM.rect_sparse(301, 67, dtype)
    if name == "67x301":
        return LM.rect_sparse(67, 301, dtype)
    m, n, rp, ci, va = _golden_rect()
    va = va.astype(dtype)
    return (m, n, rp, ci, va) if name == "rect64x300_int" else LM.transpose_csr(m, n, rp, ci, va)


def _products(m, n, rp, ci, va):
    _, _, rpt, cit, vat = LM.transpose_csr(m, n, rp, ci, va)
    return (lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)), (lambda y: O.csr_spmv64(rpt, cit, vat, y)[0].astype(va.dtype))


NAMES = ["301x67", "67x301", "rect64x300_int", "rect64x300_int^T"]
_ref_cache = {}


def _reference(name, dtype, consistent, damp):
    """(matrix, products, b, x*, sigma, ||M||_F, M), computed once per case and left unchanged"""
    key = (name, dtype, consistent, damp)
    if key not in _ref_cache:
        m, n, rp, ci, va = _matrix(name, dtype)
        b, _ = LM.inputs(m, n, rp, ci, va, dtype, consistent)
        A = LM.dense_of(m, n, rp, ci, va)
        M = np.vstack([A, damp * np.eye(n)]) if damp else A
        rhs = np.concatenate([b.astype(np.float64), np.zeros(n)]) if damp else b.astype(np.float64)
        xs = np.linalg.lstsq(M, rhs, rcond=None)[0]
        sv = np.linalg.svd(M, compute_uv=False)
        sigma = sv[sv > max(M.shape) * np.finfo(np.float64).eps * sv[0]].min()
        _ref_cache[key] = ((m, n, rp, ci, va), _products(m, n, rp, ci, va), b, xs, sigma, np.linalg.norm(M), M, rhs)
    return _ref_cache[key]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("name", NAMES)
def test_model_solves_least_squares_within_the_bound_of_its_stop_test(name, consistent, damp, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    (m, n, *_), (prod, prod_t), b, xs, sigma, fro, M, rhs = _reference(name, dtype, consistent, damp)
    tr = LM.lsqr_model(prod, prod_t, b, None, damp=damp, rtol=rtol, max_iters=400, dtype=dtype)
    last = tr.last
    info = last.scalars["info"]
    assert last.terminal and last.status == KM.CONVERGED and info.stop_test in (1, 2), (last, info)
    assert last.x.dtype == dtype and last.x.shape == (n,) and len(tr.steps) == last.iterations + 1
    err = np.linalg.norm(last.x.astype(np.float64) - xs)
    r_true = np.linalg.norm(rhs - M @ last.x.astype(np.float64))
    bound = rtol * np.linalg.norm(b.astype(np.float64)) / sigma if info.stop_test == 1 else rtol * fro * r_true / sigma ** 2
    print(f"{name} {'consistent' if consistent else 'inconsistent'} damp {damp} {prec}: {last.iterations} steps, test {info.stop_test}, "
          f"|x - x*| / bound = {err / bound:.3g} (sigma {sigma:.3g}, |M|_F {fro:.3g}, anorm {info.anorm:.3g})")
    assert err <= bound, (err, bound, err / bound)
    # the estimates the stop tests use are what they estimate: rnorm the residual of the damped system, anorm below ||M||_F times sqrt(steps)
    assert abs(last.residual_norm - r_true) <= 1e-3 * r_true + 10 * rtol * last.b_norm
    assert info.anorm <= fro * np.sqrt(last.iterations) * (1 + 1e-6)
    # the entries before the stop are those of a run that never stops
    free = LM.lsqr_model(prod, prod_t, b, None, damp=damp, rtol=0.0, max_iters=min(3, last.iterations - 1), dtype=dtype)
    for k in range(len(free.steps)):
        assert LM.compare(free.at(k), free.at(k).scalars["info"], tr.at(k)) == "", k


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("name", NAMES[:2])
def test_step_count_against_scipy(name, consistent, damp, prec):
    sla = pytest.importorskip("scipy.sparse.linalg")
    import scipy.sparse as sp
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    (m, n, rp, ci, va), (prod, prod_t), b, *_ = _reference(name, dtype, consistent, damp)
    A = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(m, n))
    ref = sla.lsqr(A, b.astype(np.float64), damp=damp, atol=rtol, btol=rtol, conlim=0, iter_lim=400)
    tr = LM.lsqr_model(prod, prod_t, b, None, damp=damp, rtol=rtol, max_iters=400, dtype=dtype)
    print(f"{name} {'consistent' if consistent else 'inconsistent'} damp {damp} {prec}: model {tr.last.iterations} steps, scipy {ref[2]} (istop {ref[1]})")
    assert ref[1] in (1, 2) and tr.last.status == KM.CONVERGED
    assert abs(tr.last.iterations - ref[2]) <= 2, (tr.last.iterations, ref[2])


def test_stop_rules_of_the_start():
    dtype = np.float64
    m, n, rp, ci, va = LM.rect_sparse(7, 3, dtype)
    prod, prod_t = _products(m, n, rp, ci, va)
    b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
    z = LM.lsqr_model(prod, prod_t, np.zeros(m), x0, rtol=1e-10).last          # b.b == 0: x = 0 whatever the start
    assert (z.status, z.iterations, z.terminal, z.residual_norm, z.scalars["info"].stop_test) == (KM.CONVERGED, 0, True, 0.0, 0) and not z.x.any()
    # a start that solves the system: beta <= rtol bnorm, test 1, x untouched
    bc, _ = LM.inputs(m, n, rp, ci, va, dtype, True)
    solved = LM.lsqr_model(prod, prod_t, bc, None, rtol=1e-14, max_iters=50).last
    assert solved.status == KM.CONVERGED
    s = LM.lsqr_model(prod, prod_t, bc, solved.x, rtol=1e-10).last
    assert (s.status, s.iterations, s.scalars["info"].stop_test) == (KM.CONVERGED, 0, 1) and np.array_equal(s.x, solved.x)
    # A^T r0 == 0: b orthogonal to the range of A (its first rows empty, b there alone): alpha == 0, test 2
    rp2 = np.concatenate([[0, 0], rp[2:] - rp[2]]).astype(np.int64)
    prod2, prod2_t = _products(m, n, rp2, ci[rp[2]:], va[rp[2]:])
    e = np.zeros(m)
    e[0] = 3.0
    t = LM.lsqr_model(prod2, prod2_t, e, None, rtol=1e-10).last
    assert (t.status, t.iterations, t.scalars["info"].stop_test, t.residual_norm) == (KM.CONVERGED, 0, 2, 3.0) and not t.x.any()
    # NaN in b: breakdown with x untouched
    bn = b.copy()
    bn[1] = np.nan
    q = LM.lsqr_model(prod, prod_t, bn, x0, rtol=1e-10).last
    assert (q.status, q.iterations, q.terminal) == (KM.BREAKDOWN, 0, True) and np.array_equal(q.x, x0)
    # max_iters = 0 forms the start only
    f = LM.lsqr_model(prod, prod_t, b, x0, rtol=0.0, max_iters=0)
    assert len(f.steps) == 1 and f.last.status == KM.MAX_ITERS and not f.last.terminal


# ---- mutants: the model with one method replaced ----
class _NormalisedU(LM.LsqrModel):
    """the recurrence of a normalised u applied to the unnormalised one: u^ = q - alpha u^"""

    def next_u(self, q, u, alpha, beta):
        return self.rnd(KM._f64(q) - alpha * KM._f64(u))


class _RhobarSign(LM.LsqrModel):
    def new_rhobar(self, c, alpha):
        return c * alpha


class _AnormWithoutDamp(LM.LsqrModel):
    def anorm2(self, anorm2, alpha, beta, damp):
        return anorm2 + (alpha * alpha + beta * beta)


class _Test2WithoutAnorm(LM.LsqrModel):
    def test2(self, arnorm, rtol, anorm, rnorm):
        return bool(arnorm <= np.float64(rtol) * rnorm)


class _WSign(LM.LsqrModel):
    def update_w(self, v, t2, w):
        return self.rnd(KM._f64(v) + t2 * KM._f64(w))


def _first_difference(mutant, dtype, damp, rtol, steps=2, shape=(301, 67)):
    m, n, rp, ci, va = LM.rect_sparse(*shape, dtype)
    prod, prod_t = _products(m, n, rp, ci, va)
    b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
    for k in range(steps + 1):
        want = LM.LsqrModel(prod, prod_t, dtype).run(b, x0, damp, rtol, k).at(k)
        got = mutant(prod, prod_t, dtype).run(b, x0, damp, rtol, k).at(k)
        msg = LM.compare(got, got.scalars["info"], want)
        if msg:
            return k, msg
    return None, ""


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("mutant,damp", [(_NormalisedU, 0.0), (_RhobarSign, 0.0), (_RhobarSign, 0.5), (_AnormWithoutDamp, 0.5), (_WSign, 0.0)],
                         ids=["normalised-u", "rhobar-sign", "rhobar-sign-damped", "anorm-without-damp", "w-sign"])
def test_compare_rejects_the_mutant_within_two_steps(mutant, damp, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    k, msg = _first_difference(mutant, dtype, damp, 0.0)
    print(f"{mutant.__name__} {prec}: rejected at max_iters = {k}: {msg}")
    assert k is not None and k <= 2, (mutant.__name__, k)


def test_compare_rejects_test_2_without_anorm():
    """an rtol between arnorm / (anorm rnorm) and arnorm / rnorm of step 1 (anorm > 1 there): the model stops by test 2, the mutant goes on"""
    dtype = np.float64
    m, n, rp, ci, va = LM.rect_sparse(301, 67, dtype)
    prod, prod_t = _products(m, n, rp, ci, va)
    b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
    e = LM.LsqrModel(prod, prod_t, dtype).run(b, x0, 0.0, 0.0, 1).at(1)
    info = e.scalars["info"]
    assert info.anorm > 1.5
    rtol = float(info.arnorm / (info.anorm * e.residual_norm)) * 1.2
    assert rtol * info.anorm * e.residual_norm > info.arnorm > rtol * e.residual_norm and e.residual_norm > rtol * e.b_norm
    want = LM.LsqrModel(prod, prod_t, dtype).run(b, x0, 0.0, rtol, 2)
    assert want.last.terminal and want.last.iterations == 1 and want.last.scalars["info"].stop_test == 2
    k, msg = _first_difference(_Test2WithoutAnorm, dtype, 0.0, rtol)
    assert k is not None and k <= 2, (k, msg)


def test_generators_are_what_they_say():
    for shape in ((301, 67), (67, 301), (5, 1), (1, 5), (3, 3)):
        for dtype in (np.float64, np.float32):
            m, n, rp, ci, va = LM.rect_sparse(*shape, dtype)
            assert (m, n) == shape and va.dtype == dtype and len(rp) == m + 1 and rp[-1] == len(ci) == len(va)
            for r in range(m):
                assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) and rp[r + 1] > rp[r]
            assert ci.min() >= 0 and ci.max() < n
            A = LM.dense_of(m, n, rp, ci, va)
            assert np.linalg.matrix_rank(A) == min(m, n)
            nt, mt, rpt, cit, vat = LM.transpose_csr(m, n, rp, ci, va)
            assert np.array_equal(LM.dense_of(nt, mt, rpt, cit, vat), A.T)
            for r in range(nt):
                assert np.all(np.diff(cit[rpt[r]:rpt[r + 1]]) > 0)
    for m, n in ((9, 4), (5, 1), (2, 2), (12, 5)):
        _, _, rp, ci, va = LM.two_per_row(m, n, np.float64)
        A = LM.dense_of(m, n, rp, ci, va)
        assert np.linalg.matrix_rank(A) == n and ((A != 0).sum(axis=1) == (1 if n == 1 else 2)).all()
        for r in range(m):
            assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_the_system_of_the_layout_test_converges_and_cuts_rows(prec):
    """lsqr_model.rect_long, the system of test_gpu_lsqr.test_layouts_against_the_model: the model converges within that file's MAX_ITERS with numpy
    products standing in for the handles, the matrix is well conditioned, and the host planner cuts rows of A and of A^T at 16 steps per chunk"""
    dtype = np.float64 if prec == "fp64" else np.float32
    m, n, rp, ci, va = LM.rect_long(dtype)
    assert (m, n) == (701, 449)
    rows = np.repeat(np.arange(m), np.diff(rp))
    assert np.all((np.diff(ci.astype(np.int64)) > 0) | (np.diff(rows) > 0))          # sorted, no duplicates: every layout takes it
    assert np.diff(rp).max() > 256 and np.bincount(ci, minlength=n).max() > 256
    sv = np.linalg.svd(LM.dense_of(m, n, rp, ci, va.astype(np.float64)), compute_uv=False)
    assert sv[-1] > 0.5 and sv[0] / sv[-1] < 8, (sv[0], sv[-1])
    _, _, rpt, _, _ = LM.transpose_csr(m, n, rp, ci, va)
    for p in (rp, rpt):
        nzb = capi.plan_chunks(p, 16)["nz_begin"]
        assert (~np.isin(nzb[1:-1], p)).any(), "no row cut over chunks"
    prod, prod_t = _products(m, n, rp, ci, va)
    b, x0 = LM.inputs(m, n, rp, ci, va, dtype, False)
    for damp, start in ((0.0, x0), (0.5, None)):
        full = LM.LsqrModel(prod, prod_t, dtype).run(b, start, damp, rtol=RTOL[dtype], max_iters=400)
        assert full.last.terminal and full.last.status == KM.CONVERGED and 3 < len(full.steps) < 200, (damp, full.last, len(full.steps))
