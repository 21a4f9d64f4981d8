"""CPU: the numpy model of the solvers (tests/krylov_model.py) before it meets a GPU -- that its tree is the documented one and not the exact sum,
that both recurrences converge with the oracle's product, and that `compare` has teeth: every mutant below is the model with one defect a kernel
could have, and the comparison the GPU tests use must tell it from the model within 6 steps, at the smallest size where the defect can show."""
import math

import numpy as np
import pytest

import krylov_model as KM
import oraclelib as O

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
G = KM.GRID


def _sizes(pack):
    return [1, 2, 3, 4, 5, 7, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, G * pack - 1, G * pack, G * pack + 1, 2 * G * pack + pack + 1]


_matrix = KM.banded


def _product(rp, ci, va):
    return lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)


_inputs = KM.inputs


def _true_residual(rp, ci, va, x, b):
    y, _ = O.csr_spmv64(rp, ci, va, x)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - y) / np.linalg.norm(b))


# ---- the sums ----
@pytest.mark.parametrize("pack", [2, 4])
def test_tree_against_the_exact_sum(pack):
    """|tree - exact| <= (pack * trips + 24) 2^-53 sum |terms| at every size where the tree changes shape; and the tree is not the exact sum:
    at some of these sizes the bits differ, so the bitwise tier pins an order"""
    rng = np.random.default_rng(pack)
    differ = []
    for n in _sizes(pack):
        a, c = rng.standard_normal(n), rng.standard_normal(n)
        if pack == 4:
            a, c = a.astype(np.float32), c.astype(np.float32)
        terms = a.astype(np.float64) * c.astype(np.float64)
        tree, exact = KM.tree_sum(terms, pack), KM.exact_sum(terms)
        bound = KM.sum_bound(n, pack) * float(np.abs(terms).sum())
        print(f"pack {pack} n {n}: |tree - exact| = {abs(tree - exact) / (2.0 ** -53 * np.abs(terms).sum()):.3f} x 2^-53 sum|terms|, bound {bound / (2.0 ** -53 * np.abs(terms).sum()):.0f}")
        assert abs(tree - exact) <= bound, (pack, n, tree, exact)
        if tree != exact:
            differ.append(n)
    assert differ, "the tree gave the exact sum everywhere"
    assert max(differ) > G * pack          # (and beyond one trip too)


def test_tree_is_the_documented_order():
    """against a plain loop over the threads, lanes, wavefronts and partials on a size with a second trip and a partial packet -- and the order is
    felt: with terms of very different size it is not the exact sum"""
    for pack in (2, 4):
        n = G * pack + 3 * pack + 1
        rng = np.random.default_rng(7)
        terms = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)

        def butterfly(v):
            v = list(v)
            for o in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ o] for l in range(64)]
            assert len(set(v)) == 1
            return v[0]

        def block(vals):
            s = 0.0
            for w in range(4):
                s += butterfly(vals[64 * w:64 * w + 64])
            return s
        acc = np.zeros(G)          # a thread's own sum: trip by trip, value by value
        for trip in range(2):
            for j in range(pack):
                idx = (trip * G + np.arange(G)) * pack + j
                ok = idx < n
                acc[ok] = acc[ok] + terms[idx[ok]]
        partials = [block(acc[256 * w:256 * w + 256]) for w in range(1024)]
        last = block([((0.0 + partials[t]) + partials[t + 256] + partials[t + 512]) + partials[t + 768] for t in range(256)])
        assert KM.tree_sum(terms, pack) == last
        assert last != KM.exact_sum(terms)


# ---- the recurrences ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [1, 2, 5, 513, 40001])
def test_models_converge_with_the_oracle_product(n, prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    rtol = RTOL[dtype]
    for kind, model in (("spd", KM.cg_model), ("nonsym", KM.bicgstab_model)):
        _, _, rp, ci, va = _matrix(kind, n, dtype)
        b, x0, minv = _inputs(n, dtype)
        for sums in ("tree", "exact"):
            for start, m in ((None, None), (x0, minv)):
                tr = model(_product(rp, ci, va), b, start, m, rtol=rtol, max_iters=60, dtype=dtype, sums=sums)
                last = tr.last
                assert last.terminal and last.status == KM.CONVERGED, (kind, n, prec, sums, last)
                assert last.residual_norm <= rtol * last.b_norm
                assert _true_residual(rp, ci, va, last.x, b) <= 2 * rtol, (kind, n, prec, sums)
                assert last.x.dtype == dtype and len(tr.steps) == last.iterations + 1
                # the entries before the stop are those of a run that never stops
                free = model(_product(rp, ci, va), b, start, m, rtol=0.0, max_iters=min(3, last.iterations), dtype=dtype, sums=sums)
                for k in range(min(3, last.iterations)):
                    assert KM.compare(free.at(k), tr.at(k)) == "", (kind, n, k)


def test_stop_rules():
    dtype = np.float64
    n = 5
    for kind, model in (("spd", KM.cg_model), ("nonsym", KM.bicgstab_model)):
        _, _, rp, ci, va = _matrix(kind, n, dtype)
        prod = _product(rp, ci, va)
        b, x0, _ = _inputs(n, dtype)
        z = model(prod, np.zeros(n), x0, rtol=1e-10)          # b.b == 0: x = 0 whatever the start
        assert len(z.steps) == 1 and z.last.terminal and not z.last.x.any() and (z.last.status, z.last.iterations, z.last.residual_norm, z.last.b_norm) == (KM.CONVERGED, 0, 0, 0)
        sol = model(prod, b, None, rtol=1e-12, max_iters=30).last
        assert sol.status == KM.CONVERGED
        s = model(prod, b, sol.x, rtol=1e-6)          # a start vector within the tolerance: untouched
        assert len(s.steps) == 1 and s.last.status == KM.CONVERGED and s.last.iterations == 0 and s.last.x.tobytes() == sol.x.tobytes()
        bad = b.copy()
        bad[2] = np.inf          # not finite: never converged, breakdown at step 0 with x untouched
        f = model(prod, bad, x0, rtol=1e-10)
        assert [st.status for st in f.steps] == [KM.MAX_ITERS, KM.BREAKDOWN] and f.last.iterations == 0 and f.last.x.tobytes() == x0.tobytes()
        assert f.at(5) is f.last
    # CG on -A: p.q < 0
    _, _, rp, ci, va = _matrix("spd", n, dtype)
    f = KM.cg_model(_product(rp, ci, -va), b, None, rtol=1e-10)
    assert f.last.status == KM.BREAKDOWN and f.last.iterations == 0 and not f.last.x.any()
    # n = 1: A = (1), solved exactly by one step; r.r == 0 then stops the run at rtol = 0
    _, _, rp, ci, va = _matrix("spd", 1, dtype)
    one = KM.cg_model(_product(rp, ci, va), np.array([0.3]), None, rtol=0.0)
    assert one.last.terminal and (one.last.status, one.last.iterations, one.last.residual_norm) == (KM.CONVERGED, 1, 0) and one.last.x[0] == 0.3
    # BiCGSTAB on the cyclic shift with b = e_0: r^ . v == 0 at step 0
    m = 6
    rp, ci, va = np.arange(m + 1, dtype=np.int64), ((np.arange(m) + 1) % m).astype(np.int32), np.ones(m)
    e0 = np.zeros(m)
    e0[0] = 1
    f = KM.bicgstab_model(_product(rp, ci, va), e0, None, rtol=1e-10)
    assert f.last.status == KM.BREAKDOWN and f.last.iterations == 0 and f.last.residual_norm == 1


def test_bicgstab_half_step_stop():
    """the half step fires where ||s|| is within the tolerance and the step before was not: the model says at which rtol"""
    dtype = np.float64
    n = 129
    _, _, rp, ci, va = _matrix("nonsym", n, dtype)
    b, _, _ = _inputs(n, dtype)
    free = KM.bicgstab_model(_product(rp, ci, va), b, None, rtol=0.0, max_iters=3, dtype=dtype)
    snorm, before = np.sqrt(free.steps[2].scalars["ss"]), free.steps[1].residual_norm
    assert snorm < before
    rtol = float(math.sqrt(snorm * before) / free.steps[0].b_norm)
    tr = KM.bicgstab_model(_product(rp, ci, va), b, None, rtol=rtol, max_iters=10, dtype=dtype)
    assert tr.last.scalars.get("half") and (tr.last.status, tr.last.iterations) == (KM.CONVERGED, 2) and tr.last.residual_norm == snorm
    assert KM.compare(tr.last, free.steps[2]) != ""          # x at the half step is not x of the whole step


# ---- the mutants ----
def _drop(f):
    """a model whose sums see f(terms, pack, name) instead of the terms"""
    def dot(self, name, a, b):
        t = f(self.terms(a, b), self.pack, name)
        return KM.tree_sum(t, self.pack) if len(t) else np.float64(0.0)
    return dot


def _mutant(base, **methods):
    return type("Mutant", (base,), methods)


def _fp32_sums(self, name, a, b):
    acc = np.float32(0)
    for v in (np.asarray(a, dtype=np.float32) * np.asarray(b, dtype=np.float32)):
        acc = np.float32(acc + v)
    return np.float64(acc)


def _fused(self, name, y, a, x):
    if name != "x":
        return KM.CgModel.axpy(self, name, y, a, x)
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no more bits than fp64 here"
    return (y.astype(np.longdouble) + np.longdouble(a) * x.astype(np.longdouble)).astype(self.T)


def _no_half_update(self, x, alpha, ph):
    return x.astype(np.float64)


# name -> (base model, the defect, dtype, with minv, n: the smallest size where it can show, and why)
MUTANTS = {
    "last value left out of p.q": (KM.CgModel, dict(dot=_drop(lambda t, pack, name: t[:-1] if name == "p.q" else t)), np.float64, False, 1,
                                   "n = 1: p.q is empty, 0, a breakdown"),
    "partial packet treated as empty": (KM.CgModel, dict(dot=_drop(lambda t, pack, name: t[: len(t) // pack * pack])), np.float64, False, 3,
                                        "n = pack + 1: the first size with a whole packet and a partial one (n < pack: every sum is 0, b.b too)"),
    "second trip of the packet loop skipped": (KM.CgModel, dict(dot=_drop(lambda t, pack, name: t[: KM.GRID * pack])), np.float64, False, KM.GRID * 2 + 1,
                                               "n = 262 144 * pack + 1: the first size with a second trip"),
    "beta inverted": (KM.CgModel, dict(beta=lambda self, new, old: old / new), np.float64, False, 2,
                      "n = 2: with one unknown the direction's length cancels in alpha * p"),
    "rz taken from the wrong parity": (KM.CgModel, dict(rz_of_step=lambda self, hist, k: hist[k - 1] if k else np.float64(0.0)), np.float64, False, 1,
                                       "n = 1: step 0 divides the empty slot, alpha = 0"),
    "sums accumulated in fp32 for an fp32 handle": (KM.CgModel, dict(dot=_fp32_sums), np.float32, False, 1, "n = 1: b * b rounded to fp32 is another b_norm"),
    "alpha rounded to T": (KM.CgModel, dict(alpha=lambda self, rz, pq: np.float64(np.float32(rz / pq))), np.float32, False, 3,
                           "n = 3: the first size of the banded generator whose alpha is not a power of two times a short fraction"),
    "fused x + alpha p": (KM.CgModel, dict(axpy=_fused), np.float64, False, 7, "n = 7: enough values for one to round the other way (about one in four does)"),
    "z not refreshed": (KM.CgModel, dict(refresh_z=lambda self, minv, r, z: z), np.float64, True, 2, "n = 2: with one unknown a stale z only rescales p"),
    "stop test on r.z instead of r.r": (KM.CgModel, dict(stop_sum=lambda self, rr, rz: rz), np.float64, True, 1, "n = 1: the reported norm is another one at once"),
    "BiCGSTAB: omega inverted": (KM.BicgstabModel, dict(omega=lambda self, ts, tt: tt / ts), np.float64, False, 2, "n = 2: with one unknown s is 0 after the half step"),
    "BiCGSTAB: the half-step update of x missing": (KM.BicgstabModel, dict(half_x=_no_half_update), np.float64, False, 1, "n = 1: x_1 lacks alpha p"),
    "BiCGSTAB: beta without alpha / omega": (KM.BicgstabModel, dict(beta=lambda self, rho1, rho, alpha, omega: rho1 / rho), np.float64, False, 2,
                                             "n = 2: the first size with a second direction"),
    "BiCGSTAB: r^ overwritten by r": (KM.BicgstabModel, dict(shadow=lambda self, rhat, r: r.copy()), np.float64, False, 2, "n = 2: the first size with a second step"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_compare_rejects_the_mutant(name):
    base, methods, dtype, pre, n, why = MUTANTS[name]
    kind = "spd" if base is KM.CgModel else "nonsym"
    _, _, rp, ci, va = _matrix(kind, n, dtype)
    prod = _product(rp, ci, va)
    b, x0, minv = _inputs(n, dtype)
    m = minv if pre else None
    steps = 6 if n < KM.GRID else 2
    good = base(prod, dtype).run(b, x0, m, rtol=0.0, max_iters=steps)
    bad = _mutant(base, **methods)(prod, dtype).run(b, x0, m, rtol=0.0, max_iters=steps)
    found = [(k, msg) for k in range(len(good.steps)) for msg in [KM.compare(bad.at(k) if bad.last.terminal else bad.steps[min(k, len(bad.steps) - 1)], good.steps[k])] if msg]
    assert found, f"{name}: not rejected at n = {n} within {steps} steps"
    k, msg = found[0]
    print(f"mutant '{name}' rejected at n = {n} ({why}), step {k}: {msg}")
    assert k <= 6
    # and the unmutated model equals itself
    again = base(prod, dtype).run(b, x0, m, rtol=0.0, max_iters=steps)
    assert all(KM.compare(again.at(k), good.at(k)) == "" for k in range(len(good.steps)))
