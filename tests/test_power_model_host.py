"""CPU: the numpy model of cvr_power_iteration (tests/power_model.py) before it meets a GPU -- that its trees are the documented ones and not the
exact sum, that the loop converges to the dominant eigenpair with the oracle's product, that on every matrix of the GPU tests' fused cases the fused
and the dense tree give different bits (so matching one of them on the GPU says which path ran), and that `power_model.compare` has teeth: every
mutant below is the model with one defect a kernel or the loop around it could have, and the comparison the GPU tests use must tell it from the model
within iters <= 4, at the smallest size where the defect can show."""
import math

import numpy as np
import pytest

import krylov_model as KM
import oraclelib as O
import power_model as PM

G = KM.GRID
SIZES = [1, 63, 64, 65, 256, 257, G - 1, G, G + 1, 2 * G + 1]


def _product(rp, ci, va):
    return lambda x: O.csr_spmv64(rp, ci, va, x)[0].astype(va.dtype)


def _chunks_of(n, rows):
    return np.arange(0, n, rows)


# ---- the sums ----
def test_trees_against_the_exact_sum():
    """|tree - fsum| <= gamma * sum |terms| with gamma = depth u / (1 - depth u), u = 2^-53 and depth the additions on the longest path
    (power_model.dense_bound: trips + 32; power_model.fused_bound: ceil(rows of a chunk / 64) + wpb + 28), at every size where the dense tree changes
    shape: below, at and above one wavefront, one workgroup, one trip of the grid, and a third trip of one value.  Neither tree is the exact sum."""
    rng = np.random.default_rng(3)
    differ = {"dense": [], "fused": []}
    for n in SIZES:
        terms = rng.standard_normal(n) * rng.standard_normal(n)
        mag, exact = float(np.abs(terms).sum()), float(math.fsum(terms.tolist()))
        rows = 100 if n <= G + 1 else 200          # (at most 1024 workgroups of 7 chunks)
        m = PM.PowerModel(None, np.float64, sums="fused", chunks=_chunks_of(n, rows), wpb=7)
        assert m.sums == "fused"
        for name, got, bound in (("dense", m.sum_dense(terms), PM.dense_bound(n)), ("fused", m.sum_step(terms), PM.fused_bound(rows, 7))):
            print(f"{name} n {n}: |tree - fsum| = {abs(got - exact) / (2.0 ** -53 * mag):.3f} x 2^-53 sum|terms|, bound {bound / 2.0 ** -53:.1f}")
            assert abs(got - exact) <= bound * mag, (name, n, got, exact)
            if got != exact:
                differ[name].append(n)
    for name, d in differ.items():
        assert d and max(d) > G, (name, d)


def test_dense_tree_is_the_documented_order():
    """against a plain loop over threads, lanes, wavefronts and partials"""
    def butterfly(v):
        v = list(v)
        for o in (32, 16, 8, 4, 2, 1):
            v = [v[l] + v[l ^ o] for l in range(64)]
        assert len(set(v)) == 1
        return v[0]

    m = PM.PowerModel(None, np.float64)
    rng = np.random.default_rng(7)
    differ = 0
    for n in (1, 63, 64, 65, 256, 257, 1025):
        terms = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        partials = [0.0] * 1024
        for blk in range(-(-n // 256)):
            s = 0.0
            for w in range(4):
                lanes = []
                for l in range(64):
                    acc, i = 0.0, blk * 256 + w * 64 + l
                    while i < n:
                        acc += terms[i]
                        i += G
                    lanes.append(acc)
                s += butterfly(lanes)
            partials[blk] = s
        lanes = []
        for t in range(64):
            acc = 0.0
            for i in range(t, 1024, 64):
                acc += partials[i]
            lanes.append(acc)
        want = butterfly(lanes)
        assert m.sum_dense(terms) == want, n
        differ += want != KM.exact_sum(terms)
    assert differ


def test_fused_tree_is_the_documented_order():
    m = PM.PowerModel(None, np.float64, sums="fused", chunks=[0, 130, 131, 300, 364, 700], wpb=4)
    rng = np.random.default_rng(8)
    n = 777
    terms = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    first = [0, 130, 131, 300, 364, 700, n]
    chunk = []
    for k in range(6):
        lanes = []
        for l in range(64):
            acc = 0.0
            for i in range(first[k] + l, first[k + 1], 64):
                acc += terms[i]
            lanes.append(acc)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
        chunk.append(lanes[0])
    cells = np.zeros(1024)
    cells[0] = (((0.0 + chunk[0]) + chunk[1]) + chunk[2]) + chunk[3]
    cells[1] = (0.0 + chunk[4]) + chunk[5]
    assert np.array_equal(m.fused_cells(terms), cells)
    assert m.sum_step(terms) == m.final(cells) != m.sum_dense(terms)


# ---- the loop ----
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_model_converges_to_the_dominant_eigenpair(prec):
    dtype = np.float64 if prec == "fp64" else np.float32
    n = 40
    n, _, rp, ci, va = PM.square([12] * n, dtype, seed=1)
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), 12), ci), va.astype(np.float64))
    w, v = np.linalg.eig(dense)
    top = int(np.argmax(np.abs(w)))
    lam_ref, v_ref = float(w[top].real), np.real(v[:, top])
    v_ref = v_ref / np.linalg.norm(v_ref) * np.sign(v_ref.sum())
    tol = 1e-12 if prec == "fp64" else 2e-6
    for sums, kw in (("dense", {}), ("exact", {}), ("fused", dict(chunks=[0, 7, 30], wpb=2))):
        r = PM.PowerModel(_product(rp, ci, va), dtype, sums=sums, **kw).run(np.ones(n, dtype=dtype), 60)
        assert abs(r.lam - lam_ref) <= tol * lam_ref and np.abs(r.x.astype(np.float64) - v_ref).max() <= 10 * tol, (sums, r.lam, lam_ref)
        assert r.x.dtype == dtype and not r.exact and abs(np.linalg.norm(r.x.astype(np.float64)) - 1) <= 10 * tol
    z = PM.PowerModel(_product(rp, ci, va), dtype).sweep(np.zeros(n, dtype=dtype), 3)
    assert all(r.lam == 0 and not r.x.any() and np.isfinite(r.x).all() for r in z)


CLAIMS = [(name, np.dtype(d).name) for name, (_, precs, _) in PM.fused_claims().items() for d in precs]


@pytest.mark.parametrize("name,prec", CLAIMS)
def test_fused_and_dense_trees_differ_on_every_fused_claim(name, prec):
    """on every matrix and start vector on which a GPU test claims that the one-launch step ran (power_model.fused_claims), with the chunks of the
    CPU mirror's planner (the GPU tests assert that the handle's exported chunks are these): the fused and the dense model differ in lambda's bits
    for some `iters` that the GPU test runs (two quotients of sums that differ can round to the same bits: not for every iters).  A device result
    equal to the fused model's for all those iters is therefore not the dense loop's."""
    dtype = np.dtype(prec).type
    opt, (n, _, rp, ci, va), x0, iters = PM.fused_claim(name, dtype)
    first, wpb = PM.mirror_chunks(opt, n, rp, ci, va)
    if name in PM.fused_cases() and PM.fused_cases()[name][2] is not None:
        assert (len(first), -(-len(first) // wpb)) == PM.fused_cases()[name][2:4]
    prod = _product(rp, ci, va)
    f = PM.PowerModel(prod, dtype, sums="fused", chunks=first, wpb=wpb)
    assert f.sums == "fused"
    ks = [k for k in iters if k > 0]
    a, b = f.sweep(x0, max(ks), ks), PM.PowerModel(prod, dtype).sweep(x0, max(ks), ks)
    differ = [k for k, p, q in zip(ks, a, b) if p.lam.tobytes() != q.lam.tobytes()]
    print(name, prec, "lambda differs at iters", differ)
    assert differ, (name, prec)


@pytest.mark.parametrize("loop", ["unfused", "fused"])
@pytest.mark.parametrize("name,scale,exact", PM.RULE)
def test_fp32_rule_cases_fall_on_the_intended_side(name, scale, exact, loop):
    """est of step 0, by the model with the oracle's product, lies on the intended side of its threshold by at least 1e-3 relative (the matrix keeps
    |A x| / |x| within 2^-8 of `scale`, which is 1 % off the threshold), and the model enters the exact mode exactly where est is out of range"""
    n = PM.RULE_N[loop]
    _, _, rp, ci, va = PM.diag_dominant(n, scale)
    prod = _product(rp, ci, va)
    kw = dict(zip(("chunks", "wpb"), PM.mirror_chunks(PM.PHASES, n, rp, ci, va)), sums="fused") if loop == "fused" else {}
    want = PM.PowerModel(prod, np.float32, **kw).sweep(PM.start_vectors(n, np.float32, PM.RULE_SEED)[0][1], 5, PM.RULE_ITERS)
    assert [w.exact for w in want] == [False, exact, exact]
    assert all(np.isfinite(w.x).all() and np.isfinite(w.lam) and abs(w.lam / scale - 1) < 2.0 ** -8 for w in want), [w.lam for w in want]
    est, edge = want[1].est, (1e15 if scale > 1 else 1e-15)
    assert abs(est / scale - 1) <= 2.0 ** -8
    assert (est > edge * (1 + 1e-3)) if scale > edge else (est < edge * (1 - 1e-3)), (name, est)
    assert exact == (not (1e-15 < est < 1e15))


def test_beyond_1024_workgroups_the_model_is_the_dense_one():
    opt, lens, nch, nwg, fused = PM.fused_cases()["smallest/1025_workgroups"]
    n, _, rp, ci, va = PM.square(lens, np.float64)
    first, _ = PM.mirror_chunks(opt, n, rp, ci, va)
    assert len(first) == nch == 1025 and not fused
    assert PM.PowerModel(None, np.float64, sums="fused", chunks=first, wpb=1).sums == "dense"


# ---- mutants ----
def _rejected(model, mutant, x0, kmax=4):
    """the iters <= kmax at which `compare` tells the mutant from the model"""
    return [k for k in range(kmax + 1) if (lambda m: PM.compare(m.x, m.lam, model.run(x0, k)))(mutant.run(x0, k)) != ""]


def _pair(cls, n, dtype, sums="dense", **kw):
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    prod = _product(rp, ci, va)
    return PM.PowerModel(prod, dtype, sums=sums, **kw), cls(prod, dtype, sums=sums, **kw)


class ThisStepsNorm(PM.PowerModel):
    def inv_of_step(self, k, yy):
        return self.inv(yy[k])


class FirstStepScaled(PM.PowerModel):
    """inv_0 from a set of partials nobody wrote (zeros) instead of 1"""
    def inv_of_step(self, k, yy):
        return self.inv(0.0) if k == 0 else self.inv(yy[k - 1])


class WrongParity(PM.PowerModel):
    """the other half of the double buffer: y.y of step k - 2"""
    def inv_of_step(self, k, yy):
        return self.inv(yy[k - 2]) if k >= 2 else PM.PowerModel.inv_of_step(self, k, yy)


class LambdaWithoutXX(PM.PowerModel):
    def lam(self, sums, iters):
        return sums[-1][0] if iters else np.float64(0.0)


class LambdaOfFirstStep(PM.PowerModel):
    def lam(self, sums, iters):
        return PM.PowerModel.lam(self, sums[:1], iters)


class NoExactLastStep(PM.PowerModel):
    def last_inv(self, k, yy):
        return self.inv_of_step(k, yy)


class Fp32Sums(PM.PowerModel):
    """the dense tree with fp32 accumulators (one trip)"""
    def sum_dense(self, t):
        t = np.asarray(t, dtype=np.float64)
        buf = np.zeros(-(-t.size // 256) * 256, dtype=np.float32)
        buf[: t.size] = t.astype(np.float32)
        w = KM.butterfly(buf.reshape(-1, 4, 64))
        part = np.zeros(1024, dtype=np.float32)
        part[: w.shape[0]] = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        acc = np.zeros(64, dtype=np.float32)
        for j in range(16):
            acc = acc + part[64 * j:64 * j + 64]
        return np.float64(KM.butterfly(acc))


class InvRoundedToT(PM.PowerModel):
    def inv(self, s):
        return np.float64(self.T(PM.PowerModel.inv(self, s)))


class DroppedLastTrip(PM.PowerModel):
    def dense_cells(self, t):
        t = np.asarray(t)
        return KM.tree_partials(t[: (t.size // G) * G] if t.size > G else t, 1)


class FourWavefrontCells(PM.PowerModel):
    def block_sum(self, w, nchunks):
        return PM.PowerModel.block_sum(self, w[:, :4], nchunks)


class NliveIsWpb(PM.PowerModel):
    """a short last workgroup waits for wavefronts that never arrive: its cell is never written"""
    def block_sum(self, w, nchunks):
        s = PM.PowerModel.block_sum(self, w, nchunks)
        if nchunks % w.shape[1]:
            s[-1] = 0.0
        return s


class RuleClosedBounds(PM.PowerModel):
    def in_range(self, est):
        return bool(est >= 1e-15 and est <= 1e15)


class RuleAtOneIteration(PM.PowerModel):
    def rule_applies(self, iters):
        return self.T is np.float32 and iters >= 1


class RuleAfterStepOne(PM.PowerModel):
    rule_step = 1


DENSE_MUTANTS = [(ThisStepsNorm, 2, np.float64), (FirstStepScaled, 2, np.float64), (WrongParity, 2, np.float64), (LambdaWithoutXX, 2, np.float64),
                 (LambdaOfFirstStep, 2, np.float64), (NoExactLastStep, 2, np.float64), (Fp32Sums, 65, np.float64), (Fp32Sums, 65, np.float32),
                 (InvRoundedToT, 2, np.float32), (DroppedLastTrip, G + 1, np.float64)]


@pytest.mark.parametrize("cls,n,dtype", DENSE_MUTANTS, ids=[f"{c.__name__}-{n}-{np.dtype(d).name}" for c, n, d in DENSE_MUTANTS])
def test_mutants_of_the_loop_are_rejected(cls, n, dtype):
    model, mutant = _pair(cls, n, dtype)
    x0 = PM.start_vectors(n, dtype)[0][1]
    bad = _rejected(model, mutant, x0, kmax=4 if n < G else 2)
    print(cls.__name__, n, "rejected at iters", bad)
    assert bad, cls.__name__
    assert _rejected(model, PM.PowerModel(model.product, dtype), x0, kmax=2) == []          # (and the model agrees with itself)


@pytest.mark.parametrize("cls", [FourWavefrontCells, NliveIsWpb])
def test_mutants_of_the_fused_tree_are_rejected(cls):
    """nine chunks of 40 rows and one of 10 with eight chunks per workgroup: a fifth wavefront, and a last workgroup of two"""
    n = 370
    model, mutant = _pair(cls, n, np.float64, sums="fused", chunks=_chunks_of(n, 40), wpb=8)
    bad = _rejected(model, mutant, PM.start_vectors(n, np.float64)[0][1])
    print(cls.__name__, "rejected at iters", bad)
    assert bad and min(bad) == 1, cls.__name__


def _column_with_norm_1e15():
    """fp32 values whose squares add up, in fp64 and in the dense tree's order, to a sum whose square root is 1e15 bit for bit: each value is the
    fp32 value at or below the root of what the squares before it leave of 1e30 (exact integer arithmetic)"""
    rest, col = 10 ** 30, []
    while rest > 0 and len(col) < 8:
        v = np.float32(math.isqrt(rest))
        while int(v) ** 2 > rest:
            v = np.nextafter(v, np.float32(0))
        if int(v) == 0:
            break
        col.append(v)
        rest -= int(v) ** 2
    return np.array(col, dtype=np.float32)


def test_mutants_of_the_fp32_rule():
    """est == 1e15 exactly (a matrix whose first column has that norm, from the start vector e_1): the rule's bounds are strict, so the exact mode
    is entered, and `<=` is told apart.  A check after step 1 instead of step 0 is told apart on a matrix scaled by 1e19.  The rule applied at
    iters == 1 too returns what the model returns -- the exact entry and the exact last step are the same x <- y / ||y|| and the same sums --, so
    no comparison of results can tell it: it costs a read-back, no bit."""
    col = _column_with_norm_1e15()
    n = len(col)
    rp, ci = np.arange(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    prod = _product(rp, ci, col)
    e1 = np.zeros(n, dtype=np.float32)
    e1[0] = 1
    model = PM.PowerModel(prod, np.float32)
    r = model.run(e1, 2)
    assert r.est == 1e15 and r.exact, (r.est, col)
    assert _rejected(model, RuleClosedBounds(prod, np.float32), e1)
    assert _rejected(model, RuleAtOneIteration(prod, np.float32), e1) == []
    n, _, rp, ci, va = PM.square([3] * 70, np.float32, scale=1e19)
    prod = _product(rp, ci, va)
    x0 = PM.start_vectors(n, np.float32)[0][1]
    model = PM.PowerModel(prod, np.float32)
    assert model.run(x0, 3).exact and np.isfinite(model.run(x0, 3).x).all()
    assert _rejected(model, RuleAfterStepOne(prod, np.float32), x0)
    assert _rejected(model, RuleAtOneIteration(prod, np.float32), x0) == []


# ---- the sharded step ----
class FirstOwner(PM.Shards):
    """of several shards that begin at row i's shard's first row -- empty ones and the owner -- the first instead of the last"""
    def owner(self, i):
        last = PM.Shards.owner(self, i)
        return np.searchsorted(self.b[: self.nparts], self.b[last], side="left")


class OwnWidthOffset(PM.Shards):
    def offset(self, p):
        return p * (self.b[p + 1] - self.b[p])


def test_shards_and_their_mutants():
    """pad / unpad are inverse, no padding slot is read, and a wrong owner (the first of several shards that begin at a row: an empty one) or a slice
    offset by the shard's own width show in one step"""
    rng = np.random.default_rng(1)
    n = 65
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    model = PM.PowerModel(None, np.float64)
    want_x, want_s = model.step(x, y, 2.5)
    for bounds, mr in (([0, 65], None), ([0, 30, 65], None), ([0, 0, 20, 20, 20, 64, 65, 65], 50), ([0, 1, 65], 70)):
        sh = PM.Shards(bounds, mr)
        padded = sh.pad(y)
        assert padded.size == sh.nparts * sh.max_rows and np.isnan(padded).sum() == padded.size - n
        assert sh.unpad(padded).tobytes() == y.tobytes()
        gx, gs = PM.sharded_step(model, sh, x, padded, 2.5)
        assert gx.tobytes() == want_x.tobytes() and gs == want_s
    for cls, bounds in ((FirstOwner, [0, 20, 20, 65]), (OwnWidthOffset, [0, 45, 65])):
        sh = cls(bounds)
        gx, gs = PM.sharded_step(model, sh, x, PM.Shards(bounds).pad(y), 2.5)
        assert gx.tobytes() != want_x.tobytes() and gs != want_s, cls.__name__
