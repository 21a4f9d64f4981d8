"""The numpy models of cvr_pbicgstab_device and cvr_pgmres_device (tests/pkrylov_model.py) on the CPU: that they are the diagonal solvers' models when
the blocks are single values, that block-Jacobi does for a nonsymmetric block-diagonal system what it is for, and that the trajectory comparison the
GPU tests use rejects an x formed from a u rounded to T, or from a block sum in the wrong order."""
import numpy as np
import pytest

import krylov_model as KM
import pkrylov_model as PK
import precond_model as PM
from cvr_amd import synth
from gmres_model import GmresModel

RTOL = {np.float64: 1e-10, np.float32: 1e-4}


def _same(a, b):
    assert len(a.steps) == len(b.steps), (len(a.steps), len(b.steps))
    for k, (s, t) in enumerate(zip(a.steps, b.steps)):
        assert KM.compare(s, t) == "", (k, KM.compare(s, t))
        assert s.terminal == t.terminal


def _banded250(dtype):
    n, _, rp, ci, va = KM.banded("nonsym", 250, dtype)
    rng = np.random.default_rng(5)
    scale = (0.5 + 1.5 * rng.random(n))[np.repeat(np.arange(n), np.diff(rp))]          # rows scaled: the diagonal is not 1
    va = (va.astype(np.float64) * scale).astype(dtype)
    return n, rp, ci, va, PM.host_product(n, rp, ci, va, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_block_size_one_is_the_diagonal_model(dtype):
    n, rp, ci, va, prod = _banded250(dtype)
    b, x0, _ = KM.inputs(n, dtype)
    W = PM.inverse_blocks(rp, ci, va, 1, dtype)
    assert W.shape == (n, 1, 1) and not np.array_equal(W.reshape(-1), np.ones(n, dtype=dtype))
    for start in (None, x0):
        for rtol, iters in ((0.0, 8), (RTOL[dtype], 60)):
            got = PK.PBicgstab(prod, dtype, W, 1).run(b, start, rtol=rtol, max_iters=iters)
            ref = KM.BicgstabModel(prod, dtype).run(b, start, W.reshape(-1), rtol=rtol, max_iters=iters)
            _same(got, ref)
            got = PK.PGmres(prod, dtype, W, 1, restart=3).run(b, start, rtol=rtol, max_iters=iters)
            gref = GmresModel(prod, dtype, restart=3).run(b, start, W.reshape(-1), rtol=rtol, max_iters=iters)
            _same(got, gref)
            assert gref.last.iterations >= 7          # (across two restarts at least)
    assert ref.last.terminal and ref.last.status == KM.CONVERGED and ref.last.iterations > 2
    assert gref.last.terminal and gref.last.status == KM.CONVERGED


def _block_diag_case(n, bs, dtype=np.float64):
    _, _, rp, ci, va = synth.block_diag_nonsym(n, bs, cond=1e3, dtype=dtype)
    return rp, ci, va, PM.host_product(n, rp, ci, va, dtype), synth.x_rand(n).astype(dtype)


def test_block_jacobi_solves_a_nonsymmetric_block_diagonal_system_at_once():
    """n = 96 in 12 blocks of 8 with condition 1e3 each: M^-1 A = I up to rounding, so both models are within 1e-10 after at most 2 steps; the plain
    models are not after 8"""
    n, bs, rtol = 96, 8, 1e-10
    rp, ci, va, prod, b = _block_diag_case(n, bs)
    W = PM.inverse_blocks(rp, ci, va, bs, np.float64)
    A = PM.dense_of(n, rp, ci, va)
    for name, pre, plain in (("BiCGSTAB", PK.PBicgstab(prod, np.float64, W, bs), KM.BicgstabModel(prod, np.float64)),
                             ("GMRES", PK.PGmres(prod, np.float64, W, bs), GmresModel(prod, np.float64))):
        got = pre.run(b, None, rtol=rtol, max_iters=8)
        ref = plain.run(b, None, None, rtol=rtol, max_iters=8)
        print(f"{name}: block-Jacobi {got.last.iterations} steps; plain after 8: residual / (rtol |b|) = {ref.last.residual_norm / (rtol * ref.last.b_norm):.3g}")
        assert got.last.status == KM.CONVERGED and got.last.iterations <= 2, (name, got.last)
        assert np.linalg.norm(b - A @ got.last.x) <= 2 * rtol * np.linalg.norm(b), name
        assert ref.last.status != KM.CONVERGED and ref.last.residual_norm > rtol * ref.last.b_norm, (name, ref.last)


# ---- the mutants of forming x ----
class _RoundedU(PK.PGmres):
    """u rounded to T on its way to the block sum"""

    def carry(self, u):
        return _f64_of(self.rnd(u))


class _ReversedX(PK.PGmres):
    """the block's columns added from the last one down where x is formed"""

    def xsum(self, terms):
        return PM.left_to_right(terms[..., ::-1])


def _f64_of(a):
    return np.asarray(a).astype(np.float64)


def _rejected(good, bad):
    for k in range(min(len(good.steps), len(bad.steps))):
        msg = KM.compare(bad.steps[k], good.steps[k])
        if msg:
            return k, msg
    return None


def test_compare_rejects_a_u_rounded_to_the_value_type():
    """fp32, n = 250 in blocks of 3: u has 53 bits, so T(u) differs from it in almost every element and x of step 1, the first x there is, in some"""
    dtype, bs = np.float32, 3
    n, rp, ci, va, prod = _banded250(dtype)
    W = PM.inverse_blocks(rp, ci, va, bs, dtype)
    b, x0, _ = KM.inputs(n, dtype)
    good = PK.PGmres(prod, dtype, W, bs, restart=3).run(b, x0, rtol=0.0, max_iters=4)
    bad = _RoundedU(prod, dtype, W, bs, restart=3).run(b, x0, rtol=0.0, max_iters=4)
    hit = _rejected(good, bad)
    assert hit is not None and hit[0] == 1 and "x differs" in hit[1], hit
    print("rounded u rejected at step", *hit)


def test_compare_rejects_the_reversed_block_sum():
    n, bs = 96, 8
    rp, ci, va, prod, b = _block_diag_case(n, bs)
    W = PM.inverse_blocks(rp, ci, va, bs, np.float64)
    _, x0, _ = KM.inputs(n, np.float64)
    good = PK.PGmres(prod, np.float64, W, bs, restart=3).run(b, x0, rtol=0.0, max_iters=2)
    bad = _ReversedX(prod, np.float64, W, bs, restart=3).run(b, x0, rtol=0.0, max_iters=2)
    hit = _rejected(good, bad)
    assert hit is not None and hit[0] == 1 and "x differs" in hit[1], hit
    print("reversed block sum rejected at step", *hit)
