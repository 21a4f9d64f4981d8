"""The numpy model of the block-Jacobi preconditioner and of cvr_pcg_device (tests/precond_model.py) on the CPU: that it is cvr_cg_device's model
when the blocks are single values, that block-Jacobi does what it is for, and that the trajectory comparison the GPU tests use rejects an apply
that sums from +0 or in the wrong order."""
import os

import numpy as np
import pytest

import krylov_model as KM
import precond_model as PM
from cvr_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _sym250(dtype):
    z = np.load(os.path.join(GOLD, "sym250_real.npz"))
    _, num_rows, num_cols = (int(v) for v in z["dims"])
    assert num_rows == num_cols
    n = num_rows + 1          # (the reference loader's arrays, read literally)
    return synth.spd_from_pattern(n, z["csr_rowptr"].astype(np.int64), z["csr_col"], dtype=dtype)


def _same(a, b):
    assert len(a.steps) == len(b.steps), (len(a.steps), len(b.steps))
    for k, (s, t) in enumerate(zip(a.steps, b.steps)):
        assert KM.compare(s, t) == "", (k, KM.compare(s, t))
        assert s.terminal == t.terminal


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_block_size_one_is_the_diagonal_model(dtype):
    n, _, rp, ci, va = _sym250(dtype)
    prod = PM.host_product(n, rp, ci, va, dtype)
    b, x0, _ = KM.inputs(n, dtype)
    W = PM.inverse_blocks(rp, ci, va, 1, dtype)
    assert W.shape == (n, 1, 1)
    for start in (None, x0):
        for rtol, iters in ((0.0, 6), (1e-10 if dtype == np.float64 else 1e-4, 60)):
            got = PM.Pcg(prod, dtype, W, 1).run(b, start, rtol=rtol, max_iters=iters)
            ref = KM.CgModel(prod, dtype).run(b, start, W.reshape(-1), rtol=rtol, max_iters=iters)
            _same(got, ref)
    assert ref.last.terminal and ref.last.status == KM.CONVERGED and ref.last.iterations > 2


def test_blocks_of_duplicates_outside_entries_and_the_short_last_block():
    # 5 x 5, bs = 2: row 0 holds (0,0) twice and (0,3) outside its block; the last block has one row
    rp = np.array([0, 4, 6, 7, 9, 10])
    ci = np.array([0, 1, 0, 3, 0, 1, 2, 2, 3, 4], dtype=np.int32)
    va = np.array([1e16, 2.0, 1.0, 9.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    B = PM.blocks_of(rp, ci, va, 2)
    assert B.shape == (3, 2, 2)
    assert np.array_equal(B[0], [[1e16 + 1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(B[1], [[5.0, 0.0], [6.0, 7.0]])
    assert np.array_equal(B[2], [[8.0, 0.0], [0.0, 1.0]])
    r = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    z = PM.apply(B, r, 2, np.float64)
    assert np.array_equal(z, [(1e16 + 1.0) * 1 + 4.0, 3.0 + 8.0, 15.0, 18.0 + 28.0, 40.0])


def _block_diag_case(n, bs, dtype=np.float64):
    _, _, rp, ci, va = synth.block_diag_spd(n, bs, cond=1e3, dtype=dtype)
    prod = PM.host_product(n, rp, ci, va, dtype)
    b = synth.x_rand(n).astype(dtype)
    return rp, ci, va, prod, b


def test_block_jacobi_solves_a_block_diagonal_system_at_once():
    """n = 96 in 12 blocks of 8 with condition 1e3 each: M^-1 A = I up to rounding, so the model is within 1e-10 after at most 2 steps; plain CG in the
    same model needs more than 8 (on the CPU: 1 step with block-Jacobi, 141 without)"""
    n, bs, rtol = 96, 8, 1e-10
    rp, ci, va, prod, b = _block_diag_case(n, bs)
    kappa = [np.linalg.cond(B) for B in PM.blocks_of(rp, ci, va, bs)]
    assert 0.99e3 <= min(kappa) and max(kappa) <= 1.01e3, (min(kappa), max(kappa))
    W = PM.inverse_blocks(rp, ci, va, bs, np.float64)
    pre = PM.Pcg(prod, np.float64, W, bs).run(b, None, rtol=rtol, max_iters=400)
    plain = KM.CgModel(prod, np.float64).run(b, None, None, rtol=rtol, max_iters=400)
    print(f"block-Jacobi: {pre.last.iterations} steps, plain CG: {plain.last.iterations} steps")
    assert pre.last.status == KM.CONVERGED and pre.last.iterations <= 2
    assert plain.last.status == KM.CONVERGED and plain.last.iterations > 8
    y = PM.dense_of(n, rp, ci, va) @ pre.last.x.astype(np.float64)
    assert np.linalg.norm(b - y) <= 2 * rtol * np.linalg.norm(b)


def test_blocks_of_adds_duplicates_in_csr_order():
    """(0, 1) three times: 1e16, -1e16, 1 is 1 in that order and 0 in the reverse (1 - 1e16 rounds to -1e16)"""
    rp = np.array([0, 4, 5])
    ci = np.array([0, 1, 1, 1, 1], dtype=np.int32)
    B = PM.blocks_of(rp, ci, np.array([2.0, 1e16, -1e16, 1.0, 2.0]), 2)
    assert np.array_equal(B[0], [[2.0, 1.0], [0.0, 2.0]])
    B = PM.blocks_of(rp, ci, np.array([2.0, 1.0, -1e16, 1e16, 2.0]), 2)
    assert np.array_equal(B[0], [[2.0, 0.0], [0.0, 2.0]])


# ---- the mutants ----
class _FromZero(PM.Pcg):
    """the sum started from +0 in place of from t_0"""

    def zsum(self, terms):
        s = np.zeros(terms.shape[:-1])
        for j in range(terms.shape[-1]):
            s = s + terms[..., j]
        return s


class _Reversed(PM.Pcg):
    """the terms added from the last column down"""

    def zsum(self, terms):
        return PM.left_to_right(terms[..., ::-1])


def _rejected(good, bad):
    for k in range(min(len(good.steps), len(bad.steps))):
        msg = KM.compare(bad.steps[k], good.steps[k])
        if msg:
            return k, msg
    return None


def test_compare_rejects_a_sum_from_plus_zero():
    """blocks (2 -1; -1 2) have an inverse without a negative entry; b = -0 and x0 = -0 in block 0 give r = -0 there (the product adds from +0), so both
    terms of z_0 are -0: z_0 = -0, and x_0 = T(-0 + alpha * -0) = -0 after a step.  Started from +0 the sum is +0, and so is x_0."""
    n, bs = 8, 2
    rp = np.arange(0, 2 * n + 1, 2)
    ci = np.array([c for k in range(n // 2) for c in (2 * k, 2 * k + 1, 2 * k, 2 * k + 1)], dtype=np.int32)
    scale = np.repeat(1.0 + np.arange(n // 2), 4)
    va = np.tile([2.0, -1.0, -1.0, 2.0], n // 2) * scale
    prod = PM.host_product(n, rp, ci, va, np.float64)
    W = PM.inverse_blocks(rp, ci, va, bs, np.float64)
    assert (W[0] > 0).all()
    b = np.array([-0.0, -0.0, 1.0, -2.0, 0.5, 3.0, -1.5, 0.25])
    x0 = np.array([-0.0, -0.0, 0.3, 0.1, -0.7, 0.2, 0.9, -0.4])
    good = PM.Pcg(prod, np.float64, W, bs).run(b, x0, rtol=0.0, max_iters=2)
    assert np.signbit(good.at(1).x[0]) and good.at(1).x[0] == 0 and good.at(1).iterations == 1
    bad = _FromZero(prod, np.float64, W, bs).run(b, x0, rtol=0.0, max_iters=2)
    hit = _rejected(good, bad)
    assert hit is not None and hit[0] == 1, hit
    print("sum from +0 rejected at step", *hit)
    assert not np.signbit(bad.at(1).x[0])


def test_compare_rejects_the_reversed_order():
    n, bs = 96, 8
    rp, ci, va, prod, b = _block_diag_case(n, bs)
    W = PM.inverse_blocks(rp, ci, va, bs, np.float64)
    good = PM.Pcg(prod, np.float64, W, bs).run(b, None, rtol=0.0, max_iters=2)
    bad = _Reversed(prod, np.float64, W, bs).run(b, None, rtol=0.0, max_iters=2)
    hit = _rejected(good, bad)
    assert hit is not None and hit[0] <= 1, hit
    print("reversed order rejected at step", *hit)
