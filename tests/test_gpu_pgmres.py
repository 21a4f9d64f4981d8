"""GPU (MI355X): restarted GMRES(m) with the block-Jacobi preconditioner object -- cvr_pgmres_device / cvr_pgmres, all through the ABI (the bodies of
the tests, shared with test_gpu_pbicgstab.py: tests/pkrylov_gpu.py).

  * the block_size = 1 contract: bit for bit cvr_gmres_device with minv_dev = the exported W, on every layout of cases.LAYOUTS in fp64 and fp32
    (nonsym_from_pattern of banded_sym(40000) with scaled rows), restart 4: to convergence, after 3 steps from a random start (x formed mid-cycle), and
    with check_every = 3 (x formed at a cycle's end inside a batch, and at the stop)
  * step by step against pkrylov_model.PGmres on the exported W, restart 3 and 5: every max_iters = k up to the model's terminal step, with the
    handle's own cvr_spmv_device as the model's product; the same bits for check_every = 1, 3 and max_iters, for arrays off the 16-byte grid and from
    the host twin; spmv_count = 1 + the steps + the restarts enqueued
  * the benefit: an exactly block-diagonal nonsymmetric matrix (blocks of condition 1e3) is solved within 2 steps, true residual (the oracle's CSR loop
    in fp64) within 2 * rtol, where the plain solver is still going after 8
  * the stop states (the lucky breakdown among them), the error returns with real objects, an object shared by two handles, and cvr_gmres_device on the
    same handle afterwards"""
import numpy as np
import pytest

import cases as K
import cvr_amd
import krylov_model as KM
import pkrylov_gpu as G
from cvr_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.LAYOUTS))
def test_block_size_one_is_gmres_with_the_exported_diagonal(layout, prec):
    G.check_block_size_one(G.Kind(4), layout, prec)


@pytest.mark.parametrize("m", [3, 5])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", [(250, 3), (1000, 8), (4099, 32)])
def test_step_by_step_against_the_model(n, bs, prec, m):
    G.check_step_by_step(G.Kind(m), n, bs, prec)


def test_block_diagonal_system_is_solved_within_two_steps():
    G.check_block_diagonal(G.Kind(30))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    G.check_stop_states(G.Kind(5), prec)


def test_errors_with_real_objects():
    G.check_errors(G.Kind(5))
    # restart out of range, with real objects
    n = 250
    _, _, rp, ci, va = KM.banded("nonsym", n, np.float64)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    P = capi.Precond.block_jacobi(rp, ci, va, 3)
    try:
        for restart in (0, capi.GMRES_MAX_RESTART + 1):
            with pytest.raises(capi.CvrError) as e:
                G.Kind(restart).solve(A, P, np.ones(n), rtol=1e-8, max_iters=3)
            assert e.value.code == capi.ERR_INVALID and "restart" in str(e.value)
    finally:
        P.close()
        A.close()


def test_device_mismatch():
    G.check_device_mismatch(G.Kind(5))


def test_one_object_two_handles():
    G.check_one_object_two_handles(G.Kind(5))
