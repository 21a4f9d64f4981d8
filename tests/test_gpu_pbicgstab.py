"""GPU (MI355X): BiCGSTAB with the block-Jacobi preconditioner object -- cvr_pbicgstab_device / cvr_pbicgstab, all through the ABI (the bodies of the
tests, shared with test_gpu_pgmres.py: tests/pkrylov_gpu.py).

  * the block_size = 1 contract: bit for bit cvr_bicgstab_device with minv_dev = the exported W, on every layout of cases.LAYOUTS in fp64 and fp32
    (nonsym_from_pattern of banded_sym(40000) with scaled rows), to convergence, after 3 steps from a random start, and with check_every = 3
  * step by step against pkrylov_model.PBicgstab on the exported W: every max_iters = k up to the model's terminal step, with the handle's own
    cvr_spmv_device as the model's product; the same bits for check_every = 1, 3 and max_iters, for arrays off the 16-byte grid and from the host twin;
    spmv_count = 1 + 2 per step enqueued
  * the benefit: an exactly block-diagonal nonsymmetric matrix (blocks of condition 1e3) is solved within 2 steps, true residual (the oracle's CSR loop
    in fp64) within 2 * rtol, where the plain solver is still going after 8
  * the stop states (the half-step stop among them), the error returns with real objects, an object shared by two handles, and cvr_bicgstab_device on
    the same handle afterwards"""
import pytest

import cases as K
import pkrylov_gpu as G

pytestmark = pytest.mark.gpu

KIND = G.Kind()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", sorted(K.LAYOUTS))
def test_block_size_one_is_bicgstab_with_the_exported_diagonal(layout, prec):
    G.check_block_size_one(KIND, layout, prec)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,bs", [(250, 3), (1000, 8), (4099, 32)])
def test_step_by_step_against_the_model(n, bs, prec):
    G.check_step_by_step(KIND, n, bs, prec)


def test_block_diagonal_system_is_solved_within_two_steps():
    G.check_block_diagonal(KIND)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_stop_states(prec):
    G.check_stop_states(KIND, prec)


def test_errors_with_real_objects():
    G.check_errors(KIND)


def test_device_mismatch():
    G.check_device_mismatch(KIND)


def test_one_object_two_handles():
    G.check_one_object_two_handles(KIND)
