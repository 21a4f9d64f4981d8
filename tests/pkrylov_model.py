"""cvr_pbicgstab_device and cvr_pgmres_device in numpy, written from the text of include/cvr_amd.h (not from the kernels), beside krylov_model.py,
gmres_model.py and precond_model.py, whose recurrences, sums, trajectories, comparison and apply it uses.

What the header fixes and this file does: both solvers are the diagonal ones word for word with M^-1 = W of the object -- `scale`, the one place where
the base models multiply by minv, is the block apply (`precond_model.apply`: z_i = T(t_0 + t_1 + ..), left to right from t_0).  GMRES forms x from the
fp64 combination u = sum y_i double(v_i), which is never rounded to T: x_i = T(double(x_i) + (t_0 + t_1 + ..)) with t_j = double(W[i][j]) * u[k*bs + j]
(`block_sum`, the apply's order with u where the apply has double(r)).

One method per operation, so that a mutant (tests/test_pkrylov_model_host.py) is the model with one method replaced."""
import numpy as np

import krylov_model as KM
import precond_model as PM
from gmres_model import GmresModel
from krylov_model import _f64


def block_sum(W, u, bs, dtype, zsum=PM.left_to_right):
    """s_i = t_0 + t_1 + .. with t_j = double(W[i][j]) * u[k*bs + j] in fp64: W (nblocks, bs, bs) in T, u n values in fp64 (used as they are); the
    columns a short last block was completed with give no term"""
    W = np.asarray(W, dtype=np.dtype(dtype).type).astype(np.float64).reshape(-1, bs, bs)
    u = np.asarray(u, dtype=np.float64)
    n = len(u)
    full = n // bs
    out = []
    with np.errstate(all="ignore"):
        if full:
            out.append(zsum(W[:full] * u[: full * bs].reshape(full, 1, bs)).reshape(-1))
        m = n - full * bs
        if m:
            out.append(zsum(W[full, :m, :m] * u[full * bs:].reshape(1, m)).reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


class _Object:
    """what both models add: the exported blocks W (what the device holds), the block size, and the apply in place of T(minv * r)"""

    def set_object(self, W, bs):
        self.W, self.bs = np.asarray(W, dtype=self.T), int(bs)

    def zsum(self, terms):
        return PM.left_to_right(terms)

    def scale(self, minv, r):
        return PM.apply(self.W, r, self.bs, self.T, zsum=self.zsum)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


class PBicgstab(_Object, KM.BicgstabModel):
    """cvr_pbicgstab_device: cvr_bicgstab_device's recurrence with p^ = W p and s^ = W s"""

    def __init__(self, product, dtype, W, bs, sums="tree"):
        KM.BicgstabModel.__init__(self, product, dtype, sums)
        self.set_object(W, bs)


class PGmres(_Object, GmresModel):
    """cvr_pgmres_device with restart = m: cvr_gmres_device's recurrence with z_j = W v_j, and x from the fp64 u through the block sum"""

    def __init__(self, product, dtype, W, bs, sums="tree", restart=30):
        GmresModel.__init__(self, product, dtype, sums, restart)
        self.set_object(W, bs)

    def carry(self, u):
        """u on its way from the combination to the block sum: fp64, as it is"""
        return u

    def xsum(self, terms):
        return self.zsum(terms)

    def form_x(self, x, minv, R, g, V, q):
        """x from q columns of the cycle (q = 0: x itself)"""
        if q == 0:
            return x
        u = self.carry(self.combination(self.back_substitute(R, g, q), V[:q]))
        return self.rnd(_f64(x) + block_sum(self.W, u, self.bs, self.T, zsum=self.xsum))
