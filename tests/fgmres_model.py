"""The recurrence of cvr_fgmres_device in numpy, written from the text of include/cvr_amd.h (not from the kernels), on gmres_model.GmresModel: the
model the flexible-GMRES tests compare the device with, value by value.

What the header fixes and this file does: everything is cvr_gmres_device's recurrence except that z_j = M_j^-1 v_j -- `apply(k, v)`, k the step (counted
from 0 over the whole call: the callback's k-th call), which returns z in the handle's type -- is KEPT for every column of the cycle, and x is formed
from those columns: per element u = +0; u = u + y_i double(Z_i), i ascending; x = T(double(x) + u).  `apply` None: z_j is v_j itself, and the run is
GmresModel's without minv, bit for bit.

`FixedFormModel` is the mutant the host test needs: the same steps, but x formed the way a solver that assumes one fixed M^-1 forms it,
x = x + M^-1 (V y) with `fixed(u)` applied to the fp64 combination of the BASIS -- wrong as soon as M_j changes from step to step."""
import numpy as np

from gmres_model import GmresModel
from krylov_model import _f64


class FgmresModel(GmresModel):
    """cvr_fgmres_device with restart = m and the per-step apply(k, v) -> z (None: the identity)"""

    def __init__(self, product, dtype, apply=None, sums="tree", restart=30):
        super().__init__(product, dtype, sums, restart)
        self.apply = apply

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        self.calls, self.Z = 0, []
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)

    def scale(self, minv, v):
        """z_j of step k = the calls so far (GmresModel asks for exactly one per step, in order), stored as column j = k mod m"""
        k = self.calls
        self.calls += 1
        if k % self.m == 0:
            self.Z = []
        z = v if self.apply is None else np.ascontiguousarray(self.apply(k, v), dtype=self.T)
        self.Z.append(z)
        return z

    def form_x(self, x, minv, R, g, V, q):
        """x from q columns of Z (q = 0: x itself)"""
        if q == 0:
            return x
        return self.rnd(_f64(x) + self.combination(self.back_substitute(R, g, q), self.Z[:q]))


class FixedFormModel(FgmresModel):
    """the same steps with x = x + fixed(V y): what right-preconditioned GMRES with one M^-1 does"""

    def __init__(self, product, dtype, apply, fixed, sums="tree", restart=30):
        super().__init__(product, dtype, apply, sums, restart)
        self.fixed = fixed

    def form_x(self, x, minv, R, g, V, q):
        if q == 0:
            return x
        return self.rnd(_f64(x) + self.fixed(self.combination(self.back_substitute(R, g, q), V[:q])))


def fgmres_model(product, b, x0=None, apply=None, restart=30, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return FgmresModel(product, dtype, apply, sums, restart).run(b, x0, rtol, max_iters)
