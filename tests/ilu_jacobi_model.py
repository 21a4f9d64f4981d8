"""The Jacobi-swept ILU(0) apply (cvr_precond_ilu0_jacobi) in numpy, written from the text of include/cvr_amd.h (not from the kernels), on top of
tests/ilu_model.py: its `factor`, `butterfly`, `default_lanes` and the sum of its `_sweep`.

The factors are ILU(0)'s; each exact triangular solve of the apply is replaced by s Jacobi sweeps on the triangular system.  With S_i(v) the sum of
row i over L's part of the row and S'_i(v) over U's part right of the diagonal -- lane e % G of G adds double(f_ij) * double(v_j) over the entries
e = 0, 1, .. in column order from +0, the lanes by the xor butterfly G/2 .. 1, exactly ilu_model._sweep's sum -- and y(0) = r as it is:
    L:  y(k)_i = T(double(r_i) - S_i(y(k-1))),   k = 1 .. s
    U:  z(0)_i = T(double(y(s)_i) / double(u_ii)),   z(k)_i = T((double(y(s)_i) - S'_i(z(k-1))) / double(u_ii)),   k = 1 .. s;   z = z(s).
A sweep reads only the vector before it, so all rows are formed at once: the loop is over the entry index e of a row, and every product and addition
is one numpy fp64 operation on the rows that have an entry e (numpy rounds each operation on its own and never fuses).

`IluJacobi` has ilu_model.Ilu's interface (rp, ci, f, G, T, apply(r, rhs_is_fp64)), so ilu_model.IluPcg, IluBicgstab and IluGmres run on it unchanged.
This file is the reference the device is compared with; nothing compares it with itself."""
import numpy as np

import ilu_model as IM

MAX_SWEEPS = 64          # include/cvr_amd.h: CVR_ILU0_MAX_SWEEPS


class _Triangle:
    """one triangle's entries by their index e within the row: per e the rows that have one, and where it lies"""

    def __init__(self, beg, cnt):
        self.n = len(beg)
        self.by_entry = []
        for e in range(int(cnt.max()) if self.n else 0):
            rows = np.flatnonzero(cnt > e)
            self.by_entry.append((rows, beg[rows] + e))

    def sums(self, f, ci, v, G):
        """S_i(v) of every row: ilu_model._sweep's s[e % G] = s[e % G] + f[q] * v[ci[q]], then its butterfly"""
        s = [np.zeros(self.n) for _ in range(G)]
        for e, (rows, q) in enumerate(self.by_entry):
            s[e % G][rows] = s[e % G][rows] + f[q] * v[ci[q]]
        return IM.butterfly(s)


class IluJacobi:
    """an object: the pattern, the factors as exported, G, the number of sweeps"""

    def __init__(self, rp, ci, f, G, dtype, sweeps):
        assert 1 <= int(sweeps) <= MAX_SWEEPS, sweeps
        self.rp, self.ci, self.f, self.G, self.T = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(f), int(G), np.dtype(dtype).type
        self.sweeps = int(sweeps)
        self.n = len(self.rp) - 1
        d = IM.diagonal_positions(self.rp, self.ci)
        self.lower = _Triangle(self.rp[:-1], d - self.rp[:-1])
        self.upper = _Triangle(d + 1, self.rp[1:] - d - 1)
        self.f64 = np.asarray(self.f, dtype=self.T).astype(np.float64)
        self.diag = self.f64[d]

    @classmethod
    def of(cls, rp, ci, va, dtype, sweeps, G=None):
        f, bad = IM.factor(rp, ci, va, dtype)
        assert bad is None, bad
        n = len(rp) - 1
        return cls(rp, ci, f, IM.default_lanes(n, int(rp[-1])) if G is None else G, dtype, sweeps)

    def _round(self, v):
        return v.astype(self.T).astype(np.float64)

    def apply(self, r, rhs_is_fp64=False):
        """z(s): r n values of T -- or of fp64, used as they are (rhs_is_fp64: GMRES's u)"""
        r = np.asarray(r, dtype=np.float64) if rhs_is_fp64 else np.asarray(r, dtype=self.T).astype(np.float64)
        with np.errstate(all="ignore"):
            y = r
            for _ in range(self.sweeps):
                y = self._round(r - self.lower.sums(self.f64, self.ci, y, self.G))
            z = self._round(y / self.diag)
            for _ in range(self.sweeps):
                z = self._round((y - self.upper.sums(self.f64, self.ci, z, self.G)) / self.diag)
        return z.astype(self.T)


def exact_sweeps(nlo, nup):
    """the least s from which the swept apply is the exact one bit for bit: after k L sweeps the rows of L-level <= k - 1 hold the exact sweep's
    values, after k U sweeps (behind z(0), which is exact on U-level 0) those of U-level <= k"""
    return max(nlo, nup - 1, 1)
