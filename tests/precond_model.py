"""The block-Jacobi preconditioner and cvr_pcg_device in numpy, written from the text of include/cvr_amd.h (not from the kernels), beside
krylov_model.py, whose sums, trajectories and comparison it uses.

What the header fixes and this file does: block k covers rows and columns k*bs .. min(n, (k+1)*bs) - 1; entry (i, j) is the fp64 sum of the CSR entries
of row i with that column in CSR order; a short last block is completed with the identity (`blocks_of`).  The inverse itself is not modelled bit for
bit -- the tests hold the exported W against numpy's inverse of `blocks_of` within the forward error bound -- but everything behind it is: the apply is
`z_i = T(t_0 + t_1 + ..)` with `t_j = double(W[i][j]) * double(r[k*bs + j])` over the columns of the block that exist, summed left to right from t_0
(`apply`), and the solver is cvr_cg_device's recurrence with that z (`Pcg`, a CgModel whose scale is the apply)."""
import numpy as np

import krylov_model as KM
from krylov_model import tree_sum  # noqa: F401  (the sums of the solver are krylov_model's)


def nblocks_of(n, bs):
    return -(-int(n) // int(bs))


def blocks_of(rp, ci, va, bs):
    """the dense diagonal blocks in fp64, shape (nblocks, bs, bs): duplicates added in CSR order from +0, entries outside the blocks ignored, the rows
    and columns a short last block lacks completed with the identity"""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    nb = nblocks_of(n, bs)
    B = np.zeros((nb, bs, bs))
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[rp[0]: rp[-1]], dtype=np.int64) if n else np.zeros(0, dtype=np.int64)
    vals = np.asarray(va[rp[0]: rp[-1]]).astype(np.float64) if n else np.zeros(0)
    inside = (cols // bs == rows // bs) & (cols >= 0) & (cols < n)
    rows, cols, vals = rows[inside], cols[inside], vals[inside]
    flat = B.reshape(-1)
    key = (rows // bs) * (bs * bs) + (rows % bs) * bs + cols % bs
    with np.errstate(all="ignore"):
        for k, v in zip(key.tolist(), vals.tolist()):          # one by one: CSR order per (i, j)
            flat[k] = flat[k] + v
    for i in range(n, nb * bs):
        B[i // bs, i % bs, i % bs] = 1.0
    return B


def left_to_right(terms):
    """terms: (..., m) fp64 -> (...): t_0 + t_1 + .. + t_(m-1), starting from t_0"""
    s = terms[..., 0]
    for j in range(1, terms.shape[-1]):
        s = s + terms[..., j]
    return s


def apply(W, r, bs, dtype, zsum=left_to_right):
    """z = M^-1 r by the header's arithmetic: W (nblocks, bs, bs) in T, r n values in T; the columns a short last block was completed with give no term"""
    T = np.dtype(dtype).type
    W = np.asarray(W, dtype=T).astype(np.float64).reshape(-1, bs, bs)
    r = np.asarray(r, dtype=T).astype(np.float64)
    n = len(r)
    full = n // bs
    out = []
    with np.errstate(all="ignore"):
        if full:
            out.append(zsum(W[:full] * r[: full * bs].reshape(full, 1, bs)).reshape(-1))
        m = n - full * bs
        if m:
            out.append(zsum(W[full, :m, :m] * r[full * bs:].reshape(1, m)).reshape(-1))
    z = np.concatenate(out) if out else np.zeros(0)
    return z.astype(T)


class Pcg(KM.CgModel):
    """cvr_pcg_device: cvr_cg_device's recurrence with z = M^-1 r.  `W`: the exported blocks (what the device holds), `bs` the block size."""

    def __init__(self, product, dtype, W, bs, sums="tree"):
        super().__init__(product, dtype, sums)
        self.W, self.bs = np.asarray(W, dtype=self.T), int(bs)

    # ---- the single operations of the header ----
    def zsum(self, terms):
        return left_to_right(terms)

    def precondition(self, r):
        return apply(self.W, r, self.bs, self.T, zsum=self.zsum)

    def scale(self, minv, r):
        """z: the apply in place of T(minv * r)"""
        return self.precondition(r)

    def start(self, b, x0, minv):
        b, x, _, r = super().start(b, x0, None)
        return b, x, self, r          # (a preconditioner is present: r.z is a sum of its own)

    def run(self, b, x0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, None, rtol, max_iters)


def dense_of(n, rp, ci, va):
    """the dense fp64 matrix of a small CSR (duplicates added)"""
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(A, (rows, np.asarray(ci[: rp[-1]], dtype=np.int64)), np.asarray(va[: rp[-1]], dtype=np.float64))
    return A


def host_product(n, rp, ci, va, dtype):
    """x -> T(A x): the CSR loop in fp64 from +0, rounded to T (the CPU stand-in for the handle's product)"""
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[: rp[-1]], dtype=np.int64)
    vals = np.asarray(va[: rp[-1]]).astype(np.float64)

    def product(x):
        y = np.zeros(n)
        with np.errstate(all="ignore"):
            np.add.at(y, rows, vals * np.asarray(x).astype(np.float64)[cols])
        return y.astype(dtype)
    return product


def inverse_blocks(rp, ci, va, bs, dtype):
    """numpy's inverse of `blocks_of`, rounded to T: a stand-in for the exported W where no device is at hand"""
    return np.linalg.inv(blocks_of(rp, ci, va, bs)).astype(dtype)
