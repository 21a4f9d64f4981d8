"""LOBPCG as cvr_lobpcg_device runs it, in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the block eigensolver's
tests compare the device with.  The conventions are tests/krylov_model.py's: every stored vector is rounded to the handle's type T once, scalars are
fp64, a sum's terms are `double(a_i) * double(b_i)` added in the documented tree (`tree_sum_many` is krylov_model.tree_sum for many sums at once:
tests/test_lobpcg_model_host.py holds the two to the same bits), and the matrix and the preconditioner enter as callables: `product` (x -> T(A x)) and
`apply` (r -> T(M r), or None).  The Rayleigh-Ritz step is the header's loops in plain Python floats, in the header's order; the small eigensolver is
the library's own cvr_sym_eig_host (capi.sym_eig_host), an ingredient exactly as the product is.

One method per operation of the header, so that a mutant (tests/test_lobpcg_model_host.py) is the model with one method replaced."""
import math

import numpy as np

import krylov_model as KM
from cvr_amd import capi, synth
from krylov_model import _f64, _Model

CONVERGED, BREAKDOWN, MAX_ITERS = 0, 2, 4          # CVR_EIG_* of include/cvr_amd.h
LARGEST, SMALLEST = 0, 1
EPS23 = 3.666852862501036e-11                      # the header's literal
MAX_BLOCK = 8
PIVOT = {"float64": 2.0 ** -30, "float32": 2.0 ** -20}          # CVR_LOBPCG_PIVOT_F64 / _F32


def tree_sum_many(terms, pack):
    """krylov_model.tree_sum of every row of `terms` (E x n, fp64), bit for bit, in one go"""
    t = np.ascontiguousarray(terms, dtype=np.float64)
    E, n = t.shape
    trips = KM.trips_of(n, pack)
    threads = KM.GRID if trips > 1 else max(KM.THREADS, -(-(-(-n // pack)) // KM.THREADS) * KM.THREADS)
    buf = np.zeros((E, trips * threads * pack))
    buf[:, :n] = t
    buf = buf.reshape(E, trips, threads, pack)
    with np.errstate(all="ignore"):
        acc = np.zeros((E, threads))
        for trip in range(trips):
            for j in range(pack):
                acc = acc + buf[:, trip, :, j]
        part = np.zeros((E, KM.BLOCKS))
        part[:, : threads // KM.THREADS] = KM._lanes_then_waves(acc.reshape(E, -1, KM.WAVES, KM.LANES))
        a = np.zeros((E, KM.THREADS))
        for j in range(KM.BLOCKS // KM.THREADS):
            a = a + part[:, j * KM.THREADS:(j + 1) * KM.THREADS]
        return KM._lanes_then_waves(a.reshape(E, KM.WAVES, KM.LANES))


class BlockEntry:
    """what the device returns: evals and resnorms (k, or none at a breakdown), X (n x k: the block as the call leaves it) and the result's fields"""

    def __init__(self, evals, resnorms, X, nconv, status, iterations, spmv_count, precond_applies, restarts_without_p, max_rel_residual):
        self.evals, self.resnorms, self.X = np.asarray(evals, dtype=np.float64), np.asarray(resnorms, dtype=np.float64), X
        self.nconv, self.status, self.iterations, self.spmv_count = int(nconv), int(status), int(iterations), int(spmv_count)
        self.precond_applies, self.restarts_without_p = int(precond_applies), int(restarts_without_p)
        self.max_rel_residual = np.float64(max_rel_residual)

    def __repr__(self):
        return (f"BlockEntry(evals={self.evals!r}, resnorms={self.resnorms!r}, nconv={self.nconv}, status={self.status}, iterations={self.iterations}, "
                f"spmv_count={self.spmv_count}, precond_applies={self.precond_applies}, restarts_without_p={self.restarts_without_p})")


def compare(got, want):
    """the bitwise comparison of a result with a model entry; "" when they agree, else what differs"""
    bad = []
    for name in ("nconv", "status", "iterations", "spmv_count", "precond_applies", "restarts_without_p"):
        if getattr(got, name) != getattr(want, name):
            bad.append(f"{name} = {getattr(got, name)}, model {getattr(want, name)}")
    for name in ("evals", "resnorms"):
        g, w = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        if g.shape != w.shape or g.tobytes() != w.tobytes():
            bad.append(f"{name} = {g!r}, model {w!r}")
    gx, wx = np.ascontiguousarray(got.X), np.ascontiguousarray(want.X)
    if gx.dtype != wx.dtype or gx.shape != wx.shape:
        bad.append(f"X is {gx.dtype}{gx.shape}, model {wx.dtype}{wx.shape}")
    elif gx.tobytes() != wx.tobytes():
        bad.append(f"X differs in {int(np.count_nonzero(gx != wx))} of {gx.size} values")
    return "; ".join(bad)


class LobpcgModel(_Model):
    """cvr_lobpcg_device"""
    passes = 2          # of step 3

    def __init__(self, product, dtype, apply=None):
        super().__init__(product, dtype, "tree")
        self.apply = apply
        self.tau = PIVOT[np.dtype(dtype).name]

    # ---- the single operations of the header ----
    def dots(self, A, B, pairs):
        """A_i . B_j for the (i, j) of `pairs`, each by the documented tree"""
        Ad, Bd = _f64(np.stack(A)), _f64(np.stack(B))
        ii, jj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        step = max(1, (1 << 23) // max(Ad.shape[1], 1))          # so many sums at once: the padded terms of a step stay below a few hundred MB
        return np.concatenate([tree_sum_many(Ad[ii[o:o + step]] * Bd[jj[o:o + step]], self.pack) for o in range(0, len(pairs), step)])

    def residual(self, ax, theta, x):
        """R_c = T(double(AX_c) - theta_c * double(X_c))"""
        return self.rnd(_f64(ax) - theta * _f64(x))

    def precondition(self, R):
        """W_c = M R_c by the object's apply, or W = R"""
        return [np.array(r) if self.apply is None else np.ascontiguousarray(self.apply(r), dtype=self.T) for r in R]

    def ortho_pass(self, X, W):
        """h_ic = X_i . W_c, all on the same W; t = double(w_c), t = t - h_0c double(x_0), ..; w_c = T(t)"""
        k = len(X)
        h = self.dots(X, W, [(i, c) for i in range(k) for c in range(k)]).reshape(k, k)
        out = []
        for c in range(k):
            t = _f64(W[c])
            for i in range(k):
                t = t - h[i, c] * _f64(X[i])
            out.append(self.rnd(t))
        return out

    def norms2(self, V):
        return self.dots(V, V, [(c, c) for c in range(len(V))])

    def divide(self, v, s):
        """T(double(v) / sqrt(s))"""
        return self.rnd(_f64(v) / np.sqrt(s))

    def gram(self, S, AS):
        """the lower triangles of G = S^T S and H = S^T (A S)"""
        m = len(S)
        pairs = [(i, j) for i in range(m) for j in range(i + 1)]
        g, h = self.dots(S, S, pairs), self.dots(S, AS, pairs)
        G, H = np.zeros((m, m)), np.zeros((m, m))
        for (i, j), gv, hv in zip(pairs, g, h):
            G[i, j], H[i, j] = gv, hv
        return G, H

    def cholesky(self, G, m, k):
        """L (lists of Python floats), or None at a pivot that is not finite, not > 0 or, with m = 3k, not > tau * G_jj"""
        g = G.tolist()
        tau = self.tau if m == 3 * k else 0.0
        L = [[0.0] * m for _ in range(m)]
        for j in range(m):
            s = g[j][j]
            for p in range(j):
                s = s - L[j][p] * L[j][p]
            if not (s > tau * g[j][j] and s > 0 and math.isfinite(s)):
                return None
            d = math.sqrt(s)
            L[j][j] = d
            for i in range(j + 1, m):
                t = g[i][j]
                for p in range(j):
                    t = t - L[i][p] * L[j][p]
                L[i][j] = t / d
        return L

    def reduced(self, L, H, m):
        """the lower triangle of M = L^-1 H L^-T, or None when it is not finite"""
        hh = H.tolist()
        Y = [[0.0] * m for _ in range(m)]
        for j in range(m):
            for i in range(m):
                t = hh[i][j] if i >= j else hh[j][i]
                for p in range(i):
                    t = t - L[i][p] * Y[p][j]
                Y[i][j] = t / L[i][i]
        M = np.zeros((m, m))
        Ml = [[0.0] * m for _ in range(m)]
        for i in range(m):
            for j in range(i + 1):
                t = Y[i][j]
                for p in range(j):
                    t = t - Ml[i][p] * L[j][p]
                Ml[i][j] = t / L[j][j]
                if not math.isfinite(Ml[i][j]):
                    return None
                M[i, j] = Ml[i][j]
        return M

    def small_eig(self, M):
        return capi.sym_eig_host(M)

    def select(self, which, m, k):
        return list(range(m - k, m)) if which == LARGEST else list(range(k))

    def back(self, L, z, m):
        """c = L^-T z"""
        x = [0.0] * m
        for i in range(m - 1, -1, -1):
            t = float(z[i])
            for p in range(i + 1, m):
                t = t - L[p][i] * x[p]
            x[i] = t / L[i][i]
        return np.array(x)

    def rayleigh_ritz(self, G, H, m, k, which):
        """(theta of the k wanted pairs, C: m x k) or None at a bad pivot"""
        L = self.cholesky(G, m, k)
        if L is None:
            return None
        M = self.reduced(L, H, m)
        if M is None:
            return None
        th, Z = self.small_eig(M)
        sel = self.select(which, m, k)
        return np.array([th[c] for c in sel]), np.stack([self.back(L, Z[:, c], m) for c in sel], axis=1)

    def p_first_row(self, k):
        """C~ is C with its first k rows zeroed: the sums of P' begin at row k"""
        return k

    def combine(self, c, V, first=0):
        """u = +0; u = u + c_l * double(V_l), l ascending from `first`; T(u)"""
        u = np.zeros(len(V[0]))
        for l in range(first, len(V)):
            u = u + c[l] * _f64(V[l])
        return self.rnd(u)

    def residual_theta(self, theta, c):
        """the Ritz value step 1 uses for column c"""
        return theta[c]

    # ---- the run ----
    def run(self, X0, which=SMALLEST, tol=1e-8, max_iters=200):
        """X0: n x k.  Returns a BlockEntry"""
        with np.errstate(all="ignore"):
            return self._run(np.ascontiguousarray(X0, dtype=self.T), which, np.float64(tol), int(max_iters))

    def _run(self, X0, which, tol, max_iters):
        n, k = X0.shape
        assert 1 <= k <= MAX_BLOCK and n >= 3 * k, (n, k)
        self.worst_xtw = 0.0
        S = [np.array(X0[:, c]) for c in range(k)]
        AS = [self.product(s) for s in S]
        spmvs, applies, fallbacks, iterations = k, 0, 0, 0

        def broken():
            return BlockEntry([], [], X0, 0, BREAKDOWN, iterations, spmvs, applies, fallbacks, 0.0)
        G, H = self.gram(S, AS)
        rr = self.rayleigh_ritz(G, H, k, k, which)
        if rr is None:
            return broken()
        theta, C = rr
        X, AX = [self.combine(C[:, c], S) for c in range(k)], [self.combine(C[:, c], AS) for c in range(k)]
        P, AP = [], []
        while True:
            last = iterations == max_iters
            R = [self.residual(AX[c], self.residual_theta(theta, c), X[c]) for c in range(k)]
            rn = np.sqrt(self.norms2(R))
            if not last:
                W = self.precondition(R)
                applies += k if self.apply is not None else 0
                for _ in range(self.passes):
                    W = self.ortho_pass(X, W)
                ww = self.norms2(W)
                W = [self.divide(W[c], ww[c]) if (ww[c] > 0 and np.isfinite(ww[c])) else W[c] for c in range(k)]
                self.worst_xtw = max(self.worst_xtw, float(np.abs(_f64(np.stack(X)) @ _f64(np.stack(W)).T).max()))          # (a diagnostic, plain numpy)
                AW = [self.product(w) for w in W]
                spmvs += k
                S, AS = X + W + P, AX + AW + AP
                G, H = self.gram(S, AS)
            scale = np.maximum(EPS23, np.abs(theta))
            if not (np.isfinite(rn).all() and np.isfinite(theta).all()):
                return broken()
            nconv = int(np.count_nonzero(rn <= tol * scale))
            entry = BlockEntry(theta, rn, np.stack(X, axis=1), nconv, CONVERGED if nconv == k else MAX_ITERS, iterations, spmvs, applies, fallbacks,
                               float(np.max(rn / scale)))
            if nconv == k or last:
                return entry
            if not all(w > 0 and np.isfinite(w) for w in ww):
                return broken()
            m = len(S)
            rr = self.rayleigh_ritz(G, H, m, k, which)
            if rr is None and m == 3 * k:
                fallbacks += 1
                m = 2 * k
                rr = self.rayleigh_ritz(G[:m, :m], H[:m, :m], m, k, which)
            if rr is None:
                return broken()
            theta, C = rr
            S, AS = S[:m], AS[:m]
            first = self.p_first_row(k)
            Xn, AXn = [self.combine(C[:, c], S) for c in range(k)], [self.combine(C[:, c], AS) for c in range(k)]
            P, AP = [self.combine(C[:, c], S, first) for c in range(k)], [self.combine(C[:, c], AS, first) for c in range(k)]
            pp = self.norms2(P)
            for c in range(k):
                if pp[c] > 0 and np.isfinite(pp[c]):
                    P[c], AP[c] = self.divide(P[c], pp[c]), self.divide(AP[c], pp[c])
            X, AX = Xn, AXn
            iterations += 1


def lobpcg_model(product, X0, apply=None, which=SMALLEST, tol=1e-8, max_iters=200, dtype=np.float64):
    return LobpcgModel(product, dtype, apply).run(X0, which, tol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def laplacian_grid(mx, my, dtype):
    """(n, n, row_ptr, col_idx, vals) of the five-point Laplacian of an mx x my grid with Dirichlet boundaries (row-major: vertex (i, j) = i * my + j)"""
    n = mx * my
    rp, ci, va = [0], [], []
    for i in range(mx):
        for j in range(my):
            for di, dj, v in ((-1, 0, -1.0), (0, -1, -1.0), (0, 0, 4.0), (0, 1, -1.0), (1, 0, -1.0)):
                if 0 <= i + di < mx and 0 <= j + dj < my:
                    ci.append((i + di) * my + j + dj)
                    va.append(v)
            rp.append(len(ci))
    return n, n, np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def banded(n, dtype, half_band=2):
    """synth.banded_sym(n, half_band) as the project's solvers use it: its pattern made symmetric positive definite by synth.spd_from_pattern
    (spectrum in [0.5, 1.5], symmetric bit for bit; the generator's own values are not symmetric)"""
    _, _, rp, ci, _ = synth.banded_sym(n, half_band=half_band)
    return synth.spd_from_pattern(n, rp, ci, dtype=dtype)


def dense_of(n, rp, ci, va):
    A = np.zeros((n, n))
    for i in range(n):
        for p in range(rp[i], rp[i + 1]):
            A[i, ci[p]] += float(va[p])
    return A


def dense_product(A, dtype):
    """x -> T(A x) in fp64 (the CPU tests' product)"""
    def product(x):
        return (A @ _f64(x)).astype(dtype)
    return product


def fused_product(n, rp, ci, va):
    """x -> A x as an fp32 SpMV of the library forms a row: the entries in CSR order from +0, one fused multiply-add each (the product exact, one
    rounding to fp32 per entry: float(double(a) * double(x) + double(acc)); the sum of an exact 48-bit product and a float is rounded to double
    first, which changes the fp32 result only in a tie of the second rounding)"""
    rp = np.asarray(rp)
    lens = np.diff(rp)
    width = int(lens.max())
    ok = np.arange(width)[None, :] < lens[:, None]
    idx = np.where(ok, rp[:-1, None] + np.arange(width)[None, :], 0)
    V, cols = np.where(ok, np.asarray(va)[idx].astype(np.float64), 0.0), np.asarray(ci)[idx]

    def product(x):
        x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
        acc = np.zeros(n, dtype=np.float32)
        for j in range(width):
            acc = np.where(ok[:, j], (V[:, j] * x64[cols[:, j]] + acc.astype(np.float64)).astype(np.float32), acc)
        return acc
    return product


def fp32_products(n, rp, ci, va):
    """the three CPU products the fp32 tolerances are found with: A x in fp64 rounded once to fp32; A x in fp32 throughout by a dense product; and
    `fused_product`"""
    A = dense_of(n, rp, ci, va)
    A32 = A.astype(np.float32)
    return {"fp64, rounded once": dense_product(A, np.float32), "fp32, dense": lambda x: A32 @ np.asarray(x, dtype=np.float32),
            "fp32, fused, CSR order": fused_product(n, rp, ci, va)}


def fp32_tolerance(n, rp, ci, va, k, max_iters=1500, tols=(1e-7, 1e-6, 1e-5, 1e-4)):
    """the smallest power of ten the model reaches in fp32 within max_iters with EVERY product of fp32_products (at fp32's rounding floor the
    rounding of the product decides whether a tolerance is reached; the handle's own product is one more such rounding), from start_block"""
    worst = 0.0
    for name, product in fp32_products(n, rp, ci, va).items():
        for tol in tols:
            if tol < worst:
                continue
            if LobpcgModel(product, np.float32).run(start_block(n, k, np.float32), SMALLEST, tol, max_iters).status == CONVERGED:
                worst = max(worst, tol)
                break
        else:
            return None
    return worst


# (matrix, k): what fp32_tolerance gives for the cases of tests/test_gpu_lobpcg.py ("lap24": laplacian_grid(24, 24), "lap40x12": laplacian_grid(40, 12),
# "band<n>": banded(n)); found on the CPU, and held there for two entries by tests/test_lobpcg_model_host.py.  Per product, the smallest power
# of ten reached, in the order of fp32_products: band63, k = 3: 1e-7, 1e-7, 1e-6 (with the fused product the model stands at residuals of
# 3.3e-8, 9.7e-8 and 1.4e-7 against 7.1e-8 after 1500 iterations: the two lowest eigenvalues are 7.7e-6 apart); band63, k = 4: 1e-6, 1e-5, 1e-5;
# lap24, k = 3 and lap40x12, k = 3: 1e-7 with one of the first two, 1e-6 with the other.
FP32_TOL = {
    ("lap24", 1): 1e-7, ("lap24", 3): 1e-6, ("lap24", 4): 1e-6, ("lap24", 8): 1e-6,
    ("lap40x12", 1): 1e-7, ("lap40x12", 3): 1e-6, ("lap40x12", 4): 1e-6, ("lap40x12", 8): 1e-6,
    ("band63", 1): 1e-7, ("band63", 3): 1e-6, ("band63", 4): 1e-5, ("band63", 8): 1e-6,
    ("band64", 3): 1e-6, ("band64", 8): 1e-6, ("band65", 4): 1e-6,
    ("band257", 1): 1e-7, ("band257", 8): 1e-5, ("band1025", 1): 1e-7, ("band4097", 1): 1e-7,
}


def start_block(n, k, dtype, seed=0):
    return np.random.default_rng(20261021 + 7 * seed + n).standard_normal((n, k)).astype(dtype)


def residual_allowance(A_abs, X, unit):
    """what one rounded product adds to a recomputed residual, per column: || unit * sum_j |a_ij x_j| ||_2 (the parity tests' allowance of one product,
    row-wise, in norm)"""
    return np.linalg.norm(unit * (A_abs @ np.abs(_f64(X))), axis=0)
