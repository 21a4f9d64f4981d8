"""The recurrences of cvr_cg_device and cvr_bicgstab_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the
solver tests compare the device with, value by value.

What the header fixes and this file does: every stored vector is rounded to the handle's type T once (`x = T(double(x) + alpha * double(p))`, two
roundings in fp64 and one to T: numpy's ufuncs never fuse), every scalar is an fp64 quotient of fp64 sums, a sum's terms are
`double(a_i) * double(b_i)`, each rounded on its own, and they are added in the documented tree (`tree_sum`).  `exact_sum` adds the same terms
without any rounding but the last (math.fsum); the two differ by at most `sum_bound` times the sum of the terms' magnitudes.

The matrix enters through `product`, a callback x -> T(A x) on arrays of n values: on the GPU the handle's own cvr_spmv_device, whose bits the header
promises for q = A p (tests/test_gpu_krylov_model.py), on the CPU the oracle's CSR loop rounded to T.  The models therefore pin the vector kernels,
the sums, the scalars and the stop logic, not the product.

A model run returns a Trajectory: steps[k] is what the device must return for max_iters = k (x, iterations, status, residual_norm, b_norm, and the
scalars that led there); the last entry is terminal when the run converged or broke down -- a larger max_iters returns the same.  Entries that are
not terminal do not depend on rtol.  `compare` is the one comparison of a device result with such an entry.

The models are classes whose methods are the single operations of the header, so that a mutant (tests/test_krylov_model_host.py) is the model with
one method replaced."""
import math

import numpy as np

from cvr_amd import synth

CONVERGED, MAX_ITERS, BREAKDOWN = 0, 1, 2          # CVR_CG_* of include/cvr_amd.h

BLOCKS, THREADS, LANES = 1024, 256, 64             # the fixed grid of the sums
GRID = BLOCKS * THREADS                            # 262 144 threads: a thread's packets are g, g + GRID, ...
WAVES = THREADS // LANES


def pack_of(dtype):
    """values per 16-byte packet: 2 for fp64, 4 for fp32"""
    return 16 // np.dtype(dtype).itemsize


def trips_of(n, pack):
    """how often the longest-serving thread goes round the packet loop over n values"""
    return max(1, -(-int(n) // (GRID * pack)))


def _f64(a):
    return np.asarray(a).astype(np.float64)


def butterfly(a):
    """a: (..., LANES) -> (...): a += a[lane ^ o] for o = 32 .. 1 (every lane ends with the same bits, fp addition being commutative: lane l < o adds
    lane l + o)"""
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    return a[..., 0]


def _lanes_then_waves(a):
    """a: (..., WAVES, LANES) -> (...): the butterfly in every wavefront, then the wavefronts in order from +0"""
    a = butterfly(a)
    s = np.zeros(a.shape[:-1])
    for w in range(WAVES):
        s = s + a[..., w]
    return s


def tree_partials(terms, pack):
    """the 1024 workgroup partials of the documented tree over fp64 terms, bit for bit: thread g = workgroup * 256 + thread of a 1024 x 256 grid adds
    its packets g, g + 262 144, ... in order, each packet's `pack` values in order, from +0; lanes by butterfly, the four wavefronts in order from +0.
    (A value that does not exist adds nothing; +0 added to a sum that started from +0 changes no bit, so the missing values are padded with +0.)"""
    t = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1)
    n = t.size
    trips = trips_of(n, pack)
    threads = GRID if trips > 1 else max(THREADS, -(-(-(-n // pack)) // THREADS) * THREADS)          # whole workgroups; the rest hold +0
    buf = np.zeros(trips * threads * pack)
    buf[:n] = t
    buf = buf.reshape(trips, threads, pack)
    acc = np.zeros(threads)
    with np.errstate(all="ignore"):
        for trip in range(trips):
            for j in range(pack):
                acc = acc + buf[trip, :, j]
        part = np.zeros(BLOCKS)
        part[: threads // THREADS] = _lanes_then_waves(acc.reshape(-1, WAVES, LANES))
    return part


def tree_sum(terms, pack):
    """the documented tree over fp64 terms, bit for bit: the partials of `tree_partials`; of those thread t adds t, t + 256, t + 512, t + 768 in order
    from +0, then the same butterfly and wavefronts"""
    part = tree_partials(terms, pack)
    with np.errstate(all="ignore"):
        a = np.zeros(THREADS)
        for j in range(BLOCKS // THREADS):
            a = a + part[j * THREADS:(j + 1) * THREADS]
        return np.float64(_lanes_then_waves(a.reshape(WAVES, LANES)))


def exact_sum(terms):
    """the correctly rounded sum of the same terms"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    if not np.isfinite(t).all():
        with np.errstate(all="ignore"):
            return np.float64(t.sum())
    return np.float64(math.fsum(t.tolist()))


def sum_bound(n, pack):
    """gamma with |tree_sum - exact_sum| <= gamma * sum |terms|: one rounding of 2^-53 relative per addition on the longest path through the tree --
    pack * trips in the thread, 6 + 4 in the workgroup, 4 + 6 + 4 over the partials"""
    return (pack * trips_of(n, pack) + 24) * 2.0 ** -53


class Step:
    """what the device returns for max_iters = k, and the scalars of the step that led there"""

    def __init__(self, x, iterations, status, residual_norm, b_norm, terminal=False, **scalars):
        self.x, self.iterations, self.status = x, int(iterations), int(status)
        self.residual_norm, self.b_norm, self.terminal = np.float64(residual_norm), np.float64(b_norm), terminal
        self.scalars = scalars

    def __repr__(self):
        return f"Step(iterations={self.iterations}, status={self.status}, residual_norm={self.residual_norm!r}, b_norm={self.b_norm!r}, terminal={self.terminal})"


class Trajectory:
    def __init__(self):
        self.steps = []
        self.first = {}

    def add(self, *a, **kw):
        self.steps.append(Step(*a, **kw))
        return self

    @property
    def last(self):
        return self.steps[-1]

    def at(self, max_iters):
        """the entry for max_iters (beyond a terminal entry: that entry)"""
        if max_iters < len(self.steps):
            return self.steps[max_iters]
        assert self.last.terminal, (max_iters, len(self.steps))
        return self.last


class Got:
    """a device result in the model's terms"""

    def __init__(self, x, iterations, status, residual_norm, b_norm):
        self.x, self.iterations, self.status, self.residual_norm, self.b_norm = x, int(iterations), int(status), np.float64(residual_norm), np.float64(b_norm)


def _bits(v):
    return np.float64(v).tobytes()


def _ulps_apart(a, b):
    """|a - b| in units of the last place of fp64; inf when one of them is not finite and the bits differ"""
    if _bits(a) == _bits(b):
        return 0.0
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    return float(abs(a - b) / np.spacing(max(abs(a), abs(b))))


def compare(got, step, norm_ulps=0):
    """the one comparison of a result (a Got or a Step) with a model entry: x byte for byte, iterations and status equal, residual_norm and b_norm
    equal as bits (`norm_ulps` > 0: within that many units of the last place).  Returns "" when they agree, else what differs."""
    bad = []
    if (got.iterations, got.status) != (step.iterations, step.status):
        bad.append(f"(iterations, status) = {(got.iterations, got.status)}, model {(step.iterations, step.status)}")
    for name in ("residual_norm", "b_norm"):
        g, m = getattr(got, name), getattr(step, name)
        if _ulps_apart(g, m) > norm_ulps:
            bad.append(f"{name} = {g!r}, model {m!r} ({_ulps_apart(g, m):.3g} ulp)")
    gx, mx = np.ascontiguousarray(got.x), np.ascontiguousarray(step.x)
    if gx.dtype != mx.dtype or gx.shape != mx.shape:
        bad.append(f"x is {gx.dtype}{gx.shape}, model {mx.dtype}{mx.shape}")
    elif gx.tobytes() != mx.tobytes():
        d = np.flatnonzero((gx.view(np.uint8).reshape(gx.size, -1) != mx.view(np.uint8).reshape(mx.size, -1)).any(axis=1))
        i = int(d[0])
        bad.append(f"x differs in {len(d)} of {gx.size} values, first at {i}: {gx[i]!r}, model {mx[i]!r}")
    return "; ".join(bad)


def _usable(v):
    return v != 0 and np.isfinite(v)


class _Model:
    def __init__(self, product, dtype, sums="tree"):
        assert sums in ("tree", "exact"), sums
        self.product, self.T, self.sums, self.pack = product, np.dtype(dtype).type, sums, pack_of(dtype)

    # ---- the single operations of the header ----
    def terms(self, a, b):
        return _f64(a) * _f64(b)

    def dot(self, name, a, b):
        """the sum called `name` ("b.b", "r.r", "r.z", "p.q", ...) of the rounded T values a and b"""
        t = self.terms(a, b)
        return tree_sum(t, self.pack) if self.sums == "tree" else exact_sum(t)

    def rnd(self, v):
        return np.asarray(v).astype(self.T)

    def scale(self, minv, r):
        """T(double(minv) * double(r)); r itself without a preconditioner"""
        return r if minv is None else self.rnd(_f64(minv) * _f64(r))

    def axpy(self, name, y, a, x):
        """the update called `name`: T(double(y) + a * double(x))"""
        return self.rnd(_f64(y) + a * _f64(x))

    def start(self, b, x0, minv):
        b = np.ascontiguousarray(b, dtype=self.T)
        x = np.zeros(len(b), dtype=self.T) if x0 is None else np.array(x0, dtype=self.T)
        m = None if minv is None else np.ascontiguousarray(minv, dtype=self.T)
        r = self.rnd(_f64(b) - _f64(self.product(x)))          # what the scaled product with alpha = -1, beta = 1 stores
        return b, x, m, r

    def within(self, norm, rtol, bnorm):
        """the stop test: a residual norm that is not finite never counts as converged"""
        return bool(norm <= np.float64(rtol) * bnorm and np.isfinite(norm))


class CgModel(_Model):
    """cvr_cg_device"""

    def alpha(self, rz, pq):
        return rz / pq

    def beta(self, rz_new, rz_old):
        return rz_new / rz_old

    def rz_of_step(self, hist, k):
        """r.z that step k divides: the one formed at the end of step k - 1 (hist[0]: at the start)"""
        return hist[k]

    def refresh_z(self, minv, r, z):
        return self.scale(minv, r)

    def stop_sum(self, rr, rz):
        return rr

    def run(self, b, x0=None, minv=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, minv, rtol, max_iters)

    def _run(self, b, x0, minv, rtol, max_iters):
        tr = Trajectory()
        b, x, m, r = self.start(b, x0, minv)
        z = self.scale(m, r)
        p = z.copy()
        bb, rr = self.dot("b.b", b, b), self.dot("r.r", r, r)
        rz = rr if m is None else self.dot("r.z", r, z)
        bnorm, rnorm = np.sqrt(bb), np.sqrt(self.stop_sum(rr, rz))
        if bb == 0:
            return tr.add(np.zeros(len(b), dtype=self.T), 0, CONVERGED, 0.0, bnorm, terminal=True, bb=bb)
        if self.within(rnorm, rtol, bnorm):
            return tr.add(x, 0, CONVERGED, rnorm, bnorm, terminal=True, bb=bb, rr=rr, rz=rz)
        tr.add(x, 0, MAX_ITERS, rnorm, bnorm, bb=bb, rr=rr, rz=rz)
        hist = [rz]
        for k in range(max_iters):
            q = self.product(p)
            pq = self.dot("p.q", p, q)
            if not (pq > 0 and np.isfinite(pq)):          # found before the step is applied: x stays at the last iterate
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, pq=pq)
            alpha = self.alpha(self.rz_of_step(hist, k), pq)
            x = self.axpy("x", x, alpha, p)
            r = self.axpy("r", r, -alpha, q)
            z = self.refresh_z(m, r, z)
            rr = self.dot("r.r", r, r)
            rz = rr if m is None else self.dot("r.z", r, z)
            rnorm = np.sqrt(self.stop_sum(rr, rz))
            sc = dict(pq=pq, alpha=alpha, rr=rr, rz=rz)
            if k == 0:
                tr.first = dict(p=p, q=q)          # the vectors of step 0, for error bounds
            if self.within(rnorm, rtol, bnorm):
                return tr.add(x, k + 1, CONVERGED, rnorm, bnorm, terminal=True, **sc)
            beta = self.beta(rz, self.rz_of_step(hist, k))
            hist.append(rz)
            p = self.axpy("p", z, beta, p)
            tr.add(x, k + 1, MAX_ITERS, rnorm, bnorm, beta=beta, **sc)
        return tr


class BicgstabModel(_Model):
    """cvr_bicgstab_device"""

    def omega(self, ts, tt):
        return ts / tt

    def beta(self, rho1, rho, alpha, omega):
        return (rho1 / rho) * (alpha / omega)

    def half_x(self, x, alpha, ph):
        """double(x) + alpha * double(p^), still in fp64"""
        return _f64(x) + alpha * _f64(ph)

    def shadow(self, rhat, r):
        """r^ after a step: unchanged"""
        return rhat

    def run(self, b, x0=None, minv=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, minv, rtol, max_iters)

    def _run(self, b, x0, minv, rtol, max_iters):
        tr = Trajectory()
        b, x, m, r = self.start(b, x0, minv)
        rhat, p = r.copy(), r.copy()
        ph = self.scale(m, p)
        bb, rho = self.dot("b.b", b, b), self.dot("r.r", r, r)
        bnorm, rnorm = np.sqrt(bb), np.sqrt(rho)
        if bb == 0:
            return tr.add(np.zeros(len(b), dtype=self.T), 0, CONVERGED, 0.0, bnorm, terminal=True, bb=bb)
        if self.within(rnorm, rtol, bnorm):
            return tr.add(x, 0, CONVERGED, rnorm, bnorm, terminal=True, bb=bb, rho=rho)
        tr.add(x, 0, MAX_ITERS, rnorm, bnorm, bb=bb, rho=rho)
        for k in range(max_iters):
            v = self.product(ph)
            rv = self.dot("r^.v", rhat, v)
            if not _usable(rv):
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, rv=rv)
            alpha = rho / rv
            s = self.axpy("s", r, -alpha, v)
            sh = self.scale(m, s)
            if k == 0:
                tr.first = dict(rhat=rhat, v=v, ph=ph, s=s, sh=sh)          # the vectors of step 0, for error bounds
            ss = self.dot("s.s", s, s)
            snorm = np.sqrt(ss)
            if self.within(snorm, rtol, bnorm):          # the half step: counts as one step, residual_norm is ||s||
                return tr.add(self.rnd(self.half_x(x, alpha, ph)), k + 1, CONVERGED, snorm, bnorm, terminal=True, half=True, rv=rv, alpha=alpha, ss=ss)
            t = self.product(sh)
            ts, tt = self.dot("t.s", t, s), self.dot("t.t", t, t)
            if k == 0:
                tr.first["t"] = t
            omega = self.omega(ts, tt)
            if not _usable(tt) or not _usable(omega):
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, rv=rv, alpha=alpha, ss=ss, ts=ts, tt=tt, omega=omega)
            x = self.rnd(self.half_x(x, alpha, ph) + omega * _f64(sh))
            r = self.axpy("r", s, -omega, t)
            rr, rho1 = self.dot("r.r", r, r), self.dot("r^.r", rhat, r)
            rnorm = np.sqrt(rr)
            sc = dict(rv=rv, alpha=alpha, ss=ss, ts=ts, tt=tt, omega=omega, rr=rr, rho1=rho1)
            if self.within(rnorm, rtol, bnorm):
                return tr.add(x, k + 1, CONVERGED, rnorm, bnorm, terminal=True, **sc)
            if not _usable(rho1):          # found before the next step
                return tr.add(x, k + 1, BREAKDOWN, rnorm, bnorm, terminal=True, **sc)
            beta = self.beta(rho1, rho, alpha, omega)
            p = self.rnd(_f64(r) + beta * (_f64(p) - omega * _f64(v)))
            ph = self.scale(m, p)
            rhat = self.shadow(rhat, r)
            rho = rho1
            tr.add(x, k + 1, MAX_ITERS, rnorm, bnorm, beta=beta, **sc)
        return tr


def cg_model(product, b, x0=None, minv=None, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return CgModel(product, dtype, sums).run(b, x0, minv, rtol, max_iters)


def bicgstab_model(product, b, x0=None, minv=None, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return BicgstabModel(product, dtype, sums).run(b, x0, minv, rtol, max_iters)


# ---- the cases the CPU and the GPU tests share ----
def banded(kind, n, dtype):
    """(n, n, row_ptr, col_idx, vals): synth.banded_sym(n, half_band=2) made SPD ("spd": spectrum in [0.5, 1.5]) or nonsymmetric ("nonsym": spectrum in
    the disc |z - 1| <= 0.5); valid from n = 1, where A = (1)"""
    n, _, rp, ci, _ = synth.banded_sym(n, half_band=2)
    return (synth.spd_from_pattern if kind == "spd" else synth.nonsym_from_pattern)(n, rp, ci, dtype=dtype)


def inputs(n, dtype, seed=0):
    """(b, a random start vector in [-1, 1), minv in [0.5, 2]), seeded by n"""
    rng = np.random.default_rng(20261018 + seed + n)
    b = rng.standard_normal(n).astype(dtype)
    x0 = (rng.random(n) * 2 - 1).astype(dtype)
    minv = (0.5 + 1.5 * rng.random(n)).astype(dtype)
    return b, x0, minv
