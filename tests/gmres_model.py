"""The recurrence of cvr_gmres_device in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the GMRES tests compare
the device with, value by value.  The conventions are tests/krylov_model.py's: every stored vector is rounded to the handle's type T once, scalars are
fp64, a sum's terms are `double(a_i) * double(b_i)` added in the documented tree, the matrix enters through `product` (x -> T(A x)), and a run returns
a Trajectory whose steps[k] is what the device must return for max_iters = k.

What GMRES adds to that: an entry is x formed from the columns of the cycle so far, so a run forms x after every step (from the cycle's start vector;
the run itself goes on from the basis).  A restart happens in front of the first step of a later cycle, so steps[k] for k a multiple of m is still the
entry behind the cycle's last step; a restart that converges or breaks down on the true residual appends a terminal entry with the same iteration count,
which Trajectory.at yields for every larger max_iters.

One method per operation of the header, so that a mutant (tests/test_gmres_host.py) is the model with one method replaced."""
import numpy as np

from krylov_model import BREAKDOWN, CONVERGED, MAX_ITERS, Trajectory, _f64, _Model, _usable


class GmresModel(_Model):
    """cvr_gmres_device with restart = m"""

    def __init__(self, product, dtype, sums="tree", restart=30):
        super().__init__(product, dtype, sums)
        assert 1 <= restart <= 64, restart
        self.m = int(restart)

    # ---- the single operations of the header ----
    def passes(self):
        """Gram-Schmidt passes per step: always two"""
        return 2

    def coefficients(self, V, w):
        """c_i = v_i . w for every column, all on the same w"""
        return [self.dot("v.w", v, w) for v in V]

    def subtract(self, V, c, w):
        """t = double(w); t = t - c_0 double(v_0); ...; w = T(t)"""
        t = _f64(w)
        for ci, v in zip(c, V):
            t = t - ci * _f64(v)
        return self.rnd(t)

    def combine(self, h, d):
        """H_i = h_i + d_i"""
        return h + d

    def rotate(self, cs, sn, a, b):
        """an earlier rotation on (H_i, H_(i+1)): the new pair"""
        return cs * a + sn * b, cs * b - sn * a

    def next_g(self, sn, g):
        """g_(j+1)"""
        return -(sn * g)

    def divisor(self, hn, rho):
        """what v_(j+1) = T(double(w) / .) divides by: the unrotated H_(j+1) = sqrt(ww)"""
        return hn

    def normalise(self, w, by):
        return self.rnd(_f64(w) / by)

    def back_substitute(self, R, g, q):
        """y of q columns: rows descending, each row's terms ascending"""
        y = np.zeros(q)
        for i in range(q - 1, -1, -1):
            t = g[i]
            for l in range(i + 1, q):
                t = t - R[i, l] * y[l]
            y[i] = t / R[i, i]
        return y

    def combination(self, y, V):
        """u = +0; u = u + y_i double(v_i), ascending"""
        u = np.zeros(len(V[0]))
        for yi, v in zip(y, V):
            u = u + yi * _f64(v)
        return u

    def form_x(self, x, minv, R, g, V, q):
        """x from q columns of the cycle (q = 0: x itself)"""
        if q == 0:
            return x
        u = self.combination(self.back_substitute(R, g, q), V[:q])
        return self.rnd(_f64(x) + (u if minv is None else _f64(minv) * u))

    def cycle_norm(self, rr, estimate):
        """a cycle's start norm: that of the true residual (estimate: |g_m| of the cycle before, None at the call's start)"""
        return np.sqrt(rr)

    def residual(self, b, x):
        return self.rnd(_f64(b) - _f64(self.product(x)))          # what the scaled product with alpha = -1, beta = 1 stores

    # ---- the run ----
    def run(self, b, x0=None, minv=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(b, x0, minv, rtol, max_iters)

    def _run(self, b, x0, minv, rtol, max_iters):
        tr = Trajectory()
        m = self.m
        b, x, mv, r = self.start(b, x0, minv)
        bb = self.dot("b.b", b, b)
        bnorm = np.sqrt(bb)
        if bb == 0:
            return tr.add(np.zeros(len(b), dtype=self.T), 0, CONVERGED, 0.0, bnorm, terminal=True, bb=bb)
        estimate = None
        k = 0
        while True:
            # a cycle's start: the call's, or in front of step k = a multiple of m
            if k > 0:
                r = self.residual(b, x)
            rr = self.dot("r.r", r, r)
            rnorm = self.cycle_norm(rr, estimate)
            if self.within(rnorm, rtol, bnorm):
                return tr.add(x, k, CONVERGED, rnorm, bnorm, terminal=True, rr=rr)
            if not np.isfinite(rnorm):
                return tr.add(x, k, BREAKDOWN, rnorm, bnorm, terminal=True, rr=rr)
            if k == 0:
                tr.add(x, 0, MAX_ITERS, rnorm, bnorm, bb=bb, rr=rr)
                if max_iters == 0:
                    return tr
            V = [self.normalise(r, rnorm)]
            g = np.zeros(m + 1)
            g[0] = rnorm
            cs, sn, R = np.zeros(m), np.zeros(m), np.zeros((m, m))
            for j in range(m):
                z = self.scale(mv, V[j])
                w = self.product(z)
                H = np.zeros(j + 2)
                parts = []
                for p in range(self.passes()):
                    c = self.coefficients(V, w)
                    w = self.subtract(V, c, w)
                    parts.append(np.array(c))
                H[: j + 1] = parts[0] if len(parts) == 1 else self.combine(parts[0], parts[1])
                ww = self.dot("w.w", w, w)
                hn = np.sqrt(ww)
                H[j + 1] = hn
                for i in range(j):
                    H[i], H[i + 1] = self.rotate(cs[i], sn[i], H[i], H[i + 1])
                rho = np.sqrt(H[j] * H[j] + H[j + 1] * H[j + 1])
                if not _usable(rho):          # found before the step is counted
                    return tr.add(self.form_x(x, mv, R, g, V, j), k, BREAKDOWN, abs(g[j]), bnorm, terminal=True, rho=rho, ww=ww)
                cs[j], sn[j] = H[j] / rho, H[j + 1] / rho
                R[:j, j] = H[:j]
                R[j, j] = rho
                g[j + 1] = self.next_g(sn[j], g[j])
                g[j] = cs[j] * g[j]
                k += 1
                e = abs(g[j + 1])
                xk = self.form_x(x, mv, R, g, V, j + 1)
                sc = dict(rho=rho, ww=ww, cs=cs[j], sn=sn[j], H=H.copy(), j=j)
                if k == 1:
                    tr.first = dict(v0=V[0], w=w)
                if self.within(e, rtol, bnorm):
                    return tr.add(xk, k, CONVERGED, e, bnorm, terminal=True, **sc)
                tr.add(xk, k, MAX_ITERS, e, bnorm, **sc)
                if k == max_iters:
                    return tr
                if j + 1 == m:
                    x, estimate = xk, e
                    break
                V.append(self.normalise(w, self.divisor(hn, rho)))


def gmres_model(product, b, x0=None, minv=None, restart=30, rtol=0.0, max_iters=6, dtype=np.float64, sums="tree"):
    return GmresModel(product, dtype, sums, restart).run(b, x0, minv, rtol, max_iters)
