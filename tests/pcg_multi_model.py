"""cvr_precond_apply_multi_device and cvr_pcg_multi_device in numpy, written from the text of include/cvr_amd.h beside precond_model.py, whose apply and
whose Pcg it runs per column.

`apply_multi` is precond_model.apply on every column of a row-major block.  `PcgMulti` runs the columns in lock step, as the device does: every column
has its own state (x, r, z, p, the sums, a stop), a step is product | p.q | update | apply | direction over the columns that have not stopped, and
every write to one of the library's blocks is logged as (step, block, column) -- the header's "from then on no kernel writes its slices" is a
statement about writes, not about values (a stopped column's r no longer changes, so a second apply would store the same z), and the log is where a
model of it can be held to it: `writes_after_stop`."""
import numpy as np

import krylov_model as KM
import precond_model as PM


def apply_multi(W, R, bs, dtype, zsum=PM.left_to_right):
    """Z = M^-1 R: R of shape (n, nvec) in T; column c of Z is precond_model.apply of column c of R"""
    R = np.asarray(R, dtype=dtype)
    Z = np.zeros(R.shape, dtype=dtype)
    for c in range(R.shape[1]):
        Z[:, c] = PM.apply(W, R[:, c], bs, dtype, zsum=zsum)
    return Z


class PcgMulti:
    """cvr_pcg_multi_device: precond_model.Pcg's single operations, column by column in lock step.  run() returns one KM.Got per column."""

    def __init__(self, product, dtype, W, bs, sums="tree"):
        self.m = PM.Pcg(product, dtype, W, bs, sums)
        self.writes, self.stopped_at = [], {}

    # ---- what a mutant overrides ----
    def apply_columns(self, live, nvec):
        """the columns the step's apply writes: those that have not stopped"""
        return [c for c in range(nvec) if live[c]]

    def precondition(self, r):
        return self.m.precondition(r)

    def _stop(self, c, k, live):
        live[c] = False
        self.stopped_at[c] = k

    def run(self, B, X0=None, rtol=0.0, max_iters=6):
        with np.errstate(all="ignore"):
            return self._run(B, X0, rtol, max_iters)

    def _run(self, B, X0, rtol, max_iters):
        m, T = self.m, self.m.T
        B = np.asarray(B, dtype=T)
        n, nvec = B.shape
        X0 = np.zeros((n, nvec), dtype=T) if X0 is None else np.asarray(X0, dtype=T)
        self.writes, self.stopped_at = [], {}
        cols, live = [], [True] * nvec
        for c in range(nvec):          # the start: r = b - A x0, z = W r, p = z, the sums, the cell
            b, x, _, r = m.start(B[:, c], X0[:, c], None)
            z = self.precondition(r)
            s = dict(b=b, x=x, r=r, z=z, p=z.copy(), iters=0, status=KM.MAX_ITERS)
            bb, rr = m.dot("b.b", b, b), m.dot("r.r", r, r)
            s["rz"] = [m.dot("r.z", r, z)]
            s["bnorm"], s["rnorm"] = np.sqrt(bb), np.sqrt(rr)
            if bb == 0:
                s.update(x=np.zeros(n, dtype=T), rnorm=np.float64(0.0), status=KM.CONVERGED)
                self._stop(c, -1, live)
            elif m.within(s["rnorm"], rtol, s["bnorm"]):
                s["status"] = KM.CONVERGED
                self._stop(c, -1, live)
            cols.append(s)
        for k in range(max_iters):
            if not any(live):
                break
            for c, s in enumerate(cols):          # product, p.q, update
                if not live[c]:
                    continue
                s["q"] = m.product(s["p"])
                pq = m.dot("p.q", s["p"], s["q"])
                if not (pq > 0 and np.isfinite(pq)):
                    s["status"] = KM.BREAKDOWN
                    self._stop(c, k, live)
                    continue
                alpha = m.alpha(s["rz"][k], pq)
                s["x"], s["r"], s["iters"] = m.axpy("x", s["x"], alpha, s["p"]), m.axpy("r", s["r"], -alpha, s["q"]), k + 1
                self.writes += [(k, "x", c), (k, "r", c)]
            for c in self.apply_columns(live, nvec):          # the apply, a launch of its own
                cols[c]["z"] = self.precondition(cols[c]["r"])
                self.writes.append((k, "z", c))
            for c, s in enumerate(cols):          # direction
                if not live[c]:
                    continue
                rr, rz = m.dot("r.r", s["r"], s["r"]), m.dot("r.z", s["r"], s["z"])
                s["rnorm"] = np.sqrt(rr)
                if m.within(s["rnorm"], rtol, s["bnorm"]):
                    s["status"] = KM.CONVERGED
                    self._stop(c, k, live)
                    continue
                s["rz"].append(rz)
                s["p"] = m.axpy("p", s["z"], m.beta(rz, s["rz"][k]), s["p"])
                self.writes.append((k, "p", c))
        return [KM.Got(s["x"], s["iters"], s["status"], s["rnorm"], s["bnorm"]) for s in cols]


def writes_after_stop(model):
    """the logged writes to a column's slices behind its stop: in a later step, or in the same step when the step's update set the stop (a breakdown:
    that step wrote no x; a stop in the direction comes behind the step's update and apply)"""
    bad = []
    for k, blk, c in model.writes:
        if c in model.stopped_at:
            ks = model.stopped_at[c]
            if k > ks or (k == ks and (ks, "x", c) not in model.writes):
                bad.append((k, blk, c))
    return bad
