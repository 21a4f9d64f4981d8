"""GPU (MI355X): cvr_cg_device, cvr_cg_multi_device and cvr_bicgstab_device step by step against the numpy model of include/cvr_amd.h
(tests/krylov_model.py; tests/test_krylov_model_host.py shows on the CPU that the comparison used here rejects a wrong sum, scalar or update).

The model's product is the handle's own cvr_spmv_device (an x buffer of info.x_elems values whose pad slot is 0, a y buffer of info.yext_elems values),
whose bits the header promises for q = A p; everything else -- the vector updates, the fixed-tree sums, the scalars, the stop and breakdown tests --
is the model's own arithmetic.  Two tiers:

  * bit for bit: for max_iters = 0 .. 6 at rtol = 0, and for one solve to the usual rtol, x byte for byte and iterations, status, residual_norm and
    b_norm equal to the model's entry (sums="tree").  The entries below the largest max_iters are compared with read-backs after every step and
    aligned arrays; the last one and the solve also with the default check_every and with b, x and minv shifted off the 16-byte grid one by one.
  * whatever the order of the sums: one step from a random start against the model with exact sums, within the derived bound of the difference
    between any summation order and the exact sum (krylov_model.sum_bound).  It tells a wrong order from wrong arithmetic if the first tier fails.

The sizes are those where the packet loop changes shape: a partial packet alone, whole packets and a partial one, one workgroup and several, every
thread with one packet (262 144 * pack values), one value more (a second trip for thread 0 alone), and a second trip that ends in a partial packet.
Beyond one trip the sweep stops at 3 steps; there the entries come from the run to rtol (entries that are not terminal do not depend on rtol)."""
import numpy as np
import pytest
import torch

import cases as K
import cvr_amd
import krylov_model as KM
from cvr_amd import synth

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-10, np.float32: 1e-4}
MAX_ITERS = 60
G = KM.GRID
SMALL = [1, 2, 3, 4, 5, 7, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 40001]
SHIFTS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]          # (b, x, minv) in elements


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _big(pack):
    return [G * pack - 1, G * pack, G * pack + 1, 2 * G * pack + pack + 1]


def _cases(small, big=True):
    return [(prec, n) for prec, pack in (("fp64", 2), ("fp32", 4)) for n in list(small) + (_big(pack) if big else [])]


def _shifts(dtype):
    return SHIFTS + ([(2, 3, 1)] if dtype == np.float32 else [])


class Dev:
    """a handle with the buffers of the model's product and the solver calls in the model's terms"""

    def __init__(self, H):
        self.H, self.n = H, H.nrows
        self.tdt = torch.float64 if H.dtype == np.float64 else torch.float32
        self.xbuf = torch.zeros(max(H.info.x_elems, self.n + 1), dtype=self.tdt, device="cuda")
        self.ybuf = torch.zeros(max(H.info.yext_elems, self.n, 1), dtype=self.tdt, device="cuda")

    def product(self, p):
        self.xbuf[: self.n].copy_(torch.from_numpy(np.ascontiguousarray(p, dtype=self.H.dtype)))
        torch.cuda.synchronize()
        self.H.spmv_device(self.xbuf.data_ptr(), self.ybuf.data_ptr())
        torch.cuda.synchronize()
        return self.ybuf[: self.n].cpu().numpy()

    def put(self, a, shift=0):
        a = np.ascontiguousarray(a, dtype=self.H.dtype).reshape(-1)
        t = torch.empty(a.size + shift, dtype=self.tdt, device="cuda")[shift:]
        t.copy_(torch.from_numpy(a))
        return t

    def solve(self, method, b, x0, minv, shifts=(0, 0, 0), **kw):
        """cvr_cg_device / cvr_bicgstab_device on arrays of exactly nrows values; (Got, result)"""
        bt = self.put(b, shifts[0])
        xt = self.put(np.zeros(self.n) if x0 is None else x0, shifts[1])
        mt = None if minv is None else self.put(minv, shifts[2])
        torch.cuda.synchronize()
        res = getattr(self.H, method)(bt.data_ptr(), xt.data_ptr(), minv_ptr=None if mt is None else mt.data_ptr(), **kw)
        torch.cuda.synchronize()
        return KM.Got(xt.cpu().numpy(), res.iterations, res.status, res.residual_norm, res.b_norm), res


def _same(got, entry, ctx):
    msg = KM.compare(got, entry)
    assert msg == "", (ctx, msg)


def _trajectory(dev, method, model, b, x0, minv, kmax, ctx):
    """the bitwise tier for one system"""
    dtype = dev.H.dtype
    rtol = RTOL[dtype]
    per_step = 1 if method == "cg" else 2
    full = model(dev.product, dtype).run(b, x0, minv, rtol=rtol, max_iters=MAX_ITERS)
    assert full.last.terminal and full.last.status == KM.CONVERGED, (ctx, full.last)
    if dev.n > 50000:          # (one model run serves both)
        assert len(full.steps) > kmax + 1, (ctx, len(full.steps))
        entries = full.steps[: kmax + 1]
    else:
        free = model(dev.product, dtype).run(b, x0, minv, rtol=0.0, max_iters=kmax)
        entries = [free.at(k) for k in range(kmax + 1)]
    for k in range(kmax + 1):
        got, res = dev.solve(method, b, x0, minv, rtol=0.0, max_iters=k, check_every=1)
        _same(got, entries[k], (ctx, "max_iters", k))
    for shifts in _shifts(dtype):
        for every in (0,) if shifts != (0, 0, 0) else (0, 3):
            got, _ = dev.solve(method, b, x0, minv, shifts=shifts, rtol=0.0, max_iters=kmax, check_every=every)
            _same(got, entries[kmax], (ctx, "max_iters", kmax, "shifts", shifts, "check_every", every))
    got, res = dev.solve(method, b, x0, minv, rtol=rtol, max_iters=MAX_ITERS, check_every=1)
    _same(got, full.last, (ctx, "rtol"))
    if full.last.iterations > 0:
        assert res.spmv_count == per_step * res.iterations + 1, (ctx, res.spmv_count, res.iterations)
    for shifts in _shifts(dtype)[:2] + _shifts(dtype)[-1:]:
        got, _ = dev.solve(method, b, x0, minv, shifts=shifts, rtol=rtol, max_iters=MAX_ITERS)
        _same(got, full.last, (ctx, "rtol", "shifts", shifts))
    return full


def _ulp(x):
    return np.spacing(np.abs(x)).astype(np.float64)


def _close(a, b, rel=1e-12):
    return abs(float(a) - float(b)) <= rel * abs(float(b))


def _one_step_any_order(dev, method, model, b, x0, minv, ctx):
    """the order-independent tier: x_1 from a random start against the model with exact sums.  gamma = krylov_model.sum_bound: any order of the
    additions is within gamma * sum |terms| of the exact sum.
    CG: alpha = r.z / p.q; r.z has condition 1 (with minv in [0.5, 2]: its terms are positive), p.q >= 0.5 p.p and sum |p_i q_i| <= 1.5 p.p for a
    spectrum in [0.5, 1.5], condition <= 3: the relative error of alpha is at most 2 * 3 * gamma, and
      |x_1 - x_1^model| <= ulp_T(x_1) + 6 gamma |alpha p|     (two values within d of each other round to values within d + ulp).
    BiCGSTAB: alpha = rho / r^.v with relative error ea = 2 gamma c_rv, c_rv = sum |r^_i v_i| / |r^.v| >= 1 from the model's terms, da = ea |alpha|.
    s = T(r - alpha v) moves by da |v|, s^ by da |M v|, t = A s^ by da |u| with u = A M v (one more product), so omega = t.s / t.t moves by at most
      do = 2 gamma c_ts |omega| + da ((|u| |s| + |t| |v|) / t.t + 2 |omega| |u| / |t|),   c_ts = sum |t_i s_i| / |t.s|   (2-norms, first order), and
      |x_1 - x_1^model| <= ulp_T(x_1) + da |p^| + do |s^| + |omega| da |M v|."""
    dtype = dev.H.dtype
    n, pack = dev.n, KM.pack_of(dev.H.dtype)
    gamma = KM.sum_bound(n, pack)
    ex = model(dev.product, dtype, sums="exact").run(b, x0, minv, rtol=0.0, max_iters=1)
    e1 = ex.at(1)
    got, _ = dev.solve(method, b, x0, minv, rtol=0.0, max_iters=1)
    assert (got.iterations, got.status) == (e1.iterations, e1.status), (ctx, got.iterations, got.status, e1)
    assert e1.iterations == 1, (ctx, e1)
    f64 = lambda a: np.asarray(a).astype(np.float64)
    sc = e1.scalars
    if method == "cg":
        bound = _ulp(e1.x) + 6 * gamma * np.abs(sc["alpha"] * f64(ex.first["p"]))
    else:
        f = {k: f64(v) for k, v in ex.first.items()}
        da = 2 * gamma * (np.abs(f["rhat"] * f["v"]).sum() / abs(sc["rv"])) * abs(sc["alpha"])
        bound = _ulp(e1.x) + da * np.abs(f["ph"])
        if not sc.get("half"):
            mv = f["v"] if minv is None else f64((f64(minv) * f["v"]).astype(dtype))
            u = f64(dev.product(mv.astype(dtype)))
            nrm = np.linalg.norm
            om = abs(sc["omega"])
            do = 2 * gamma * (np.abs(f["t"] * f["s"]).sum() / abs(sc["ts"])) * om + da * ((nrm(u) * nrm(f["s"]) + nrm(f["t"]) * nrm(f["v"])) / sc["tt"] + 2 * om * nrm(u) / nrm(f["t"]))
            bound = bound + do * np.abs(f["sh"]) + om * da * np.abs(mv)
    err = np.abs(f64(got.x) - f64(e1.x))
    worst = float(np.max(err / bound))
    print(f"{ctx}: |x_1 - model| / bound = {worst:.3g}; residual_norm {got.residual_norm!r} (model {e1.residual_norm!r}), b_norm {got.b_norm!r} (model {e1.b_norm!r})")
    assert (err <= bound).all(), (ctx, worst)
    assert _close(got.residual_norm, e1.residual_norm) and _close(got.b_norm, e1.b_norm), (ctx, got.residual_norm, e1.residual_norm, got.b_norm, e1.b_norm)


def _variants(n, dtype):
    """(name, start, minv): without and with minv, from a zero and a random start; all four where the model is cheap"""
    b, x0, minv = KM.inputs(n, dtype)
    out = [("plain/zero", None, None), ("minv/random", x0, minv)]
    if n <= 50000:
        out += [("plain/random", x0, None), ("minv/zero", None, minv)]
    return b, x0, minv, out


def _run_single(H, method, model, n, dtype, ctx):
    dev = Dev(H)
    b, x0, minv, variants = _variants(n, dtype)
    kmax = 6 if n <= 50000 else 3
    for name, start, m in variants:
        _trajectory(dev, method, model, b, start, m, kmax, (ctx, name))
    for m in (None, minv):
        _one_step_any_order(dev, method, model, b, x0, m, (ctx, "one step", "minv" if m is not None else "plain"))


@pytest.mark.parametrize("prec,n", _cases(SMALL))
def test_cg_against_the_model(prec, n):
    dtype = _dtype(prec)
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        _run_single(A, "cg", KM.CgModel, n, dtype, ("cg", prec, n))
    finally:
        A.close()


@pytest.mark.parametrize("prec,n", _cases([1, 2, 3, 5, 129, 513, 1025, 40001]))
def test_bicgstab_against_the_model(prec, n):
    dtype = _dtype(prec)
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        _run_single(A, "bicgstab", KM.BicgstabModel, n, dtype, ("bicgstab", prec, n))
    finally:
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_bicgstab_half_step_stop(prec):
    """n = 129 from a zero start: ||s|| of step 2 lies below ||r|| of step 1 (tests/test_krylov_model_host.py finds the same on the CPU), so an rtol
    between them stops the solve at the half step of step 2 -- x = x_1 + alpha p^, residual_norm = ||s||"""
    dtype = _dtype(prec)
    n = 129
    _, _, rp, ci, va = KM.banded("nonsym", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va)
    try:
        dev = Dev(A)
        b, _, minv = KM.inputs(n, dtype)
        for m in (None, minv):
            free = KM.BicgstabModel(dev.product, dtype).run(b, None, m, rtol=0.0, max_iters=3)
            halves = [k for k in (1, 2, 3) if np.sqrt(free.steps[k].scalars["ss"]) < free.steps[k - 1].residual_norm]
            assert halves, "no step whose half-step residual lies below the residual before it"
            k = halves[-1]
            snorm, before = np.sqrt(free.steps[k].scalars["ss"]), free.steps[k - 1].residual_norm
            rtol = float(np.sqrt(snorm * before) / free.steps[0].b_norm)
            tr = KM.BicgstabModel(dev.product, dtype).run(b, None, m, rtol=rtol, max_iters=10)
            assert tr.last.scalars.get("half") and (tr.last.status, tr.last.iterations, tr.last.residual_norm) == (KM.CONVERGED, k, snorm)
            for shifts in _shifts(dtype):
                for every in (1, 0):
                    got, res = dev.solve("bicgstab", b, None, m, shifts=shifts, rtol=rtol, max_iters=10, check_every=every)
                    _same(got, tr.last, ("half step", prec, m is not None, shifts, every))
                    if every == 1:
                        assert res.spmv_count == 2 * k + 1
    finally:
        A.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("layout", ["default", "panels", "gang", "nvec"])
def test_cg_layouts_against_the_model(layout, prec):
    """the vector kernels are the same across layouts; info.x_elems, info.yext_elems, the scratch tail r shares with the scaled product and the
    library's buffers are not"""
    dtype = _dtype(prec)
    nrows, _, prp, pci, _ = synth.web_google_like(scale=0.05)
    n, _, rp, ci, va = synth.spd_from_pattern(nrows, prp, pci, dtype=dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, **K.ALL_LAYOUTS[layout])
    try:
        _run_single(A, "cg", KM.CgModel, n, dtype, ("cg", layout, prec))
    finally:
        A.close()


# ---- the batched solver against the model, column by column ----
def _multi(dev, B, X0, minv, nvec, **kw):
    """cvr_cg_multi_device with ldb = nvec + 1, ldx = nvec + 2, every array one element off the allocation's start; (X, results)"""
    n = dev.n
    ldb, ldx = nvec + 1, nvec + 2
    hb = np.full((n, ldb), -777.25, dtype=dev.H.dtype)
    hb[:, :nvec] = B[:, :nvec]
    hx = np.full((n, ldx), -777.25, dtype=dev.H.dtype)
    hx[:, :nvec] = X0[:, :nvec]
    bt, xt = dev.put(hb, 1), dev.put(hx, 1)
    mt = None if minv is None else dev.put(minv, 1)
    torch.cuda.synchronize()
    res = dev.H.cg_multi(bt.data_ptr(), ldb, xt.data_ptr(), ldx, nvec, minv_ptr=None if mt is None else mt.data_ptr(), **kw)
    torch.cuda.synchronize()
    X = xt.cpu().numpy().reshape(n, ldx)
    assert (X[:, nvec:] == -777.25).all() and bt.cpu().numpy().tobytes() == hb.tobytes()
    return X, res


@pytest.mark.parametrize("prec,n", _cases([3, 5, 513, 40001], big=False) + [("fp64", 2 * G * 2 + 3)])
def test_cg_multi_against_the_model(prec, n):
    """the columns stop at different steps: an ordinary one, b = 0, a start that solves the system already, b scaled by 1e-3 under a random start, and
    four more ordinary ones; nvec = 1, 3, 8 take the first columns.  Every column and res[j] against that column's own model run -- not through
    cvr_cg_device."""
    dtype = _dtype(prec)
    rtol = RTOL[dtype]
    two_trips = n > G
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
    try:
        dev = Dev(A)
        b, x0, minv = KM.inputs(n, dtype)
        rng = np.random.default_rng(n)
        ncol = 3 if two_trips else 8          # (beyond one trip the model of a column costs most of a second per solve: three columns)
        B = rng.standard_normal((n, 8)).astype(dtype)
        X0 = np.zeros((n, 8), dtype=dtype)
        B[:, 0] = b
        B[:, 1] = 0
        X0[:, 1] = x0
        for pre in (None, minv):
            solved = KM.CgModel(dev.product, dtype).run(b, None, pre, rtol=rtol / 8, max_iters=MAX_ITERS).last
            assert solved.status == KM.CONVERGED
            B[:, 2], X0[:, 2] = b, solved.x
            B[:, 3], X0[:, 3] = (1e-3 * B[:, 4]).astype(dtype), x0
            X0[:, 6] = x0
            full = [KM.CgModel(dev.product, dtype).run(B[:, j], X0[:, j], pre, rtol=rtol, max_iters=MAX_ITERS) for j in range(ncol)]
            assert all(t.last.terminal and t.last.status == KM.CONVERGED for t in full)
            assert full[1].last.iterations == 0 and full[2].last.iterations == 0 and not full[1].last.x.any()
            if ncol == 8:
                assert len({t.last.iterations for t in full}) >= (3 if n > 500 else 2), [t.last.iterations for t in full]          # (three unknowns are solved in three steps)
            free = [KM.CgModel(dev.product, dtype).run(B[:, j], X0[:, j], pre, rtol=0.0, max_iters=4) for j in range(ncol)]
            for nvec in (1, 3, 8):
                if nvec > ncol:
                    continue
                for k in range(5):
                    X, res = _multi(dev, B, X0, pre, nvec, rtol=0.0, max_iters=k, check_every=1 if k % 2 else 0)
                    for j in range(nvec):
                        r = res[j]
                        _same(KM.Got(np.ascontiguousarray(X[:, j]), r.iterations, r.status, r.residual_norm, r.b_norm), free[j].at(k), ("cg_multi", prec, n, pre is not None, nvec, "max_iters", k, "column", j))
                X, res = _multi(dev, B, X0, pre, nvec, rtol=rtol, max_iters=MAX_ITERS)
                for j in range(nvec):
                    r = res[j]
                    _same(KM.Got(np.ascontiguousarray(X[:, j]), r.iterations, r.status, r.residual_norm, r.b_norm), full[j].last, ("cg_multi", prec, n, pre is not None, nvec, "rtol", "column", j))
    finally:
        A.close()


def test_every_listed_nvec_runs_beyond_one_trip():
    """nvec = 8 on the two-trip size for the sweep's first steps (the model of eight columns to rtol would take most of a minute)"""
    dtype, n = np.float64, 2 * G * 2 + 3
    _, _, rp, ci, va = KM.banded("spd", n, dtype)
    A = cvr_amd.CvrMatrix(n, n, rp, ci, va, nvec=8)
    try:
        dev = Dev(A)
        rng = np.random.default_rng(8)
        B = rng.standard_normal((n, 8))
        X0 = np.zeros((n, 8))
        X0[:, 5] = rng.random(n) * 2 - 1
        B[:, 2] = 0
        free = [KM.CgModel(dev.product, dtype).run(B[:, j], X0[:, j], None, rtol=0.0, max_iters=2) for j in range(8)]
        for k in (0, 2):
            X, res = _multi(dev, B, X0, None, 8, rtol=0.0, max_iters=k)
            for j in range(8):
                r = res[j]
                _same(KM.Got(np.ascontiguousarray(X[:, j]), r.iterations, r.status, r.residual_norm, r.b_norm), free[j].at(k), ("cg_multi", n, 8, "max_iters", k, "column", j))
    finally:
        A.close()
