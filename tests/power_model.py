"""The loop of cvr_power_iteration in numpy, written from the text of include/cvr_amd.h (not from the kernels): the model the power-iteration tests
compare the device with, value by value.  Built like krylov_model.py, whose sum stages it shares: every stored x is rounded to the handle's type T
once (`x = T(double(y) * inv)`), every scalar is fp64, a sum's terms are `double(a_i) * double(b_i)`, each rounded on its own.

The matrix enters through `product`, a callback x -> T(A x) on arrays of n values: on the GPU the handle's own cvr_spmv_device, on the CPU the
oracle's CSR loop rounded to T.  The model therefore pins the vector work, the sums, the lagged norm, the fp32 range rule and lambda, not the product.

sums = "dense": every sum by the dense tree (`dense_cells`, then `final`): the unfused, exact-mode and sharded loops.
sums = "fused": the steps' sums by the fused tree over the chunks' row ranges (`chunks` = the first row of every chunk, in order; `wpb` = chunks per
                workgroup), as the header describes them; the start and the exact mode stay dense.  More than 1024 workgroups: the header says the
                fused tree does not apply, and the model is the dense one (`self.sums` says which).
sums = "exact": every sum correctly rounded (math.fsum), for bounds that hold whatever the order.

`sweep(x0, kmax)` returns a Result (x, lam, exact) for every iters = 0 .. kmax: what the device must return for that `iters`.  The last step
normalises exactly and the fp32 rule looks at `iters`, so the results are not prefixes of one another; the lagged iterates before the last step are.

The model is a class whose methods are the single operations of the header, so that a mutant (tests/test_power_model_host.py) is the model with one
method replaced.  `Shards` is the padded all-gather layout and its index map, and `sharded_step` the model of one sharded step."""
import numpy as np

import krylov_model as KM

CELLS = KM.BLOCKS          # 1024 partial sums per set


def _f64(a):
    return np.asarray(a).astype(np.float64)


class Result:
    """what the device returns for one `iters`: x (n values of T), lambda, and whether the exact mode was entered; sums = (x.y, y.y, x.x) of the last step"""

    def __init__(self, x, lam, exact, sums=None, est=None):
        self.x, self.lam, self.exact, self.sums, self.est = x, np.float64(lam), bool(exact), sums, est

    def __repr__(self):
        return f"Result(lam={self.lam!r}, exact={self.exact}, sums={self.sums})"


def compare(x, lam, res, lam_ulps=0):
    """the one comparison of a device result with a model Result: x byte for byte, lambda bit for bit (`lam_ulps` > 0: within that many units of the
    last place).  Returns "" when they agree, else what differs."""
    bad = []
    if KM._ulps_apart(lam, res.lam) > lam_ulps:
        bad.append(f"lambda = {np.float64(lam)!r}, model {res.lam!r} ({KM._ulps_apart(lam, res.lam):.3g} ulp)")
    gx, mx = np.ascontiguousarray(x), np.ascontiguousarray(res.x)
    if gx.dtype != mx.dtype or gx.shape != mx.shape:
        bad.append(f"x is {gx.dtype}{gx.shape}, model {mx.dtype}{mx.shape}")
    elif gx.tobytes() != mx.tobytes():
        d = np.flatnonzero((gx.view(np.uint8).reshape(gx.size, -1) != mx.view(np.uint8).reshape(mx.size, -1)).any(axis=1))
        i = int(d[0])
        bad.append(f"x differs in {len(d)} of {gx.size} values, first at {i}: {gx[i]!r}, model {mx[i]!r}")
    return "; ".join(bad)


class PowerModel:
    """cvr_power_iteration on one GPU (and, the sums being the dense tree's, of the sharded loop)"""

    rule_step = 0          # the step after which an fp32 handle looks at est

    def __init__(self, product, dtype, sums="dense", chunks=None, wpb=1):
        assert sums in ("dense", "fused", "exact"), sums
        self.product, self.T, self.sums = product, np.dtype(dtype).type, sums
        if sums == "fused":
            self.first = np.asarray(chunks, dtype=np.int64).reshape(-1)
            self.wpb = max(1, int(wpb))
            assert len(self.first) > 0 and self.first[0] == 0 and (np.diff(self.first) > 0).all(), "chunks: the first row of every chunk, ascending from 0"
            self.blocks = -(-len(self.first) // self.wpb)
            if self.blocks > CELLS:
                self.sums = "dense"

    # ---- the single operations of the header ----
    def terms(self, a, b):
        return _f64(a) * _f64(b)

    def final(self, cells):
        """the sum over 1024 cells: lane t adds t, t + 64, ..., t + 960 in order from +0, then the butterfly"""
        c = np.asarray(cells, dtype=np.float64).reshape(CELLS // KM.LANES, KM.LANES)
        acc = np.zeros(KM.LANES)
        for j in range(CELLS // KM.LANES):
            acc = acc + c[j]
        return np.float64(KM.butterfly(acc))

    def dense_cells(self, t):
        """the dense tree's 1024 workgroup partials: krylov_model's stage with one value per packet"""
        return KM.tree_partials(t, 1)

    def block_sum(self, w, nchunks):
        """w: (workgroups, wpb) chunk sums, +0 where a workgroup's wavefront has no chunk -> the workgroups' cells: its live wavefronts in chunk order
        from +0 (a +0 added to a sum that started from +0 changes no bit)"""
        s = np.zeros(w.shape[0])
        for j in range(w.shape[1]):
            s = s + w[:, j]
        return s

    def fused_cells(self, t):
        """the fused tree's 1024 cells: lane l of a chunk's wavefront adds the chunk's rows l, l + 64, ... in order from +0, butterfly, then block_sum"""
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        n, first = t.size, self.first
        assert first[-1] < n
        count = np.diff(np.append(first, n))
        nch = len(first)
        trips = -(-int(count.max()) // KM.LANES)
        owner = np.repeat(np.arange(nch), count)
        buf = np.zeros((nch, trips * KM.LANES))
        buf[owner, np.arange(n) - first[owner]] = t
        buf = buf.reshape(nch, trips, KM.LANES)
        acc = np.zeros((nch, KM.LANES))
        for j in range(trips):
            acc = acc + buf[:, j, :]
        w = np.zeros(self.blocks * self.wpb)
        w[:nch] = KM.butterfly(acc)
        cells = np.zeros(CELLS)
        cells[: self.blocks] = self.block_sum(w.reshape(self.blocks, self.wpb), nch)
        return cells

    def sum_dense(self, t):
        return KM.exact_sum(t) if self.sums == "exact" else self.final(self.dense_cells(t))

    def sum_step(self, t):
        """a sum of a step outside the exact mode"""
        return self.final(self.fused_cells(t)) if self.sums == "fused" else self.sum_dense(t)

    def inv(self, s):
        """1 / sqrt(s) where s > 0, else 0"""
        return np.float64(1.0) / np.sqrt(np.float64(s)) if s > 0 else np.float64(0.0)

    def scale(self, y, inv):
        return (_f64(y) * inv).astype(self.T)

    def inv_of_step(self, k, yy):
        """inv_k; yy[j] = y.y of step j (yy[k] is known too, and not used)"""
        return np.float64(1.0) if k == 0 else self.inv(yy[k - 1])

    def last_inv(self, k, yy):
        """the last step normalises exactly: with its own y.y"""
        return self.inv(yy[k])

    def rule_applies(self, iters):
        return self.T is np.float32 and iters > 1

    def est(self, yy, xx):
        return np.sqrt(yy / xx) if xx > 0 else np.float64(0.0)

    def in_range(self, est):
        return bool(est > 1e-15 and est < 1e15)

    def lam(self, sums_of_steps, iters):
        """lambda from the sums (x.y, y.y, x.x) of the steps 0 .. iters - 1"""
        if iters == 0:
            return np.float64(0.0)
        xy, _, xx = sums_of_steps[-1]
        return xy / xx if xx > 0 else np.float64(0.0)

    def start(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=self.T)
        return self.scale(x0, self.inv(self.sum_dense(self.terms(x0, x0))))

    def sums3(self, x, y, dense):
        f = self.sum_dense if dense else self.sum_step
        return (f(self.terms(x, y)), f(self.terms(y, y)), f(self.terms(x, x)))

    def step(self, x, y, prev_yy=None):
        """one step's vector work on given x and y (cvr_power_step_selfcheck): (new x, (x.y, y.y, x.x))"""
        s = self.sums3(x, y, dense=True)
        return self.scale(y, np.float64(1.0) if prev_yy is None else self.inv(prev_yy)), s

    # ---- the loop ----
    def _trajectory(self, x0, want, rule):
        """{iters: Result} for the `iters` in `want`, all of which give rule_applies(iters) == rule: one walk along the lagged iterates, which do not
        depend on `iters` otherwise; only the last step's x does"""
        out = {}
        x = self.start(x0)
        exact, est, sums, yy = False, None, [], []
        for k in range(max(want) if want else 0):
            last = k + 1 in want
            y = self.product(x)
            s = self.sums3(x, y, dense=exact)
            sums.append(s)
            yy.append(s[1])
            if not exact and rule and k == self.rule_step:
                est = self.est(s[1], s[2])
                exact = not self.in_range(est)
            if exact:
                x = self.scale(y, self.inv(s[1]))
                if last:
                    out[k + 1] = Result(x, self.lam(sums, k + 1), True, s, est)
                continue
            if last:
                out[k + 1] = Result(self.scale(y, self.last_inv(k, yy)), self.lam(sums, k + 1), False, s, est)
            x = self.scale(y, self.inv_of_step(k, yy))
        return out

    def sweep(self, x0, kmax, iters=None):
        """[Result for iters = 0 .. kmax] (or for the listed `iters`)"""
        want = list(range(kmax + 1)) if iters is None else list(iters)
        out = {}
        with np.errstate(all="ignore"):
            if 0 in want:
                out[0] = Result(self.start(x0), self.lam([], 0), False)
            for rule in (False, True):
                out.update(self._trajectory(x0, {k for k in want if k > 0 and bool(self.rule_applies(k)) == rule}, rule))
        return [out[k] for k in want]

    def run(self, x0, iters):
        return self.sweep(x0, iters, [iters])[0]


# ---- the sharded form ----
class Shards:
    """row blocks [bounds[p], bounds[p + 1]) of n = bounds[-1] rows, all-gathered in equal slices of max_rows values: shard p's rows lie at
    padded[p * max_rows ...]; the rest of a slice is padding nobody may read"""

    def __init__(self, bounds, max_rows=None):
        self.b = np.asarray(bounds, dtype=np.int64)
        assert self.b[0] == 0 and (np.diff(self.b) >= 0).all()
        self.nparts, self.n = len(self.b) - 1, int(self.b[-1])
        widest = int(np.diff(self.b).max())
        self.max_rows = widest if max_rows is None else int(max_rows)
        assert self.max_rows >= widest

    def owner(self, i):
        """the shard of row i: the LAST p with bounds[p] <= i (an empty shard owns nothing)"""
        return np.searchsorted(self.b[: self.nparts], i, side="right") - 1

    def offset(self, p):
        """where shard p's slice begins in the padded vector"""
        return p * self.max_rows

    def index(self):
        """j[i]: the place of row i in the padded vector"""
        i = np.arange(self.n, dtype=np.int64)
        p = self.owner(i)
        return self.offset(p) + (i - self.b[p])

    def pad(self, y, fill=np.nan):
        """the padded layout of a dense y, the padding slots holding `fill`"""
        y = np.ascontiguousarray(y)
        out = np.full(self.nparts * self.max_rows, fill, dtype=y.dtype)
        for p in range(self.nparts):
            r0, r1 = int(self.b[p]), int(self.b[p + 1])
            out[p * self.max_rows: p * self.max_rows + (r1 - r0)] = y[r0:r1]
        return out

    def unpad(self, padded):
        return np.ascontiguousarray(np.asarray(padded)[self.index()])


def sharded_step(model, shards, x, padded, prev_yy=None):
    """one step of the sharded loop: by the header the dense step on the un-padded vector"""
    return model.step(x, shards.unpad(padded), prev_yy)


# ---- bounds of the trees against the exact sum ----
def _gamma(depth):
    """|sum in some order - exact sum| <= gamma * sum |terms| when no term passes through more than `depth` additions: each rounds by 2^-53 relative,
    (1 + u)^depth - 1 <= depth u / (1 - depth u)"""
    u = 2.0 ** -53
    return depth * u / (1 - depth * u)


def dense_bound(n):
    """the dense tree: `trips` additions in the thread, 6 in the butterfly, 4 over the wavefronts; 16 in a lane over the partials and 6 in the last
    butterfly"""
    return _gamma(KM.trips_of(n, 1) + 6 + 4 + 16 + 6)


def fused_bound(most_rows, wpb):
    """the fused tree: ceil(rows of the fullest chunk / 64) additions in a lane, 6 in the butterfly, wpb over the workgroup's wavefronts, 16 + 6 over
    the cells"""
    return _gamma(-(-int(most_rows) // KM.LANES) + 6 + int(wpb) + 16 + 6)


# ---- the cases the CPU and the GPU tests share ----
def square(lens, dtype, seed=0, scale=1.0):
    """(n, n, row_ptr, col_idx, vals) with the given row lengths: columns drawn at random and ascending inside a row, values in [0.25, 1] * scale"""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    rng = np.random.default_rng(20261018 + seed)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    rows = np.repeat(np.arange(n), lens)
    ci = rng.integers(0, n, size=int(rp[-1]))
    ci = ci[np.lexsort((ci, rows))].astype(np.int32)
    va = ((0.25 + 0.75 * rng.random(int(rp[-1]))) * scale).astype(dtype)
    return n, n, rp, ci, va


def power_law(n, dtype, seed=0):
    """a square power-law matrix with about 25 % empty rows rows of up to 900 entries and one of min(n, 3000) (a small split_threshold cuts the long ones over chunks)"""
    rng = np.random.default_rng(977 + seed + n)
    lens = np.minimum((rng.pareto(1.3, size=n) + 1).astype(np.int64), min(900, max(n, 1)))
    lens[rng.random(n) < 0.25] = 0
    lens[n // 2] = min(3000, n)          # (one long row: with a small split_threshold it is cut over chunks wherever it does not fit what is left of one)
    return square(lens, dtype, seed)


def start_vectors(n, dtype, seed=0):
    """named start vectors: random in [-1, 1), ones, all zero"""
    rng = np.random.default_rng(5 + seed + n)
    return [("random", (rng.random(n) * 2 - 1).astype(dtype)), ("ones", np.ones(n, dtype=dtype)), ("zero", np.zeros(n, dtype=dtype))]


PHASES = dict(steps_per_chunk=12, waves_per_block=8, x_window=2048, col_phases=6, col_panels=1)                                     # cases.LAYOUTS["phases"]
TAGS = dict(steps_per_chunk=24, waves_per_block=4, x_window=2048, col_phases=4, row_tags16=1, piece_max=8, col_panels=1)          # ["phases_tags_pieces"]
SMALLEST = dict(steps_per_chunk=4, waves_per_block=1, x_window=0, col_phases=2, col_panels=1)          # the smallest S and wpb there are: 256 slots per chunk
_EDGE = [3, 0, 0, 9, 1]          # (cases.py: leading_trailing_empty)


def fused_cases():
    """name -> (options, row lengths, chunks, workgroups, fused): square matrices for the one-launch step, none with a row longer than the default
    split_threshold (32 S), so no row is cut; an empty row takes one slot.  `chunks` and `workgroups` are what the planner must make of them."""
    c = {}
    c["phases/one_chunk"] = (PHASES, [0] * 80 + _EDGE * 36 + [0] * 130, 1, 1, True)                                 # 390 rows in 750 of 768 slots
    c["phases/one_full_workgroup"] = (PHASES, [2] * (8 * 384), 8, 1, True)
    c["phases/short_last_workgroup"] = (PHASES, [0] * 70 + [2] * (8 * 384) + [0] * 130, 9, 2, True)
    c["phases/empty_runs"] = (PHASES, [0] * 700 + _EDGE * 400 + [0] * 1300, None, None, True)
    c["phases/65_workgroups"] = (PHASES, [3] * (512 * 256 + 50), 513, 65, True)
    c["tags/one_chunk"] = (TAGS, [0] * 70 + _EDGE * 40 + [0] * 130, 1, 1, True)
    c["tags/short_last_workgroup"] = (TAGS, [0] * 70 + [4] * (4 * 384) + [0] * 130, 5, 2, True)
    c["smallest/1024_workgroups"] = (SMALLEST, [1] * (1024 * 256 - 100), 1024, 1024, True)
    c["smallest/1025_workgroups"] = (SMALLEST, [1] * (1024 * 256 + 1), 1025, 1025, False)
    return c


def diag_dominant(n, scale):
    """a diagonal of 1 and two neighbours of 2^-10 on each side (cyclic), times `scale`, in fp32: |A x| / |x| lies within 2^-8 of `scale` for every x"""
    rows = np.repeat(np.arange(n), 5)
    ci = (rows + np.tile([-2, -1, 0, 1, 2], n)) % n
    va = np.tile([2.0 ** -10, 2.0 ** -10, 1.0, 2.0 ** -10, 2.0 ** -10], n) * scale
    order = np.lexsort((ci, rows))
    return n, n, np.arange(0, 5 * n + 1, 5, dtype=np.int64), ci[order].astype(np.int32), va[order].astype(np.float32)


def transposed(n, rp, ci, va):
    """(n, n, row_ptr, col_idx, vals) of the transpose of a square matrix, the entries of a row in ascending column order"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    order = np.lexsort((rows, ci))
    trp = np.zeros(n + 1, dtype=np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
    return n, n, trp, rows[order].astype(np.int32), va[order]


# the fp32 range rule's cases: est just inside and outside both thresholds (1 % off; the matrix keeps est within 0.4 % of `scale`), and far outside
RULE = [("inside_1e15", 1e15 * (1 - 0.01), False), ("outside_1e15", 1e15 * (1 + 0.01), True), ("inside_1e-15", 1e-15 * (1 + 0.01), False),
        ("outside_1e-15", 1e-15 * (1 - 0.01), True), ("far_above", 1e19, True), ("far_below", 1e-19, True)]
RULE_N = {"fused": 3272, "unfused": 1025}
RULE_ITERS = [1, 2, 5]
RULE_SEED = 5          # of the start vector: one for which the fused and the dense tree differ in lambda on all six matrices (tests/test_power_model_host.py)
VARIANT = "phases/short_last_workgroup"


def fused_claims():
    """name -> (options, precisions, iters): every matrix on which a GPU test claims that the one-launch step ran, with the `iters` that test runs.  The
    fused cases; the handles of the variants test (new values, the transpose); the fp32 rule's matrices (the sums of step 0 are the fused tree's even
    where the exact mode follows); banded matrices on the phases layout."""
    both = (np.float64, np.float32)
    c = {k: (v[0], both, list(range(7))) for k, v in fused_cases().items() if v[4]}
    c["variant/new_values"] = (PHASES, both, list(range(7)))
    c["variant/transposed"] = (PHASES, both, list(range(7)))
    for name, _, _ in RULE:
        c["rule/" + name] = (PHASES, (np.float32,), RULE_ITERS)
    for n in (1025, 4097):
        c[f"banded/{n}"] = (PHASES, both, list(range(7)))
    return c


def fused_claim(name, dtype):
    """(options, (n, n, row_ptr, col_idx, vals), start vector, iters) of a fused claim"""
    opt, _, iters = fused_claims()[name]
    kind, _, what = name.partition("/")
    if kind == "variant":
        mat = square(fused_cases()[VARIANT][1], dtype)
        if what == "new_values":          # the same pattern, other values
            mat = mat[:4] + (square(fused_cases()[VARIANT][1], dtype, seed=9)[4],)
        if what == "transposed":
            mat = transposed(mat[0], *mat[2:])
    elif kind == "rule":
        assert np.dtype(dtype) == np.float32
        mat = diag_dominant(RULE_N["fused"], {r[0]: r[1] for r in RULE}[what])
    elif kind == "banded":
        mat = KM.banded("nonsym", int(what), dtype)
    else:
        mat = square(fused_cases()[name][1], dtype)
    return opt, mat, start_vectors(mat[0], dtype, RULE_SEED if kind == "rule" else 0)[0][1], iters


def mirror_chunks(opt, n, rp, ci, va):
    """(the first row of every chunk, chunks per workgroup) from the CPU mirror's planner with the handle's defaults -- split_threshold = 32 S, no more
    rows in a chunk than it has slots --, for a matrix none of whose rows is cut"""
    import oraclelib as O
    S = opt["steps_per_chunk"]
    m = O.Cvr64(n, n, rp, ci, va, S, 32 * S, phases=opt["col_phases"], max_rows=64 * S, tag16=opt.get("row_tags16", 0), piece_max=opt.get("piece_max", 0))
    assert m.nshared == 0 and m.phases == opt["col_phases"], (m.nshared, m.phases)
    return m.desc[:, 0].astype(np.int64), opt["waves_per_block"]
