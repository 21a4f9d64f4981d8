"""Seeded small matrices for the parity tests: the adversarial shapes of SURVEY.md section 4 (rows spanning
several chunks, chunks with fewer rows than lanes, empty rows everywhere, single row, dense row + singletons)."""
import numpy as np


def csr_from_lengths(lens, ncols, rng, dtype=np.float64, sort=True):
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(len(lens) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, ncols, size=int(rp[-1])).astype(np.int32)
    if sort:
        for r in range(len(lens)):
            ci[rp[r]:rp[r + 1]].sort()
    va = (rng.random(int(rp[-1])) * 2 - 1).astype(dtype)
    return len(lens), ncols, rp, ci, va


def cases(dtype=np.float64):
    rng = np.random.default_rng(20261002)
    out = {}
    out["empty_matrix_rows_only"] = csr_from_lengths([0] * 37, 5, rng, dtype)
    out["single_entry"] = csr_from_lengths([1], 1, rng, dtype)
    out["one_row_long"] = csr_from_lengths([5000], 300, rng, dtype)                      # one row over many chunks
    out["diag_96"] = csr_from_lengths([1] * 96, 96, rng, dtype)
    out["exact_fill"] = csr_from_lengths([8] * 64, 64, rng, dtype)                       # 512 slots = one S=8 chunk
    out["few_rows_lt_lanes"] = csr_from_lengths([300, 2, 1, 700, 3], 1000, rng, dtype)    # fewer rows than lanes
    out["leading_trailing_empty"] = csr_from_lengths([0] * 70 + [3, 0, 0, 9, 1] * 40 + [0] * 130, 500, rng, dtype)
    out["dense_row_plus_singletons"] = csr_from_lengths([1] * 500 + [20000] + [1] * 500, 4096, rng, dtype)
    out["two_giants"] = csr_from_lengths([3000, 0, 0, 4097, 5] + [2] * 50, 2048, rng, dtype)
    lens = np.minimum((rng.pareto(1.3, size=3000) + 1).astype(np.int64), 900)
    lens[rng.random(3000) < 0.25] = 0
    out["power_law_3000"] = csr_from_lengths(lens, 3000, rng, dtype)
    lens = rng.integers(0, 40, size=2000)
    out["uniform_2000"] = csr_from_lengths(lens, 777, rng, dtype)
    out["thr_edge"] = csr_from_lengths([127, 128, 129, 130, 1, 126, 2, 128, 128, 128, 128, 1], 64, rng, dtype)
    return out


# The layout table of the per-layout GPU tests (scaled product, CG, transpose, value updates, non-finite data): cvr_options by name.
LAYOUTS = dict(
    plain=dict(steps_per_chunk=16, col_panels=1, col_phases=0, hub_table=0, narrow_cols=0, interleave=0, gang=0),
    narrow=dict(steps_per_chunk=16, col_panels=1, col_phases=0, hub_table=0, narrow_cols=1),
    window=dict(steps_per_chunk=12, waves_per_block=8, x_window=2048, col_phases=0, col_panels=1),
    phases=dict(steps_per_chunk=12, waves_per_block=8, x_window=2048, col_phases=6, col_panels=1),
    phases_tags_pieces=dict(steps_per_chunk=24, waves_per_block=4, x_window=2048, col_phases=4, row_tags16=1, piece_max=8, col_panels=1),
    hub=dict(hub_table=300, steps_per_chunk=16, col_panels=1),
    hub_reorder=dict(hub_table=300, hub_reorder=1, steps_per_chunk=16, col_panels=1),
    panels=dict(col_panels=3, steps_per_chunk=16),
    interleaved=dict(col_panels=1, interleave=1, steps_per_chunk=32, waves_per_block=4),
    interleaved_panels=dict(col_panels=8, interleave=1),
    gang=dict(col_panels=1, interleave=1, steps_per_chunk=32, waves_per_block=4, gang=1),
    gang_tags=dict(col_panels=1, interleave=1, steps_per_chunk=16, waves_per_block=2, gang=1, row_tags16=1),
    nvec=dict(nvec=4),
)
ALL_LAYOUTS = dict(LAYOUTS, default={})


# ---- non-finite data: which entries to poison, and what class every row of y must then have ----
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
FILLS = (np.inf, np.nan, -np.inf)


def poison_patterns(nrows, ncols, rp, ci, rng):
    """named (columns, fill) sets -- the entries of x to make non-finite, fill cycling +Inf, NaN, -Inf: the neighbour of the pad element, column 0,
    the columns a hub table stages, columns read once, the edges of an x window of 2048, and 2 % of the columns at random.  Empty sets are left out."""
    cnt = np.bincount(ci[int(rp[0]):int(rp[-1])], minlength=ncols)[:ncols] if ncols else np.zeros(0, dtype=np.int64)
    sets = [("last_col", [ncols - 1]), ("first_col", [0]),
            ("hot", np.argsort(-cnt, kind="stable")[: min(8, ncols)]),
            ("cold", np.flatnonzero(cnt == 1)[:8]),
            ("window_edges", [c for c in (2047, 2048, 4095, 4096) if c < ncols]),
            ("random2pct", np.sort(rng.choice(ncols, size=min(ncols, max(1, ncols // 50)), replace=False)) if ncols else [])]
    for name, cols in sets:
        cols = np.asarray(cols, dtype=np.int64)
        if ncols > 0 and len(cols):
            yield name, cols, np.array([FILLS[i % 3] for i in range(len(cols))])


def poisoned(x, cols, fill):
    """(x with x[cols] = fill, x with x[cols] = 0)"""
    xp, x0 = np.array(x, copy=True), np.array(x, copy=True)
    xp[cols] = fill.astype(xp.dtype)
    x0[cols] = 0
    return xp, x0


def classify(y):
    """FINITE / POS_INF / NEG_INF / NAN per value"""
    y = np.asarray(y)
    return np.where(np.isnan(y), NAN, np.where(y == np.inf, POS_INF, np.where(y == -np.inf, NEG_INF, FINITE))).astype(np.int8)


def expected_class(rp, ci, va, x):
    """the class of every row of A x from its terms t_k = a_k * x[c_k], formed in the type of va: NAN if a term is NaN or +Inf and -Inf both occur,
    else POS_INF / NEG_INF if such a term occurs, else FINITE.  Independent of the order of the additions as long as no finite sum overflows
    (the suite's finite data lies in [-1, 1] or in the fuzz's small value set)."""
    nrows = len(rp) - 1
    j0, j1 = int(rp[0]), int(rp[-1])
    with np.errstate(all="ignore"):
        t = np.asarray(va)[j0:j1] * np.asarray(x, dtype=np.asarray(va).dtype)[ci[j0:j1]]
    rows = np.repeat(np.arange(nrows), np.diff(rp))

    def any_in_row(mask):
        return np.bincount(rows[mask], minlength=nrows)[:nrows] > 0 if nrows else np.zeros(0, dtype=bool)
    nan, pos, neg = any_in_row(np.isnan(t)), any_in_row(t == np.inf), any_in_row(t == -np.inf)
    return np.where(nan | (pos & neg), NAN, np.where(pos, POS_INF, np.where(neg, NEG_INF, FINITE))).astype(np.int8)
