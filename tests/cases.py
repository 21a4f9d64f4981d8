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


def random_case(rng, max_nnz=400_000):
    """one matrix of the fuzz tests: 1 .. 3999 rows, 1 .. 5999 columns, row lengths uniform, power-law, a few giants, constant or mostly empty, at most
    about max_nnz entries, rows sorted or not: (nrows, ncols, row_ptr, col_idx, vals, sorted).  With the default max_nnz it consumes the generator
    exactly as the loops of test_gpu_fuzz.py always did (tests/test_fuzz_checks_host.py pins a digest of its cases)."""
    kind = rng.integers(0, 5)
    nrows = int(rng.integers(1, 4000))
    ncols = int(rng.integers(1, 6000))
    if kind == 0:
        lens = rng.integers(0, 12, size=nrows)
    elif kind == 1:
        lens = np.minimum((rng.pareto(1.1, size=nrows) + 0.5).astype(np.int64), 3000)
    elif kind == 2:
        lens = np.zeros(nrows, dtype=np.int64)
        lens[rng.integers(0, nrows, size=max(1, nrows // 50))] = rng.integers(1, 5000, size=max(1, nrows // 50))
    elif kind == 3:
        lens = np.full(nrows, int(rng.integers(1, 70)))
    else:
        lens = rng.integers(0, 3, size=nrows) * rng.integers(0, 40, size=nrows)
    lens = np.asarray(lens, dtype=np.int64)
    if lens.sum() > max_nnz:
        lens = lens // (lens.sum() // max_nnz + 1)
    srt = bool(rng.integers(0, 2))
    return csr_from_lengths(lens, ncols, rng, sort=srt) + (srt,)


def random_options(rng, ncols, sorted_rows):
    """CvrMatrix keyword options drawn as the two loops of test_gpu_fuzz.py draw them, for a matrix of `ncols` columns whose rows are sorted or not:
    one time in eight the defaults ({}), four in eight the draw of test_fuzz_parity (chunk length, split threshold, panels, window, wavefronts per
    workgroup, column phases, hub table, re-ordered x, tags, piece limit, swizzle), three in eight the draw of test_fuzz_interleaved_chunks
    (interleaved and gang chunks).  The guards are those loops': column phases only on one panel, from 320 columns on and with sorted rows (the
    library refuses them on a row whose columns descend), a hub table only without phases, re-ordered x only with a hub table on one panel, tags
    and piece limit only with phases."""
    family = int(rng.integers(0, 8))
    if family == 0:
        return {}
    if family <= 4:
        S = int(rng.choice([4, 8, 12, 16, 32, 64, 96, 128]))
        thr = int(rng.choice([0, 1, 7, 64, 10**6]))
        P = int(rng.choice([1, 1, 2, 3]))
        win = int(rng.choice([0, 0, 64, 1000]))
        wpb = int(rng.choice([1, 1, 2, 8, 16]))
        ph = int(rng.choice([1, 1, 2, 5])) if P == 1 and ncols >= 320 and sorted_rows else 1
        hub = int(rng.choice([0, 0, 7, 300])) if ph == 1 else 0
        reo = int(rng.integers(0, 2)) if hub and P == 1 else 0
        tags = int(rng.choice([-1, 0, 1])) if ph > 1 else -1
        pmax = int(rng.choice([-1, 0, 2, 8])) if ph > 1 else -1
        swz = int(rng.choice([-1, -1, 0, 3, 4, 5, 6]))
        return dict(steps_per_chunk=S, split_threshold=thr, col_panels=P, x_window=win, waves_per_block=wpb, col_phases=ph, hub_table=hub, hub_reorder=reo,
                    row_tags16=tags, piece_max=pmax, xcd_swizzle=swz)
    S = int(rng.choice([4, 8, 16, 32, 64, 128, 256, 508]))
    P = int(rng.choice([1, 1, 1, 2, 3, 8]))
    wpb = int(rng.choice([0, 1, 2, 4, 8]))
    tags = int(rng.choice([-1, -1, 0, 1]))          # (0 is refused only where column and row do not fit one word: never below 2^13 columns)
    gang = int(rng.integers(0, 2))
    return dict(steps_per_chunk=S, col_panels=P, waves_per_block=wpb, row_tags16=tags, interleave=1, gang=gang)


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
