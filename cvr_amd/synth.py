"""Seeded synthetic stand-ins for the matrices BASELINE.json names (there is no network: the real
SuiteSparse / SNAP files are used instead when CVR_DATA_DIR holds them).  SURVEY.md 8(d).

All generators return 0-based CSR: (nrows, ncols, row_ptr int64, col_idx int32, vals) with the entries of a
row sorted by column, no duplicates.
"""
import os

import numpy as np

WEB_GOOGLE = dict(n=916_428, nnz=5_105_039, empty_frac=0.193, max_deg=456, seed=20261002)
LIVEJOURNAL = dict(n=4_847_571, nnz=68_993_773, empty_frac=0.11, max_deg=20_293, seed=20261003)


def _coo_to_csr(n, rows, cols, nnz_target=None, rng=None):
    """sort by (row, col), drop duplicates, trim to nnz_target by dropping random entries"""
    key = rows.astype(np.int64) * np.int64(n) + cols.astype(np.int64)
    key = np.unique(key)
    if nnz_target is not None and len(key) > nnz_target:
        drop = rng.choice(len(key), size=len(key) - nnz_target, replace=False)
        keep = np.ones(len(key), dtype=bool)
        keep[drop] = False
        key = key[keep]
    r = (key // n).astype(np.int64)
    c = (key % n).astype(np.int32)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rp, c


def power_law_graph(n, nnz, empty_frac, max_deg, seed, alpha=2.1, local_frac=0.5, local_scale=2000.0, pattern_values=True):
    """Web-graph-like square matrix: Zipf-like out-degrees (rows) with a share of empty rows; half of the
    columns drawn by popularity (power-law in-degree), half near the diagonal (host locality).
    pattern_values: value = (file-order index) % 13, as the reference assigns to `pattern` files
    (spmv.cpp:417); row-major order stands in for the file order."""
    rng = np.random.default_rng(seed)
    nonempty = rng.random(n) >= empty_frac
    k = int(nonempty.sum())
    over = 1.03                                       # duplicates are dropped later
    # discrete power-law degrees >= 1, truncated at max_deg, rescaled to the target mean
    u = rng.random(k)
    deg = np.floor((1.0 - u) ** (-1.0 / (alpha - 1.0))).astype(np.int64)
    deg = np.clip(deg, 1, max_deg)
    want = int(nnz * over)
    scale = want / deg.sum()
    deg = np.clip(np.maximum(1, np.rint(deg * scale)).astype(np.int64), 1, max_deg)
    diff = want - int(deg.sum())
    if diff > 0:                                      # top up on random rows
        idx = rng.integers(0, k, size=diff)
        np.add.at(deg, idx, 1)
        deg = np.clip(deg, 1, max_deg)
    rows_ne = np.nonzero(nonempty)[0]
    rows = np.repeat(rows_ne, deg)
    m = len(rows)
    # columns
    is_local = rng.random(m) < local_frac
    off = np.rint(rng.laplace(0.0, local_scale, size=m)).astype(np.int64)
    loc = np.clip(rows + off, 0, n - 1)
    # popularity: column rank ~ power law, then a fixed permutation scatters the hubs
    pr = rng.random(m)
    rank = np.floor(n * pr ** 2.6).astype(np.int64)   # density ~ rank^(-0.615): heavy head
    perm = rng.permutation(n)
    pop = perm[np.clip(rank, 0, n - 1)]
    cols = np.where(is_local, loc, pop)
    rp, ci = _coo_to_csr(n, rows, cols, nnz_target=nnz, rng=rng)
    if pattern_values:
        vals = (np.arange(len(ci), dtype=np.int64) % 13).astype(np.float64)
    else:
        vals = rng.random(len(ci)) * 2.0 - 1.0
    return n, n, rp, ci, vals


def web_google_like(scale=1.0, seed=None):
    """916 428 x 916 428, 5 105 039 nnz, ~19 % empty rows, max out-degree 456 (the real web-Google's shape);
    `scale` < 1 shrinks rows and nnz together for quick tests."""
    p = dict(WEB_GOOGLE)
    if seed is not None:
        p["seed"] = seed
    n = max(64, int(p["n"] * scale))
    nnz = max(64, int(p["nnz"] * scale))
    return power_law_graph(n, nnz, p["empty_frac"], min(p["max_deg"], n // 2), p["seed"])


def livejournal_like(scale=1.0, seed=None):
    p = dict(LIVEJOURNAL)
    if seed is not None:
        p["seed"] = seed
    n = max(64, int(p["n"] * scale))
    nnz = max(64, int(p["nnz"] * scale))
    return power_law_graph(n, nnz, p["empty_frac"], min(p["max_deg"], n // 2), p["seed"], alpha=1.9, local_scale=50000.0)


def rmat(scale, edge_factor=16, a=0.57, b=0.19, c=0.19, seed=1, dtype=np.float32, dedupe=False):
    """R-MAT (Graph500 parameters): 2^scale vertices, edge_factor * 2^scale edges, duplicates kept (summed
    order = generation order is not kept: entries of a row are sorted by column)."""
    rng = np.random.default_rng(seed)
    n = 1 << scale
    m = edge_factor * n
    rows = np.zeros(m, dtype=np.int64)
    cols = np.zeros(m, dtype=np.int64)
    ab, abc = a + b, a + b + c
    for lvl in range(scale):
        r = rng.random(m)
        rbit = r >= ab
        cbit = ((r >= a) & (r < ab)) | (r >= abc)
        rows |= rbit.astype(np.int64) << lvl
        cols |= cbit.astype(np.int64) << lvl
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    if dedupe:
        keep = np.ones(m, dtype=bool)
        keep[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        rows, cols = rows[keep], cols[keep]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    vals = rng.random(len(rows)).astype(dtype)
    return n, n, rp, cols.astype(np.int32), vals


def banded_sym(n, half_band=13, seed=7, dtype=np.float64):
    """KKT-like banded symmetric pattern (~2*half_band+1 nnz per row): the stand-in for nlpkkt240's shape"""
    rng = np.random.default_rng(seed)
    offs = np.arange(-half_band, half_band + 1, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), len(offs))
    cols = rows + np.tile(offs, n)
    ok = (cols >= 0) & (cols < n)
    rows, cols = rows[ok], cols[ok]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    vals = (rng.random(len(rows)) * 2 - 1).astype(dtype)
    return n, n, rp, cols.astype(np.int32), vals


def rect_banded(m, n, half_band=2, extra=0, seed=17, dtype=np.float64):
    """An m x n least-squares test matrix of full rank min(m, n) (the LSQR probe's shapes): row i has a dominant entry in [1, 2) at its
    diagonal-like column d_i = i * n // m (m >= n; i itself when m < n), entries in [-0.5, 0.5) / (2 half_band + extra) at the columns
    d_i - half_band .. d_i + half_band that exist, and `extra` more of them at random columns (duplicates dropped).  Columns of a row
    ascending.  Returns (m, n, row_ptr, col_idx, vals) like the generators above."""
    rng = np.random.default_rng(seed)
    i = np.arange(m, dtype=np.int64)
    d = i * n // m if m >= n else i
    offs = np.arange(-half_band, half_band + 1, dtype=np.int64)
    rows = np.concatenate([np.repeat(i, len(offs)), np.repeat(i, extra)])
    cols = np.concatenate([(d[:, None] + offs[None, :]).reshape(-1), rng.integers(0, n, size=m * extra)])
    ok = (cols >= 0) & (cols < n)
    key, first = np.unique(rows[ok] * np.int64(n) + cols[ok], return_index=True)
    r, c = key // n, key % n
    vals = (rng.random(len(key)) - 0.5) / max(2 * half_band + extra, 1)
    on = c == d[r]
    vals[on] = 1.0 + rng.random(int(on.sum()))
    rp = np.zeros(m + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(r, minlength=m))
    return m, n, rp, c.astype(np.int32), vals.astype(dtype)


def spd_from_pattern(n, rp, ci, c=0.5, dscale=None, dtype=np.float64):
    """A symmetric positive definite matrix with a known condition bound from any square pattern (the solver's test matrices):
    W = P u P^T without the diagonal and without duplicates, d_i = the degree of vertex i in W, A = I + c D^-1/2 W D^-1/2.  The normalised
    adjacency has its spectrum in [-1, 1], so A's lies in [1 - c, 1 + c] -- kappa(A) <= 3 for c = 0.5 whatever the degrees, isolated
    vertices (rows with the diagonal alone) included.  dscale = s (n positive values): S A S instead, badly conditioned as s spreads, whose
    Jacobi preconditioner 1 / s^2 (the inverse of its diagonal) gives A's spectrum back.  Entries are computed in fp64 and symmetric bit for
    bit (also after rounding to dtype).  Returns (n, n, row_ptr, col_idx, vals) like the generators above."""
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[: rp[-1]], dtype=np.int64)
    off = rows != cols
    rows, cols = rows[off], cols[off]
    key = np.unique(np.concatenate([rows * np.int64(n) + cols, cols * np.int64(n) + rows]))
    wr, wc = key // n, key % n
    deg = np.bincount(wr, minlength=n).astype(np.float64)
    wv = c / np.sqrt(deg[wr] * deg[wc])
    diag = np.arange(n, dtype=np.int64)
    key = np.concatenate([key, diag * np.int64(n) + diag])
    val = np.concatenate([wv, np.ones(n)])
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    r, cc = key // n, key % n
    if dscale is not None:
        s = np.asarray(dscale, dtype=np.float64)
        val = (s[r] * s[cc]) * val
    out_rp = np.zeros(n + 1, dtype=np.int64)
    out_rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return n, n, out_rp, cc.astype(np.int32), val.astype(dtype)


def laplacian_2d(m, dtype=np.float64):
    """The 5-point Laplacian of an m x m grid with Dirichlet boundaries (n = m * m rows, 4 on the diagonal, -1 to the grid neighbours): the model
    problem whose CG iteration count grows with the mesh.  Its spectrum is 4 - 2 cos(i pi / (m + 1)) - 2 cos(j pi / (m + 1)), i, j = 1 .. m.
    Returns (n, n, row_ptr, col_idx, vals) like the generators above, the columns of a row ascending."""
    n = m * m
    i, j = np.divmod(np.arange(n, dtype=np.int64), m)
    rows, cols, vals = [], [], []
    for ok, off, v in ((i > 0, -m, -1.0), (j > 0, -1, -1.0), (np.ones(n, dtype=bool), 0, 4.0), (j < m - 1, 1, -1.0), (i < m - 1, m, -1.0)):
        r = np.flatnonzero(ok)
        rows.append(r)
        cols.append(r + off)
        vals.append(np.full(len(r), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, n, rp, cols[order].astype(np.int32), vals[order].astype(dtype)


def upwind_2d(m, cx=-0.5, cy=-0.25, dtype=np.float64):
    """Convection-diffusion on an m x m grid with Dirichlet boundaries, first-order upwind: diffusion 1 (the 5-point Laplacian above) plus the
    convection (bx, by) . grad u with cx = bx h and cy = by h.  Row: 4 + |cx| + |cy| on the diagonal, -1 to the four grid neighbours and -|cx|, -|cy|
    more to the upwind one in each direction: for cx > 0 the west neighbour (j - 1), for cx < 0 the east one (j + 1); cy likewise with i.
    Nonsymmetric for cx or cy != 0 and weakly diagonally dominant by rows for every cx, cy.  The default flow goes towards the smaller indices, so
    the extra weight lies in the UPPER triangle: the plain-aggregation AMG set-up inverts its coarsest matrix by an LDL^T that reads the lower
    triangle, which then is the Laplacian's and has positive pivots; with cx, cy > 0 it reads the heavier triangle and declines the matrix.
    Returns (n, n, row_ptr, col_idx, vals), the columns of a row ascending."""
    n = m * m
    i, j = np.divmod(np.arange(n, dtype=np.int64), m)
    rows, cols, vals = [], [], []
    for ok, off, v in ((i > 0, -m, -1.0 - max(cy, 0.0)), (j > 0, -1, -1.0 - max(cx, 0.0)), (np.ones(n, dtype=bool), 0, 4.0 + abs(cx) + abs(cy)),
                       (j < m - 1, 1, -1.0 - max(-cx, 0.0)), (i < m - 1, m, -1.0 - max(-cy, 0.0))):
        r = np.flatnonzero(ok)
        rows.append(r)
        cols.append(r + off)
        vals.append(np.full(len(r), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, n, rp, cols[order].astype(np.int32), vals[order].astype(dtype)


def block_diag_spd(n, bs, cond=1e3, seed=11, dtype=np.float64):
    """An exactly block-diagonal symmetric positive definite matrix (the block-Jacobi preconditioner's test family): dense blocks of bs rows (the last
    one shorter when bs does not divide n), each Q diag(lambda) Q^T with a random orthogonal Q and eigenvalues spread log-uniformly over [1, cond] --
    both ends in every block, the others drawn per block, so the matrix has about n distinct eigenvalues and plain CG needs many steps while
    block-Jacobi with the same bs solves it in one.  Symmetric bit for bit.  Returns (n, n, row_ptr, col_idx, vals) like the generators above."""
    rng = np.random.default_rng(seed)
    nb = -(-n // bs)
    q, _ = np.linalg.qr(rng.standard_normal((nb, bs, bs)))
    lam = cond ** rng.random((nb, bs))
    lam[:, 0], lam[:, -1] = 1.0, cond
    blocks = np.einsum("kij,kj,klj->kil", q, lam, q)
    blocks = 0.5 * (blocks + blocks.transpose(0, 2, 1))
    rows = np.repeat(np.arange(nb * bs, dtype=np.int64), bs)
    cols = (rows // bs) * bs + np.tile(np.arange(bs, dtype=np.int64), nb * bs)
    vals = blocks.reshape(-1)
    ok = (rows < n) & (cols < n)
    rows, cols, vals = rows[ok], cols[ok], vals[ok]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, n, rp, cols.astype(np.int32), vals.astype(dtype)


def block_diag_nonsym(n, bs, cond=1e3, seed=13, dtype=np.float64):
    """The nonsymmetric sibling of block_diag_spd (the test family of the preconditioned BiCGSTAB and GMRES): exactly block-diagonal, dense blocks of bs
    rows (the last one shorter when bs does not divide n), each U diag(sigma) V^T with independent random orthogonal U and V and singular values spread
    log-uniformly over [1, cond] -- both ends in every block, so every block is nonsingular with condition cond, and not symmetric.  A short last block
    is a block of its own size, built the same way.  Returns (n, n, row_ptr, col_idx, vals) like the generators above."""
    rng = np.random.default_rng(seed)
    nb, last = -(-n // bs), n % bs
    rows, cols, vals = [], [], []

    def blocks_of(count, m, first_row):
        if count == 0:
            return
        u, _ = np.linalg.qr(rng.standard_normal((count, m, m)))
        v, _ = np.linalg.qr(rng.standard_normal((count, m, m)))
        sig = cond ** rng.random((count, m))
        sig[:, 0] = 1.0
        sig[:, -1] = cond if m > 1 else 1.0
        blk = np.einsum("kij,kj,klj->kil", u, sig, v)
        r = first_row + np.repeat(np.arange(count * m, dtype=np.int64), m)
        rows.append(r)
        cols.append(first_row + ((r - first_row) // m) * m + np.tile(np.arange(m, dtype=np.int64), count * m))
        vals.append(blk.reshape(-1))

    full = nb - (1 if last else 0)
    blocks_of(full, bs, 0)
    blocks_of(1 if last else 0, last, full * bs)
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, n, rp, cols.astype(np.int32), vals.astype(dtype)


def nonsym_from_pattern(n, rp, ci, c=0.5, rscale=None, seed=3, dtype=np.float64):
    """A nonsymmetric, strictly diagonally dominant matrix from any square pattern (the BiCGSTAB solver's test matrices): W = the pattern as
    it is (not symmetrised) without the diagonal and without duplicates, with seeded weights in [0.5, 1.5) and each row scaled to the absolute
    sum c; A = I - W.  Gershgorin puts A's spectrum into the disc |z - 1| <= c, so A is nonsingular for c < 1, and it is nonsymmetric in
    pattern (wherever the pattern is) and in values; rows without an off-diagonal entry hold the diagonal alone.  rscale = s (n positive
    values): diag(s) A instead, badly scaled by rows as s spreads, whose Jacobi preconditioner is 1 / s (the inverse of its diagonal).
    Entries are computed in fp64, then rounded to dtype.  Returns (n, n, row_ptr, col_idx, vals) like the generators above."""
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci[: rp[-1]], dtype=np.int64)
    off = rows != cols
    key = np.unique(rows[off] * np.int64(n) + cols[off])
    wr = key // n
    w = 0.5 + np.random.default_rng(seed).random(len(key))
    rowsum = np.bincount(wr, weights=w, minlength=n)
    wv = -c * w / rowsum[wr]
    diag = np.arange(n, dtype=np.int64)
    key = np.concatenate([key, diag * np.int64(n) + diag])
    val = np.concatenate([wv, np.ones(n)])
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    r, cc = key // n, key % n
    if rscale is not None:
        val = np.asarray(rscale, dtype=np.float64)[r] * val
    out_rp = np.zeros(n + 1, dtype=np.int64)
    out_rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return n, n, out_rp, cc.astype(np.int32), val.astype(dtype)


def x_rand(n, dtype=np.float64):
    """splitmix64(0xC0FFEE, j) -> uniform [-1, 1): identical to cvr_fill_x(mode 1) and the oracle's orc_x_rand"""
    j = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(0xC0FFEE) + (j + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) * 2.0 - 1.0).astype(dtype)


def b_alg(nrows, ncols, nnz, vbytes=8):
    """algorithmic bytes of one SpMV, each array touched once"""
    return nnz * (vbytes + 4) + (nrows + 1) * 4 + ncols * vbytes + nrows * vbytes


def to_refcompat(nrows, ncols, rp, ci, vals):
    """0-based CSR -> the reference loader's 1-based int arrays as it would have
    produced them from a Matrix-Market file of these entries: nnz padded to a multiple of 16 with zero copies
    of the last entry, rowptr[numRows+2] with tail = nItems-1.  For bench.py's CPU baseline."""
    nnz = len(ci)
    npad = nnz if nnz % 16 == 0 else (nnz + 16) // 16 * 16
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rp))
    last_r, last_c = int(rows[-1]), int(ci[-1])
    cols1 = np.concatenate([ci.astype(np.int32) + 1, np.full(npad - nnz, last_c + 1, dtype=np.int32)])
    v = np.concatenate([np.asarray(vals, dtype=np.float32).astype(np.float64), np.zeros(npad - nnz)])
    cnt = np.bincount(rows, minlength=nrows).astype(np.int64)
    cnt[last_r] += npad - nnz
    # the pads (same coordinates as the last entry) sort to the end of the last non-empty row
    rp1 = np.zeros(nrows + 2, dtype=np.int64)      # 1-based rows: row 0 is empty (Q1)
    rp1[2:] = np.cumsum(cnt)
    rp1[last_r + 2:] = npad - 1                    # Q9: row pointers after the last non-empty row
    return dict(nItems=npad, nItemsRaw=nnz, numRows=nrows, numCols=ncols, val=v, cols=cols1, rowptr=rp1.astype(np.int32))


def data_file(name):
    d = os.environ.get("CVR_DATA_DIR")
    if d and os.path.exists(os.path.join(d, name)):
        return os.path.join(d, name)
    return None
