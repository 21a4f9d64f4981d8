"""What the derived-operation tests expect, as functions of arrays: the transposed CSR of the contract, the comparisons of handles, images, scaled
products and SpMM blocks, and the generator of the cases of tests/test_gpu_fuzz_derived.py.

The first part are the helpers test_gpu_transpose.py and test_gpu_spmv_scaled.py defined (moved here unchanged and imported back there).  The
second part are the same expectations cut so that they take arrays only: tests/test_fuzz_checks_host.py feeds them subtly wrong arrays on the CPU
and shows that each one rejects them.  The third part draws the fuzz cases: every draw is made before anything touches a GPU, so the coverage
the cases reach is a property of the generator and is asserted on the CPU as well."""
import ctypes as C
import os

import numpy as np

import cases as K
import cvr_amd
import oraclelib as O
from cvr_amd import capi


# ---- moved from test_gpu_transpose.py ----
def stable_transpose(nrows, ncols, rp, ci, va):
    """T = the CSR of A^T as the contract defines it (numpy, stable)"""
    j0, j1 = int(rp[0]), int(rp[-1])
    cols = ci[j0:j1].astype(np.int64)
    pos = j0 + np.argsort(cols, kind="stable")
    rows = np.searchsorted(rp, pos, side="right") - 1
    rpt = np.zeros(ncols + 1, dtype=np.int64)
    rpt[1:] = np.cumsum(np.bincount(cols, minlength=ncols))
    return ncols, nrows, rpt, rows.astype(np.int32), np.ascontiguousarray(va[pos]), pos


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in arrays]


def _from_device(nrows, ncols, rp, ci, va, opts, transpose=0, mutable_values=0):
    """a handle from device arrays with ANY options (CvrMatrix.from_device takes a subset)"""
    import torch
    dtype = va.dtype.type
    trp, tci, tva = _dev(rp.astype(np.int64), ci.astype(np.int32), va)
    torch.cuda.synchronize()
    H = cvr_amd.CvrMatrix.__new__(cvr_amd.CvrMatrix)
    H._h = C.c_void_p()
    H.tuning_s = 0.0
    H.f32 = dtype == np.float32
    H.dtype = np.float32 if H.f32 else np.float64
    view = capi.CsrView(nrows, ncols, trp.data_ptr(), tci.data_ptr(), tva.data_ptr(), int(H.f32), 1)
    kw = dict(opts)
    H._build(view, nrows, ncols, 0, kw.pop("steps_per_chunk", 0), kw.pop("split_threshold", 0), kw.pop("xcd_swizzle", -1), kw.pop("x_window", -1), False, 0,
             kw.pop("col_panels", -1), kw.pop("value_dict", -1), False, transpose=transpose, mutable_values=mutable_values, **kw)
    return H


TIME_FIELDS = {name for name, _ in capi.Info._fields_ if name.endswith("_s")}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _diff_keys(H, R):
    """the parts of the exported images that differ (column panels export no image: their y is compared)"""
    if H.info.col_panels > 1:
        return set()
    a, b = H.export_image(), R.export_image()
    assert sorted(a) == sorted(b)
    return {k for k in a if not (a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])))}


def assert_same_handle(H, R, remake=None):
    """every cvr_info field but the times, and the exported image bit for bit.  Interleaved images leave `target` unwritten (nothing reads it;
    not compared) and may leave gang tables unwritten: such a key may differ only when it differs between R and a second handle of R's CSR
    (remake())."""
    for name, _ in capi.Info._fields_:
        if name not in TIME_FIELDS:
            assert getattr(H.info, name) == getattr(R.info, name), name
    diff = _diff_keys(H, R) - ({"target"} if H.info.interleave else set())
    if diff:
        assert H.info.interleave and remake is not None, diff
        R2 = remake()
        loose = _diff_keys(R, R2)
        R2.close()
        assert diff <= loose <= {"target", "gbase"}, (diff, loose)


def assert_transposed_product(y, nrows, ncols, rp, ci, va, x):
    """y against numpy's A.T @ x in fp64: within 1e-12 (fp64) of sum |a x| per row of A^T; fp32 within its own rounding"""
    j0, j1 = int(rp[0]), int(rp[-1])
    rows = np.searchsorted(rp, np.arange(j0, j1), side="right") - 1
    a = va[j0:j1].astype(np.float64)
    prod = a * x.astype(np.float64)[rows]
    want = np.bincount(ci[j0:j1], weights=prod, minlength=ncols)
    scale = np.bincount(ci[j0:j1], weights=np.abs(prod), minlength=ncols)
    cnt = np.bincount(ci[j0:j1], minlength=ncols)
    tol = 1e-12 * scale if va.dtype == np.float64 else 1.2e-7 * (cnt + 2) * scale
    err = np.abs(y.astype(np.float64) - want)
    assert (err <= tol + 1e-300).all(), (np.flatnonzero(err > tol)[:5], err.max())


# ---- moved from test_gpu_spmv_scaled.py ----
def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _expect(s, y0, alpha, beta, dtype):
    """the contract in numpy: alpha and beta rounded to the type, two rounded products and a rounded sum; beta = 0 reads no y, alpha = 0 no s"""
    a, b = dtype(alpha), dtype(beta)
    with np.errstate(all="ignore"):
        if a == 0:
            return (b * y0).astype(dtype) if b != 0 else np.zeros_like(y0)
        if b == 0:
            return (a * s).astype(dtype)
        return (a * s + b * y0).astype(dtype)


# ---- the expectations of test_gpu_fuzz_derived.py on arrays ----
TOL = {np.float64: 1e-12, np.float32: 1e-5}          # of the row's sum |a x|: the CSR oracle's bounds (tests/README.md)
SENTINEL = -7.25


def images_differ(a, b):
    """the keys of two exported images (dicts of arrays: cvr_amd.CvrMatrix.export_image, or image_of_mirror) that are not equal bit for bit"""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    return {k for k in a if not (a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])))}


def assert_same_image(a, b, interleave=False, loose=frozenset()):
    """two exported images bit for bit.  An interleaved image leaves `target` unwritten (not compared) and may leave `gbase` unwritten: `loose`
    names the keys two conversions of the same CSR were seen to differ in, which is allowed for these two alone (the allowance
    test_gpu_update_values._check_update documents); the stream (`image`) is always compared."""
    allowed = {"target", "gbase"} if interleave else set()
    assert set(loose) <= allowed, (loose, allowed)
    diff = images_differ(a, b) - set(loose) - ({"target"} if interleave else set())
    assert not diff, diff


def assert_oracle(y, rp, ci, va, x, ctx=None):
    """y against the CSR oracle: every row within 1e-12 (fp64) / 1e-5 (fp32) of its sum |a x|"""
    dtype = np.dtype(va.dtype).type
    yref, absy = O.csr_spmv64(rp, ci, va, np.asarray(x, dtype=dtype))
    bad, worst = O.tol_check(y, yref, absy + 1e-30, tol=TOL[dtype])
    assert len(bad) == 0, (ctx, bad[:5], worst)


def assert_scaled(y, s, y0, alpha, beta, dtype):
    """y of cvr_spmv_scaled_device against the contract, bit for bit, s being the plain product of the same handle; beta = 0 reads no y (y0 is
    NaN there: none may come through)"""
    want = _expect(s, y0, alpha, beta, dtype)
    assert _bits_equal(y, want), (alpha, beta, np.flatnonzero(np.ascontiguousarray(y).view(dtype_bits(dtype)) != want.view(dtype_bits(dtype)))[:8])
    if dtype(beta) == 0:
        assert not np.isnan(y).any() or np.isnan(s).any(), (alpha, beta)


def dtype_bits(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def assert_spmm_block(Yall, nrows, k, columns, sentinel=SENTINEL):
    """the whole Y buffer of a cvr_spmm_device call (scratch rows included, ldy columns, pre-filled with the sentinel) against `columns`, the
    nrows x k results of cvr_spmv_device on the same handle: bit for bit, no NaN, every position beyond k untouched"""
    Y = np.ascontiguousarray(Yall[:nrows, :k])
    assert Y.shape == columns.shape, (Y.shape, columns.shape)
    for j in range(k):
        assert _bits_equal(Y[:, j], np.ascontiguousarray(columns[:, j])), ("column", j, "rows", np.flatnonzero(Y[:, j] != columns[:, j])[:8])
    assert not np.isnan(Y).any()
    assert np.all(Yall[:, k:] == sentinel), ("beyond nvec", np.argwhere(Yall[:, k:] != sentinel)[:4])


def image_of_mirror(nrows, ncols, rp, ci, va, S=16, thr=0):
    """the plain image of a CSR from the CPU mirror of the format, as a dict like export_image's: the CPU stand-in for a handle's image"""
    m = O.Cvr64(nrows, ncols, rp, ci, va, S, thr)
    return dict(image=m.image.copy(), desc=m.desc.copy(), target=m.target.copy(), shared=m.shared.copy())


# ---- the cases ----
SEEDS = (20264275, 20263313)          # the base seeds of the two tests (chosen so that the coverage conditions of test_fuzz_checks_host.py hold)
BLOCKS = 6
CASES_PER_BLOCK = 8
SMALL_VALUES = np.array([0.0, 1.0, -1.0, 0.5, 3.0, 1e-3, -7.25])
FIXED_PAIRS = [(1.0, 0.0), (2.5, 0.0), (1.0, 1.0), (-1.0, 1.0), (0.0, 3.0), (0.0, 0.0)]


def base_seed(which):
    """the base seed of test `which` (0: transpose / update / scaled, 1: SpMM); block b of a test draws from base + b.  CVR_FUZZ_SEED replaces
    it (the SpMM test takes that seed + 1000: other matrices than the first test's)"""
    env = os.environ.get("CVR_FUZZ_SEED")
    return SEEDS[which] if env is None else int(env) + 1000 * which


def cases_per_block():
    return CASES_PER_BLOCK * max(1, int(os.environ.get("CVR_FUZZ_CASES", "1")))


class Case:
    pass


def _matrix(rng):
    c = Case()
    c.nrows, c.ncols, c.rp, c.ci, va, c.srt = K.random_case(rng, max_nnz=100_000)
    c.f32 = bool(rng.integers(0, 4) == 0)
    if rng.integers(0, 3) == 0:                      # few distinct values: a handle that is not mutable takes the value dictionary
        va = rng.choice(SMALL_VALUES, size=len(va))
    c.dtype = np.float32 if c.f32 else np.float64
    c.va = va.astype(c.dtype)
    c.A = (c.nrows, c.ncols, c.rp, c.ci, c.va)
    return c


def _unrepresentable(rng):
    """a real in [-2, 2] that fp32 does not hold: the kernel has to round it to the handle's type first"""
    while True:
        a = float(rng.random() * 4 - 2)
        if a != 0 and float(np.float32(a)) != a:
            return a


def _values(rng, n, dtype):
    return (rng.random(n) * 4 - 2).astype(dtype)


def derived_cases(seed, ncases):
    """the cases of one block of test_fuzz_transpose_update_scaled: matrix, options (valid for A and for A^T: the narrower of the two shapes decides
    about column phases), new values, vectors and coefficients"""
    rng = np.random.default_rng(seed)
    for k in range(ncases):
        c = _matrix(rng)
        c.index = k
        c.opts = K.random_options(rng, min(c.nrows, c.ncols), c.srt)
        c.transposed_update = bool(rng.integers(0, 3) == 0)
        sub = np.random.default_rng([seed, k])          # (the vectors: a child generator, so the sequence of matrices and options stays what it is)
        c.v2, c.v3 = _values(sub, len(c.va), c.dtype), _values(sub, len(c.va), c.dtype)
        c.xt = (sub.random(c.nrows) * 2 - 1).astype(c.dtype)          # x of A^T
        c.x = (sub.random(c.ncols) * 2 - 1).astype(c.dtype)
        c.pairs = [FIXED_PAIRS[i] for i in sub.choice(len(FIXED_PAIRS), size=2, replace=False)] + [(_unrepresentable(sub), _unrepresentable(sub)) for _ in range(2)]
        c.sub = sub
        c.ctx = dict(seed=seed, case=k, nrows=c.nrows, ncols=c.ncols, nnz=len(c.ci), f32=c.f32, sorted=c.srt, transposed_update=c.transposed_update, opts=c.opts)
        yield c


def spmm_cases(seed, ncases):
    """the cases of one block of test_fuzz_spmm"""
    rng = np.random.default_rng(seed)
    for k in range(ncases):
        c = _matrix(rng)
        c.index = k
        c.S = int(rng.choice([4, 8, 16, 32, 64]))
        c.thr = int(rng.choice([0, 1, 7, 16, 64, 10**6]))
        c.nvec = int(rng.choice([2, 3, 4, 8, 16]))
        c.k = int(rng.integers(1, 17))
        c.ldx, c.ldy = c.k + int(rng.integers(0, 6)), c.k + int(rng.integers(0, 6))
        c.xoff, c.yoff = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        c.mutable = bool(rng.integers(0, 4) == 0)
        c.opts = dict(steps_per_chunk=c.S, split_threshold=c.thr, nvec=c.nvec)
        sub = np.random.default_rng([seed, k])
        c.X = (sub.random((c.ncols, c.k)) * 2 - 1).astype(c.dtype)
        c.v2 = _values(sub, len(c.va), c.dtype)
        c.ctx = dict(seed=seed, case=k, nrows=c.nrows, ncols=c.ncols, nnz=len(c.ci), f32=c.f32, S=c.S, thr=c.thr, nvec=c.nvec, k=c.k, ldx=c.ldx, ldy=c.ldy, xoff=c.xoff,
                     yoff=c.yoff, mutable=c.mutable)
        yield c


def all_cases():
    """every case of both tests for the seeds and counts in force: (derived cases, SpMM cases)"""
    n = cases_per_block()
    return ([c for b in range(BLOCKS) for c in derived_cases(base_seed(0) + b, n)], [c for b in range(BLOCKS) for c in spmm_cases(base_seed(1) + b, n)])


def coverage(derived, spmm):
    """what the cases reach, from the generator alone (numpy and the host planner): a dict of counts"""
    def cut(c, S, thr):
        if S <= 0 or c.nrows == 0:
            return False
        nzb = capi.plan_chunks(c.rp, S, thr)["nz_begin"]
        return bool((~np.isin(nzb[1:-1], c.rp)).any())          # a chunk starts inside a row

    def dup(c):
        rows = np.repeat(np.arange(c.nrows, dtype=np.int64), np.diff(c.rp))
        key = rows * (c.ncols + 1) + c.ci
        return len(np.unique(key)) < len(key)

    def unsorted(c):
        rows = np.repeat(np.arange(c.nrows), np.diff(c.rp))
        return len(c.ci) > 1 and bool(((np.diff(c.ci.astype(np.int64)) < 0) & (np.diff(rows) == 0)).any())

    both = derived + spmm
    o = [c.opts for c in derived]
    return dict(
        cut_rows=sum(cut(c, c.opts.get("steps_per_chunk", 0), c.opts.get("split_threshold", 0)) for c in both),
        few_rows=sum(c.nrows < 64 for c in both),
        tall=sum(c.ncols < c.nrows / 4 for c in both),
        wide=sum(c.nrows < c.ncols / 4 for c in both),
        unsorted=sum(unsorted(c) for c in both),
        duplicates=sum(dup(c) for c in both),
        empty_columns=sum(len(np.unique(c.ci)) < c.ncols for c in both),
        fp32=sum(c.f32 for c in both),
        interleaved_or_gang=sum(p.get("interleave", 0) > 0 for p in o),
        phases=sum(p.get("col_phases", 1) > 1 for p in o),
        hub=sum(p.get("hub_table", 0) > 0 for p in o),
        panels=sum(p.get("col_panels", 1) > 1 for p in o),
    )


COVERAGE_MIN = dict(cut_rows=6, few_rows=6, tall=6, wide=6, unsorted=10, duplicates=10, empty_columns=10, fp32=8, interleaved_or_gang=8, phases=4, hub=4, panels=4)
