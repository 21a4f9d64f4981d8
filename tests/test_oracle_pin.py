"""The checker every GPU test calls (orc_csr_spmv64, tests/oraclelib.csr_spmv64) is the pinned oracle (orc_csr_spmv = the reference's
CSR self-check loop, spmv.cpp:1843-1850, pinned by tests/golden/*.npz) bit for bit, and the product's own host loop (cvr_csr_spmv_host,
which spmv.cvr's verdict uses) equals the reference's y on the fixtures.  The same checks run on the CPU and -- marked gpu -- on the GPU
box, so that the box pins what its parity tests rely on."""
import glob
import os

import numpy as np
import pytest

import cvr_amd
import oraclelib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz")))


def _oracle64_is_the_pinned_oracle(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    numRows = int(z["dims"][1])
    rp, ci, va = z["csr_rowptr"][: numRows + 1].astype(np.int64), z["csr_col"], z["csr_val"]
    for mode in ("ones", "rand"):
        x = z[f"x_{mode}"]
        y64, absy = O.csr_spmv64(rp, ci, va, x)
        assert np.array_equal(y64.view(np.uint64), z[f"y_csr_{mode}"][:numRows].view(np.uint64)), (name, mode)      # == the reference's own y
        y32 = np.zeros(numRows, dtype=np.float64)
        rp32, ci32 = np.ascontiguousarray(z["csr_rowptr"], dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)      # (kept alive across the call)
        va64, x64 = np.ascontiguousarray(va, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
        O.lib().orc_csr_spmv(numRows, rp32.ctypes.data, ci32.ctypes.data, va64.ctypes.data, x64.ctypes.data, y32.ctypes.data)
        assert np.array_equal(y64.view(np.uint64), y32.view(np.uint64)), (name, mode)
        assert np.all(absy >= np.abs(y64) * (1 - 1e-15))


def _host_loop_is_the_reference_loop(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    numRows = int(z["dims"][1])
    for mode, code in (("ones", 0), ("rand", 1)):
        x = z[f"x_{mode}"]
        assert np.array_equal(cvr_amd.fill_x(len(x), code), x)
        y = cvr_amd.csr_spmv_host(z["csr_rowptr"][: numRows + 1], z["csr_col"], z["csr_val"], x, nthreads=2)
        assert np.array_equal(y.view(np.uint64), z[f"y_csr_{mode}"].view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_oracle64_equals_pinned_oracle(name):
    _oracle64_is_the_pinned_oracle(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_oracle64_equals_pinned_oracle_on_the_gpu_box(name):
    _oracle64_is_the_pinned_oracle(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_csr_loop_equals_reference_on_the_gpu_box(name):
    _host_loop_is_the_reference_loop(name)


# ---- the shared row checker (oraclelib.tol_check): non-finite rows ----
def _tol_check_before(y, yref, absy, tol=1e-12):
    """the checker as it was (NaN-blind: `err > bound` is false for a NaN err); the new one must equal it on finite data"""
    err = np.abs(np.asarray(y, dtype=np.float64) - yref)
    bound = tol * absy + 1e-300
    bad = np.nonzero(err > bound)[0]
    return bad, (err / np.maximum(absy, 1e-300)).max() if len(err) else 0.0


def test_tol_check_non_finite_rows():
    nan, inf = np.nan, np.inf
    absy = np.array([1.0, 2.0, 3.0])
    bad, worst = O.tol_check([nan, 2, inf], [1, 2, 3], absy)
    assert bad.tolist() == [0, 2] and worst == inf                       # NaN or Inf against finite is bad
    bad, worst = O.tol_check([nan, 2.0, 3.0], [nan, 2.0, 3.0], absy)
    assert bad.tolist() == [] and worst == 0.0                           # NaN against NaN is good
    bad, worst = O.tol_check([inf, -inf, 3.0], [inf, -inf, 3.0], absy)
    assert bad.tolist() == [] and worst == 0.0                           # the same signed infinity is good
    bad, worst = O.tol_check([inf, -inf, 3.0], [-inf, inf, 3.0], absy)
    assert bad.tolist() == [0, 1] and worst == inf                       # +Inf against -Inf is bad
    bad, worst = O.tol_check([1.0, nan, inf], [nan, inf, nan], absy)
    assert bad.tolist() == [0, 1, 2] and worst == inf                    # finite against NaN, NaN against Inf, Inf against NaN
    # sum |a x| of a poisoned row is itself Inf or NaN: the bound is not finite, the rule still holds
    for a in (inf, nan):
        absy = np.array([a, a, a, a, 1.0])
        bad, worst = O.tol_check([1.0, nan, inf, nan, 5.0], [inf, 1.0, inf, nan, 5.0], absy)
        assert bad.tolist() == [0, 1] and worst == inf, a
        bad, worst = O.tol_check([nan, nan, -inf, inf, 5.0], [nan, nan, -inf, inf, 5.0], absy)
        assert bad.tolist() == [] and not np.isnan(worst), a
    # a finite wrong row among good non-finite ones: worst is that row's, not nan
    bad, worst = O.tol_check([nan, 2.5, inf], [nan, 2.0, inf], np.array([1.0, 2.0, 3.0]))
    assert bad.tolist() == [1] and worst == 0.25


def test_tol_check_empty_arrays():
    e = np.zeros(0)
    bad, worst = O.tol_check(e, e, e)
    assert len(bad) == 0 and worst == 0.0
    bad, worst = O.tol_check(e.astype(np.float32), e, e, tol=1e-5)
    assert len(bad) == 0 and worst == 0.0


def test_tol_check_unchanged_on_finite_data():
    """finite inputs: the same bad rows and the same worst figure, bit for bit, as before -- random rows, rows exactly at the bound (good),
    one ulp-scale step beyond it (bad), rows with sum |a x| = 0"""
    rng = np.random.default_rng(20261017)
    tol = 2.0 ** -20
    for n in (1, 7, 1000):
        yref = rng.integers(-1, 2, size=n).astype(np.float64)
        absy = np.ones(n)                                                # bound = 2^-20 (+ 1e-300, absorbed): y = yref + 2^-20 is exact
        step = rng.choice([0.0, 2.0 ** -21, 2.0 ** -20, 2.0 ** -20 + 2.0 ** -50, -(2.0 ** -20), -(2.0 ** -20) - 2.0 ** -50, 2.0 ** -10], size=n)
        y = yref + step
        assert np.array_equal(np.abs(y - yref), np.abs(step))            # (the rows at the bound sit exactly on it)
        got, want = O.tol_check(y, yref, absy, tol=tol), _tol_check_before(y, yref, absy, tol=tol)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        assert np.array_equal(got[0], np.flatnonzero(np.abs(step) > tol))
        for t in (1e-12, 1e-5):                                          # random data at the suite's tolerances, fp32 y included
            yref = rng.standard_normal(n)
            absy = np.abs(yref) * rng.uniform(1, 5, n)
            absy[rng.random(n) < 0.1] = 0.0
            y = yref + absy * t * rng.choice([0.0, 0.5, 0.999, 1.001, 2.0, -3.0], size=n) + (rng.random(n) < 0.05) * 1e-200
            for yy in (y, y.astype(np.float32)):
                got, want = O.tol_check(yy, yref, absy, tol=t), _tol_check_before(yy, yref, absy, tol=t)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (n, t)
