"""CPU: the error paths of cvr_amd/capi.py that need no device, on CSR arrays of n = 4 -- the ValueError of short col_idx / vals from every host-array
constructor of Precond and every host helper, raised before the library is loaded; amg_block's setup string; `which` of eigsh_host and lobpcg_host; the
lengths of b, x0 and v0; and a build the C side rejects in its argument checks (a negative n, block_size = 0, sweeps = 0, nvec = 0, degree = 0, a bad
option or omega: all answered before the handle or a device is looked at), which leaves _p null and raises CvrError naming the C entry that was called."""
import ctypes as C
import types

import numpy as np
import pytest

from cvr_amd import capi

N = 4
RP = np.array([0, 2, 4, 6, 8], dtype=np.int64)
CI = np.array([0, 1, 0, 1, 2, 3, 2, 3], dtype=np.int32)
VA = np.array([4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0])
MATRIX = types.SimpleNamespace(_h=C.c_void_p(1))          # a handle that is never looked at

HOST_CONSTRUCTORS = {"block_jacobi": lambda P, *a: P.block_jacobi(*a, 2), "ilu0": lambda P, *a: P.ilu0(*a), "ilu0_jacobi": lambda P, *a: P.ilu0_jacobi(*a, 2),
                     "mcsgs": lambda P, *a: P.mcsgs(*a), "fsai": lambda P, *a: P.fsai(*a), "amg": lambda P, *a: P.amg(MATRIX, *a),
                     "amg_smoothed": lambda P, *a: P.amg_smoothed(MATRIX, *a), "amg_mis2": lambda P, *a: P.amg_mis2(MATRIX, *a),
                     "amg_block": lambda P, *a: P.amg_block(MATRIX, *a, 2)}
HOST_HELPERS = {"fsai_factor_host": capi.fsai_factor_host, "amg_setup_host": capi.amg_setup_host, "amg_smoothed_setup_host": capi.amg_smoothed_setup_host,
                "amg_mis2_setup_host": capi.amg_mis2_setup_host, "amg_mis2_aggregate_host": capi.amg_mis2_aggregate_host}
SHORT = {"col_idx": (CI[:7], VA, "col_idx / vals hold 7 / 8 entries, row_ptr[nrows] = 8"), "vals": (CI, VA[:5], "col_idx / vals hold 8 / 5 entries, row_ptr[nrows] = 8")}


def _no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was asked for before the arrays were checked")
    monkeypatch.setattr(capi, "lib", boom)


@pytest.mark.parametrize("short", sorted(SHORT))
@pytest.mark.parametrize("name", sorted(HOST_CONSTRUCTORS))
def test_short_arrays_raise_the_same_text_from_every_constructor_before_the_library_loads(monkeypatch, name, short):
    ci, va, text = SHORT[short]
    _no_library(monkeypatch)
    for vals in (va, va.astype(np.float32)):
        with pytest.raises(ValueError) as e:
            HOST_CONSTRUCTORS[name](capi.Precond, RP, ci, vals)
        assert str(e.value) == text


@pytest.mark.parametrize("short", sorted(SHORT))
@pytest.mark.parametrize("name", sorted(HOST_HELPERS))
def test_short_arrays_raise_the_same_text_from_every_host_helper_before_the_library_loads(monkeypatch, name, short):
    ci, va, text = SHORT[short]
    _no_library(monkeypatch)
    with pytest.raises(ValueError) as e:
        HOST_HELPERS[name](RP, ci, va)
    assert str(e.value) == text


def test_amg_block_refuses_an_unknown_setup_string():
    for build in (lambda: capi.Precond.amg_block(MATRIX, RP, CI, VA, 2, setup="nope"),
                  lambda: capi.Precond.amg_block_from_device(MATRIX, N, None, None, None, 2, setup="nope")):
        with pytest.raises(ValueError) as e:
            build()
        assert str(e.value) == "setup = 'nope': one of ['mis2', 'plain', 'smoothed']"


def _matrix(nrows=N, ncols=N):
    """a CvrMatrix without a handle: enough for the checks its methods make before their C call"""
    A = capi.CvrMatrix.__new__(capi.CvrMatrix)
    A._h, A.nrows, A.ncols, A.f32, A.dtype = C.c_void_p(), nrows, ncols, False, np.float64
    return A


def test_which_raises_the_same_text_from_eigsh_host_and_lobpcg_host():
    A = _matrix()
    for call in (lambda: A.eigsh_host(1, which="XX"), lambda: A.lobpcg_host(np.ones((N, 2)), which="XX")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "which = 'XX': must be 'LA' or 'SA'"
    assert A._eig_options(1, "LA", 0, 1e-8, 100).which == capi.EIG_LARGEST and A._lobpcg_options(1, "SA", 1e-8, 200).which == capi.EIG_SMALLEST


def test_short_vectors_raise_their_texts(monkeypatch):
    A = _matrix(N, 3)
    for text, call in (("v0 is shorter than nrows", lambda: A.eigsh_host(1, v0=np.ones(N - 1))),          # (behind the options: the library is loaded)
                       ("v0 is shorter than ncols", lambda: A.svds_host(A, v0=np.ones(2)))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    _no_library(monkeypatch)
    b = np.ones(N)
    for text, call in (("b is shorter than nrows", lambda: A.cg_host(b[:3])), ("x0 is shorter than nrows", lambda: A.cg_host(b, x0=b[:3])),
                       ("x0 is shorter than nrows", lambda: A.minres_host(b, x0=b[:3])), ("b is shorter than nrows", lambda: A.lsqr_host(A, b[:3])),
                       ("x0 is shorter than ncols", lambda: A.lsqr_host(A, b, x0=b[:2]))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    bb, x = A._host_vectors(b, b)
    assert bb.dtype == x.dtype == np.float64 and len(x) == N and x is not b


DEV = (-1, None, None, None)          # a device view of a negative size: every kind refuses it in its argument checks
FAILING = [("cvr_precond_block_jacobi", lambda P: P.block_jacobi(RP, CI, VA, 0)),
           ("cvr_precond_block_jacobi", lambda P: P.block_jacobi_from_device(*DEV, 2)),
           ("cvr_precond_chebyshev", lambda P: P.chebyshev(MATRIX, 0, 1.0, 2.0)),
           ("cvr_precond_ilu0", lambda P: P.ilu0_from_device(*DEV)),
           ("cvr_precond_ilu0_jacobi", lambda P: P.ilu0_jacobi(RP, CI, VA, 0)),
           ("cvr_precond_ilu0_jacobi", lambda P: P.ilu0_jacobi_from_device(*DEV, 2)),
           ("cvr_precond_mcsgs", lambda P: P.mcsgs_from_device(*DEV)),
           ("cvr_precond_fsai", lambda P: P.fsai_from_device(*DEV)),
           ("cvr_precond_amg", lambda P: P.amg(MATRIX, RP, CI, VA, sweeps=0)),
           ("cvr_precond_amg", lambda P: P.amg_from_device(MATRIX, *DEV)),
           ("cvr_precond_amg_smoothed", lambda P: P.amg_smoothed(MATRIX, RP, CI, VA, omega=5.0)),
           ("cvr_precond_amg_smoothed", lambda P: P.amg_smoothed_from_device(MATRIX, *DEV)),
           ("cvr_precond_amg_mis2", lambda P: P.amg_mis2(MATRIX, RP, CI, VA, omega=5.0)),
           ("cvr_precond_amg_mis2", lambda P: P.amg_mis2_from_device(MATRIX, *DEV)),
           ("cvr_precond_amg_block", lambda P: P.amg_block(MATRIX, RP, CI, VA, 0)),
           ("cvr_precond_amg_block", lambda P: P.amg_block(MATRIX, RP, CI, VA, 2, setup="smoothed", omega=5.0)),
           ("cvr_precond_amg_block", lambda P: P.amg_block_from_device(MATRIX, *DEV, 2)),
           ("cvr_precond_amg_block", lambda P: P.amg_block_from_device(MATRIX, *DEV, 2, setup="mis2")),
           ("cvr_precond_amg_block", lambda P: P.amg_block_from_device(MATRIX, *DEV, 2, setup=capi.AMG_SETUP_SMOOTHED))]


@pytest.mark.parametrize("case", range(len(FAILING)))
def test_a_failing_build_leaves_p_null_and_names_the_entry_called(case):
    entry, build = FAILING[case]
    made = []

    class Spy(capi.Precond):
        def __init__(self):
            super().__init__()
            made.append(self)

    with pytest.raises(capi.CvrError) as e:
        build(Spy)
    assert e.value.code == capi.ERR_INVALID and str(e.value).startswith(entry + ": error -1: "), str(e.value)
    assert len(made) == 1 and isinstance(made[0]._p, C.c_void_p) and not made[0]._p
    assert not hasattr(made[0], "dtype") and not hasattr(made[0], "_matrix")          # (nothing behind the failed call ran)
    made[0].close()          # a no-op on the null object
